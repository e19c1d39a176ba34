// libmgacbam.so, C ABI (include/ext/mgaap.h): average precision per class from the accumulated rows, in 3 + 3 * passes + 7 * niou launches
#include "detmaps_host.cuh"
#include "ap.cuh"

#include "../../include/ext/mgamatch.h"
#include "../../include/ext/mgaap.h"

static_assert(kApTile == MGAAP_TILE && kApPoints == MGAAP_AP_POINTS && kApCurve == MGAAP_CURVE_POINTS, "ApArgs against the ABI");
static_assert(MGAAP_MAX_NC == kApMaxNc, "k_ap_keys counts the classes in static LDS");
static_assert(MGAAP_MAX_NC <= kApScanBlock, "k_ap_starts scans the classes with one thread each");
static_assert(sizeof(mgaap_desc_t) == 128, "the descriptor's layout (mirrored by _lib.ApDesc)");

static int ap_class_passes(int nc) { return nc <= 1 ? 0 : (nc <= 256 ? 1 : 2); }

// Everything a descriptor is checked for that does not involve a pointer's value; fills the kernel arguments' geometry and the ws size.
static int ap_check(const char* what, const mgaap_desc_t* D, ApArgs& A, size_t (&off)[12], size_t& ws_total) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (D->niou < 1 || D->niou > MGAMATCH_MAX_IOU) return fail(MGACBAM_E_ARG, "%s: niou=%d (1 .. %d)", what, D->niou, MGAMATCH_MAX_IOU);
  if (D->nc < 1 || D->nc > MGAAP_MAX_NC) return fail(MGACBAM_E_ARG, "%s: nc=%d (1 .. %d)", what, D->nc, MGAAP_MAX_NC);
  if (D->reserved != 0) return fail(MGACBAM_E_ARG, "%s: reserved=%d (0)", what, D->reserved);
  const long long limit = (1ll << 31) / D->niou;
  if (D->rows_cap < 1 || D->tgt_cap < 1 || D->rows_cap >= limit || D->tgt_cap >= limit)
    return fail(MGACBAM_E_SHAPE, "%s: rows_cap=%d tgt_cap=%d (1 .. 2^31 / niou - 1 = %lld)", what, D->rows_cap, D->tgt_cap, limit - 1);
  A.rows_cap = D->rows_cap; A.tgt_cap = D->tgt_cap; A.niou = D->niou; A.nc = D->nc;
  const size_t rows = static_cast<size_t>(D->rows_cap), tiles = (rows + kApTile - 1) / kApTile;
  Carver cv;
  off[0] = cv.take(8);                                         // ctl
  off[1] = cv.take(static_cast<size_t>(D->nc) + 2);            // starts
  for (int k = 2; k < 8; ++k) off[k] = cv.take(rows);          // ckey[0], ckey[1], pay[0], pay[1], clskey, S
  off[8] = cv.take(2 * rows);                                  // env (fp64)
  off[9] = cv.take(256 * tiles);                               // table
  off[10] = cv.take(tiles);                                    // tpagg
  off[11] = cv.take(8 * tiles);                                // envagg, envcarry
  ws_total = cv.total;
  return 0;
}

extern "C" size_t mgaap_ws_bytes(const mgaap_desc_t* desc) {
  ApArgs A;
  size_t off[12], total;
  if (ap_check("mgaap_ws_bytes", desc, A, off, total)) return 0;
  g_err[0] = 0;
  return total;
}

static int ap_bind(const char* what, const mgaap_desc_t* D, ApArgs& A, const size_t (&off)[12], size_t ws_total) {
  if (!D->rows_tp || !D->rows_conf || !D->rows_cls || !D->tgt_cls || !D->state || !D->grid_ap || !D->grid_curve || !D->result || !D->status || !D->ws)
    return fail(MGACBAM_E_NULL, "%s: rows_tp, rows_conf, rows_cls, tgt_cls, state, grid_ap, grid_curve, result, status, ws must not be NULL", what);
  if (!aligned_to(D->grid_ap, 8) || !aligned_to(D->grid_curve, 8) || !aligned_to(D->result, 8))
    return fail(MGACBAM_E_ALIGN, "%s: grid_ap, grid_curve, result (fp64) must be 8-byte aligned", what);
  const void* words[] = {D->rows_conf, D->rows_cls, D->rows_img, D->tgt_cls, D->tgt_img, D->state, D->status};
  if (int e = check_words_and_ws(what, words, D->ws, ws_total, D->ws_bytes)) return e;
  A.rows_tp = D->rows_tp; A.rows_conf = D->rows_conf; A.rows_cls = D->rows_cls; A.tgt_cls = D->tgt_cls; A.state = D->state;
  A.grid_ap = D->grid_ap; A.grid_curve = D->grid_curve; A.status = D->status;
  const size_t nc = static_cast<size_t>(D->nc);
  A.ap = static_cast<double*>(D->result);
  A.p_curve = A.ap + nc * D->niou; A.r_curve = A.p_curve + nc * kApCurve; A.prec_values = A.r_curve + nc * kApCurve;
  A.nt = reinterpret_cast<int*>(A.prec_values + nc * kApCurve); A.n_det = A.nt + nc;
  A.ctl = at<int>(D->ws, off[0]); A.starts = at<int>(D->ws, off[1]);
  A.ckey[0] = at<unsigned>(D->ws, off[2]); A.ckey[1] = at<unsigned>(D->ws, off[3]);
  A.pay[0] = at<unsigned>(D->ws, off[4]); A.pay[1] = at<unsigned>(D->ws, off[5]);
  A.clskey = at<unsigned>(D->ws, off[6]); A.S = at<int>(D->ws, off[7]); A.env = at<double>(D->ws, off[8]);
  A.table = at<int>(D->ws, off[9]); A.tpagg = at<int>(D->ws, off[10]);
  const size_t tiles = (static_cast<size_t>(D->rows_cap) + kApTile - 1) / kApTile;
  A.envagg = at<int4>(D->ws, off[11]); A.envcarry = A.envagg + tiles;
  return 0;
}

extern "C" int mgaap_run(const mgaap_desc_t* D, void* stream) {
  const char* what = "mgaap_run";
  ApArgs A;
  size_t off[12], ws_total;
  if (int e = ap_check(what, D, A, off, ws_total)) return e;
  if (int e = ap_bind(what, D, A, off, ws_total)) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const long long tiles = (static_cast<long long>(A.rows_cap) + kApTile - 1) / kApTile;
  const long long most = std::max(A.rows_cap, A.tgt_cap);
  if (int e = launch("k_ap_init", k_ap_init, 1, kBlock, 0, st, A)) return e;
  if (int e = launch("k_ap_keys", k_ap_keys, std::min<long long>((most + kBlock - 1) / kBlock, 2048), kBlock, 0, st, A)) return e;
  if (int e = launch("k_ap_starts", k_ap_starts, 1, kApScanBlock, 0, st, A)) return e;
  int src = 0;
  const int passes = 4 + ap_class_passes(A.nc);
  for (int p = 0; p < passes; ++p, src ^= 1) {
    const ApPass P{src, p < 4 ? 8 * p : 8 * (p - 4), p >= 4};
    if (int e = launch("k_ap_hist", k_ap_hist, tiles, kBlock, 0, st, A, P)) return e;
    if (int e = launch("k_ap_scan", k_ap_scan, 1, kApScanBlock, 0, st, A)) return e;
    if (int e = launch("k_ap_scatter", k_ap_scatter, tiles, kBlock, 0, st, A, P)) return e;
  }
  for (int t = 0; t < A.niou; ++t) {
    const ApCol C{src, t};
    if (int e = launch("k_ap_tp_reduce", k_ap_tp_reduce, tiles, kBlock, 0, st, A, C)) return e;
    if (int e = launch("k_ap_tp_scan", k_ap_tp_scan, 1, kApScanBlock, 0, st, A)) return e;
    if (int e = launch("k_ap_tp_apply", k_ap_tp_apply, tiles, kBlock, 0, st, A, C)) return e;
    if (int e = launch("k_ap_env_reduce", k_ap_env_reduce, tiles, kBlock, 0, st, A, C)) return e;
    if (int e = launch("k_ap_env_scan", k_ap_env_scan, 1, kBlock, 0, st, A)) return e;
    if (int e = launch("k_ap_env_apply", k_ap_env_apply, tiles, kBlock, 0, st, A, C)) return e;
    if (int e = launch("k_ap_curves", k_ap_curves, A.nc, kBlock, 0, st, A, C)) return e;
  }
  g_err[0] = 0;
  return 0;
}
