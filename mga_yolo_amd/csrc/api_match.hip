// libmgacbam.so, C ABI (include/ext/mgamatch.h): detections matched to labels for the validation metrics, in two launches
#include "detmaps_host.cuh"
#include "match.cuh"

#include "../../include/ext/mgamatch.h"

static_assert(kMatchMaxGt == MGADET_MAX_GT && kMatchMaxIou == MGAMATCH_MAX_IOU, "MatchArgs against the ABI");
static_assert(sizeof(mgamatch_desc_t) == 264, "the descriptor's layout (mirrored by _lib.MatchDesc)");

// Everything a descriptor is checked for that does not involve a pointer's value; fills the kernel arguments' geometry and the ws size.
static int match_check(const char* what, const mgamatch_desc_t* D, MatchArgs& A, size_t& ws_total) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (int e = labels_check(what, D->B, D->max_det, D->n_cap, D->m_cap, D->reserved, D->img_w, D->img_h)) return e;
  if (D->niou < 1 || D->niou > MGAMATCH_MAX_IOU) return fail(MGACBAM_E_ARG, "%s: niou=%d (1 .. %d)", what, D->niou, MGAMATCH_MAX_IOU);
  for (int t = 0; t < D->niou; ++t)
    if (!(D->iouv[t] > (t ? D->iouv[t - 1] : 0.f) && D->iouv[t] <= 1.f))
      return fail(MGACBAM_E_ARG, "%s: iouv[%d]=%g (strictly ascending, in (0, 1])", what, t, D->iouv[t]);
  if (D->flags & ~MGAMATCH_SINGLE_CLS) return fail(MGACBAM_E_ARG, "%s: flags=0x%x", what, D->flags);
  A.B = D->B; A.max_det = D->max_det; A.m_cap = D->m_cap; A.niou = D->niou;
  A.single_cls = D->flags & MGAMATCH_SINGLE_CLS ? 1 : 0;
  A.img_w = D->img_w; A.img_h = D->img_h;
  for (int t = 0; t < MGAMATCH_MAX_IOU; ++t) A.iouv[t] = t < D->niou ? D->iouv[t] : 2.f;
  A.rows_cap = D->rows_cap; A.tgt_cap = D->tgt_cap;
  Carver cv;
  cv.take(static_cast<size_t>(D->B) + 4);                                        // the images' overflow words, then state's snapshot
  ws_total = cv.total;
  return 0;
}

extern "C" size_t mgamatch_ws_bytes(const mgamatch_desc_t* desc) {
  MatchArgs A;
  size_t total;
  if (match_check("mgamatch_ws_bytes", desc, A, total)) return 0;
  g_err[0] = 0;
  return total;
}

static int match_bind(const char* what, const mgamatch_desc_t* D, MatchArgs& A, size_t ws_total) {
  if (!D->dets || !D->count || !D->tp || !D->best_iou || !D->best_gt || !D->status || !D->ws)
    return fail(MGACBAM_E_NULL, "%s: dets, count, tp, best_iou, best_gt, status, ws must not be NULL", what);
  if (int e = labels_bind(what, D, A.labels)) return e;
  const void* acc[] = {D->rows_tp, D->rows_conf, D->rows_cls, D->rows_img, D->tgt_cls, D->tgt_img, D->state};
  int given = 0;
  for (const void* p : acc) given += p != nullptr;
  if (given != 0 && given != 7)
    return fail(MGACBAM_E_NULL, "%s: rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state are given together or not at all (%d of 7)", what, given);
  if (given && (D->rows_cap < 1 || D->tgt_cap < 1)) return fail(MGACBAM_E_ARG, "%s: rows_cap=%d tgt_cap=%d (both >= 1 with the accumulation on)", what, D->rows_cap, D->tgt_cap);
  const void* words[] = {D->dets, D->count, D->batch_idx, D->cls, D->bboxes, D->n, D->best_iou, D->best_gt, D->rows_conf, D->rows_cls, D->rows_img,
                         D->tgt_cls, D->tgt_img, D->state, D->status};
  if (int e = check_words_and_ws(what, words, D->ws, ws_total, D->ws_bytes)) return e;
  A.dets = D->dets; A.count = D->count;
  A.tp = D->tp; A.best_iou = D->best_iou; A.best_gt = D->best_gt;
  A.rows_tp = D->rows_tp; A.rows_conf = D->rows_conf; A.rows_cls = D->rows_cls; A.rows_img = D->rows_img;
  A.tgt_cls = D->tgt_cls; A.tgt_img = D->tgt_img; A.state = D->state; A.status = D->status;
  A.over = at<int>(D->ws, 0); A.snap = A.over + D->B;
  return 0;
}

extern "C" int mgamatch_run(const mgamatch_desc_t* D, void* stream) {
  const char* what = "mgamatch_run";
  MatchArgs A;
  size_t ws_total;
  if (int e = match_check(what, D, A, ws_total)) return e;
  if (int e = match_bind(what, D, A, ws_total)) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = launch("k_match", k_match, A.B, kBlock, 0, st, A)) return e;
  const long long chunks = A.state ? A.B + (static_cast<long long>(A.labels.n_cap) + kBlock - 1) / kBlock : 1;   // without the accumulation: the status word alone
  if (int e = launch("k_match_append", k_match_append, chunks, kBlock, 0, st, A)) return e;
  g_err[0] = 0;
  return 0;
}
