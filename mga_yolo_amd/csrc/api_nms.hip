// libmgacbam.so, C ABI (include/mganms.h): the detection post-process -- Detect decode, candidates, greedy NMS -- in two launches
#include "detmaps_host.cuh"
#include "nms.cuh"

#include "../../include/ext/mgamaps.h"        // mganms.h, and the entry point that takes the maps' layout

static_assert(kMapsLevelsMax == MGANMS_MAX_LEVELS, "NmsArgs against the ABI");
static_assert(kBlock == 256, "k_nms_greedy's radix select has one bin per thread");
static_assert(sizeof(mganms_desc_t) == 184, "the descriptor's layout (mirrored by _lib.NmsDesc)");

// ws, in the order it is carved
struct NmsLayout { size_t cnt, keys, boxes, total; };

// Everything a descriptor is checked for that does not involve a pointer's value; fills the kernel arguments' geometry and the ws layout.
static int nms_check(const char* what, const mganms_desc_t* D, NmsArgs& A, NmsLayout& L) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (int e = maps_levels(what, 0, D->n_levels)) return e;                     // 0 with pred, 1 .. with feats
  bool any_feat = false;
  for (int l = 0; l < MGANMS_MAX_LEVELS; ++l) any_feat = any_feat || D->feats[l] != nullptr;
  if (int e = check_dtype(what, D->dtype)) return e;
  if (D->n_levels > 0 ? D->pred != nullptr : any_feat)
    return fail(MGACBAM_E_ARG, "%s: exactly one of feats (n_levels >= 1) and pred (n_levels = 0) is given", what);
  if (!(D->conf_thres >= 0.f && D->conf_thres <= 1.f) || !(D->iou_thres >= 0.f && D->iou_thres <= 1.f))
    return fail(MGACBAM_E_ARG, "%s: conf_thres=%g iou_thres=%g (both in [0, 1])", what, D->conf_thres, D->iou_thres);
  if (D->max_det < 1 || D->max_nms < 1 || D->cand_cap < 1) return fail(MGACBAM_E_ARG, "%s: max_det=%d max_nms=%d cand_cap=%d (all >= 1)", what, D->max_det, D->max_nms, D->cand_cap);
  if (D->flags & ~(MGANMS_MULTI_LABEL | MGANMS_AGNOSTIC)) return fail(MGACBAM_E_ARG, "%s: flags=0x%x", what, D->flags);
  if (D->reserved != 0) return fail(MGACBAM_E_ARG, "%s: reserved=%d (0)", what, D->reserved);
  if (D->A < 0) return fail(MGACBAM_E_SHAPE, "%s: A=%d", what, D->A);
  if (int e = maps_check(what, D->n_levels, D->H, D->W, D->stride, D->B, D->nc, false, A.maps)) return e;
  if (D->n_levels > 0 && D->A != 0 && D->A != A.maps.A) return fail(MGACBAM_E_SHAPE, "%s: A=%d, the levels hold %d anchors", what, D->A, A.maps.A);
  if (D->n_levels == 0) A.maps.A = D->A;                                       // with pred: the descriptor's
  const long long anchors = A.maps.A;
  if (anchors < 1) return fail(MGACBAM_E_SHAPE, "%s: A=%lld", what, anchors);
  if (anchors * D->nc >= (1ll << 31) || anchors * D->B >= (1ll << 31))
    return fail(MGACBAM_E_SHAPE, "%s: A * nc and B * A must stay below 2^31", what);
  A.bpi = (A.maps.A + kBlock - 1) / kBlock;
  A.pred = nullptr;
  A.conf = D->conf_thres; A.iou = D->iou_thres; A.max_det = D->max_det; A.max_nms = D->max_nms; A.cand_cap = D->cand_cap;
  A.multi = (D->flags & MGANMS_MULTI_LABEL) && D->nc > 1 ? 1 : 0;              // ops.py:266
  A.agnostic = D->flags & MGANMS_AGNOSTIC ? 1 : 0;
  const size_t slots = static_cast<size_t>(D->B) * D->cand_cap;
  Carver cv;
  L.cnt = cv.take(D->B); L.keys = cv.take(slots * 2); L.boxes = cv.take(slots * 4);
  L.total = cv.total;
  return 0;
}

extern "C" size_t mganms_ws_bytes(const mganms_desc_t* desc) {
  NmsArgs A;
  NmsLayout L;
  if (nms_check("mganms_ws_bytes", desc, A, L)) return 0;
  g_err[0] = 0;
  return L.total;
}

static int nms_bind(const char* what, const mganms_desc_t* D, NmsArgs& A, const NmsLayout& L) {
  const size_t es = elem_size(D->dtype);
  if (int e = maps_bind(what, D->feats, nullptr, D->dtype, A.maps)) return e;
  if (D->n_levels == 0 && !D->pred) return fail(MGACBAM_E_NULL, "%s: pred is NULL with n_levels=0", what);
  if (D->pred && !aligned_to(D->pred, es)) return fail(MGACBAM_E_ALIGN, "%s: pred must be aligned to its element (%zu bytes)", what, es);
  A.pred = D->pred;
  if (!D->dets || !D->count || !D->keep || !D->status || !D->ws) return fail(MGACBAM_E_NULL, "%s: dets, count, keep, status, ws must not be NULL", what);
  const void* words[] = {D->dets, D->count, D->keep, D->status};
  if (int e = check_words_and_ws(what, words, D->ws, L.total, D->ws_bytes)) return e;
  A.cnt = at<int>(D->ws, L.cnt); A.keys = at<nms_key_t>(D->ws, L.keys); A.boxes = at<float4>(D->ws, L.boxes);
  A.dets = D->dets; A.count = D->count; A.keep = D->keep; A.status = D->status;
  return 0;
}

// flags: 0 (mganms_run) or MGAMAPS_LAYOUT_NHWC.  The layout changes no other check and no size; a decoded prediction has no NHWC form, which is
// refused last, so a descriptor with another fault is refused for that fault under either flags.
static int nms_run(const char* what, const mganms_desc_t* D, int32_t flags, void* stream) {
  if (flags & ~MGAMAPS_LAYOUT_NHWC) return fail(MGACBAM_E_ARG, "%s: flags=0x%x (0 or MGAMAPS_LAYOUT_NHWC)", what, flags);
  NmsArgs A;
  NmsLayout L;
  if (int e = nms_check(what, D, A, L)) return e;
  if (int e = nms_bind(what, D, A, L)) return e;
  const bool nhwc = flags & MGAMAPS_LAYOUT_NHWC;
  if (nhwc && D->pred) return fail(MGACBAM_E_ARG, "%s: MGAMAPS_LAYOUT_NHWC with pred: a decoded prediction is (B, 4 + nc, A)", what);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  auto cand = with_elem(D->dtype, [&](auto t) {
    using T = elem_t<decltype(t)>;
    return nhwc ? k_nms_cand<T, MapsLayout::kNHWC> : k_nms_cand<T, MapsLayout::kNCHW>;
  });
  if (int e = launch("k_nms_cand", cand, static_cast<long long>(A.maps.B) * A.bpi, kBlock, 0, st, A)) return e;
  if (int e = launch("k_nms_greedy", k_nms_greedy, A.maps.B, kBlock, 0, st, A)) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mganms_run(const mganms_desc_t* D, void* stream) { return nms_run("mganms_run", D, 0, stream); }
extern "C" int mgamaps_nms_run(const mganms_desc_t* D, int32_t flags, void* stream) { return nms_run("mgamaps_nms_run", D, flags, stream); }
