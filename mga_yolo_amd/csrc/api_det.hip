// libmgacbam.so, C ABI (include/mgadet.h): the detection criterion -- task-aligned assignment, CIoU, DFL, BCE -- on the Detect maps
#include "detmaps_host.cuh"
#include "det.cuh"

#include "../../include/ext/mgamaps.h"        // mgadet.h, and the entry points that take the maps' layout

static_assert(kMapsLevelsMax == MGADET_MAX_LEVELS && kDetTopkMax == MGADET_MAX_TOPK && kDetMMax == MGADET_MAX_GT, "DetArgs against the ABI");
static_assert(kDetMMax <= kDetSlotMask, "a slot fits under the resolve's action bits");
static_assert(sizeof(mgadet_desc_t) == 256, "the descriptor's layout (mirrored by _lib.DetDesc)");

// ws, in the order it is carved
struct DetLayout { size_t cand_n, cand_row, cand_anchor, cand_metric, cand_overlap, tss_part, ovf, partial, fin, total; };

// Everything a descriptor is checked for that does not involve a pointer; fills the kernel arguments' geometry and the ws layout.
static int det_check(const char* what, const mgadet_desc_t* D, DetArgs& A, DetLayout& L) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (int e = maps_levels(what, 1, D->n_levels)) return e;
  if (int e = check_dtype(what, D->dtype)) return e;
  if (D->reg_max != kMapsReg) return fail(MGACBAM_E_ARG, "%s: reg_max=%d (16 is the one built)", what, D->reg_max);
  if (D->topk < 1 || D->topk > MGADET_MAX_TOPK) return fail(MGACBAM_E_ARG, "%s: topk=%d (1 .. %d)", what, D->topk, MGADET_MAX_TOPK);
  if (int e = labels_caps(what, D->m_cap, D->reserved)) return e;
  if (D->n_cap < 0) return fail(MGACBAM_E_SHAPE, "%s: n_cap=%d", what, D->n_cap);
  if (int e = maps_check(what, D->n_levels, D->H, D->W, D->stride, D->B, D->nc, true, A.maps)) return e;
  if (static_cast<long long>(D->W[0]) * D->stride[0] > (1 << 24) || static_cast<long long>(D->H[0]) * D->stride[0] > (1 << 24))
    return fail(MGACBAM_E_SHAPE, "%s: an image side above 2^24 pixels", what);
  A.topk = D->topk; A.m_cap = D->m_cap;
  for (int k = 0; k < 3; ++k) A.gain[k] = D->gains[k];
  A.img_w = static_cast<float>(D->W[0] * D->stride[0]); A.img_h = static_cast<float>(D->H[0] * D->stride[0]);
  A.nblk = static_cast<int>((static_cast<long long>(D->B) * A.maps.A + kBlock - 1) / kBlock);
  const size_t slots = static_cast<size_t>(D->B) * D->m_cap;
  Carver cv;
  L.cand_n = cv.take(slots); L.cand_row = cv.take(slots);
  L.cand_anchor = cv.take(slots * kDetTopkMax); L.cand_metric = cv.take(slots * kDetTopkMax); L.cand_overlap = cv.take(slots * kDetTopkMax);
  L.tss_part = cv.take(D->B); L.ovf = cv.take(D->B);
  L.partial = cv.take(static_cast<size_t>(A.nblk) * 3);
  L.fin = cv.take(4);
  L.total = cv.total;
  return 0;
}

extern "C" size_t mgadet_ws_bytes(const mgadet_desc_t* desc) {
  DetArgs A;
  DetLayout L;
  if (det_check("mgadet_ws_bytes", desc, A, L)) return 0;
  g_err[0] = 0;
  return L.total;
}

// the pointers of a call; bwd: g_feats and upstream as well
static int det_bind(const char* what, const mgadet_desc_t* D, DetArgs& A, const DetLayout& L, bool bwd) {
  if (int e = maps_bind(what, D->feats, bwd ? D->g_feats : nullptr, D->dtype, A.maps)) return e;
  for (int l = 0; l < kMapsLevelsMax; ++l) A.gfeat[l] = bwd && l < D->n_levels ? D->g_feats[l] : nullptr;
  if (D->n_cap > 0 && (!D->batch_idx || !D->cls || !D->bboxes)) return fail(MGACBAM_E_NULL, "%s: a label buffer is NULL with n_cap=%d", what, D->n_cap);
  if (!D->assign_gt || !D->assign_score || !D->out || !D->items || !D->status || !D->ws || (bwd && !D->upstream))
    return fail(MGACBAM_E_NULL, "%s: assign_gt, assign_score, out, items, status, ws%s must not be NULL", what, bwd ? ", upstream" : "");
  const void* words[] = {D->batch_idx, D->cls, D->bboxes, D->n, D->assign_gt, D->assign_score, D->out, D->items, D->status, D->upstream};
  if (int e = check_words_and_ws(what, words, D->ws, L.total, D->ws_bytes)) return e;
  A.labels = LabelBatch{D->batch_idx, D->cls, D->bboxes, D->n, D->n_cap};
  A.asg_gt = D->assign_gt; A.asg_score = D->assign_score;
  A.cand_n = at<int>(D->ws, L.cand_n); A.cand_row = at<int>(D->ws, L.cand_row); A.cand_anchor = at<int>(D->ws, L.cand_anchor);
  A.cand_metric = at(D->ws, L.cand_metric); A.cand_overlap = at(D->ws, L.cand_overlap);
  A.tss_part = at(D->ws, L.tss_part); A.ovf = at<int>(D->ws, L.ovf); A.partial = at(D->ws, L.partial); A.fin = at(D->ws, L.fin);
  A.out = D->out; A.items = D->items; A.status = D->status; A.upstream = D->upstream;
  return 0;
}

template <typename T, MapsLayout L>
static int det_forward(const DetArgs& A, hipStream_t st) {
  const size_t E = static_cast<size_t>(A.m_cap) * kDetTopkMax;
  const size_t smem = E * 14 + static_cast<size_t>(A.m_cap) * 12;       // k_det_resolve: e_anc, e_met, e_ov, e_gt; pos_m, pos_o, s_row
  if (int e = launch("k_det_assign", k_det_assign<T, L>, static_cast<long long>(A.maps.B) * A.m_cap, kBlock, 0, st, A)) return e;
  if (int e = launch("k_det_resolve", k_det_resolve<T, L>, A.maps.B, kBlock, smem, st, A)) return e;
  if (int e = launch("k_det_loss", k_det_loss<T, L>, A.nblk, kBlock, 0, st, A)) return e;
  return launch("k_det_final", k_det_final, 1, kBlock, 0, st, A);
}

// the maps' layout as a tag for the kernels' template parameter (host.cuh: with_elem's way)
template <MapsLayout L> using LayoutTag = std::integral_constant<MapsLayout, L>;
template <typename F>
static auto with_layout(bool nhwc, F f) { return nhwc ? f(LayoutTag<MapsLayout::kNHWC>{}) : f(LayoutTag<MapsLayout::kNCHW>{}); }

// either direction: check, bind, launch in the maps' element type and layout.  flags: 0 (mgadet_*) or MGAMAPS_LAYOUT_NHWC.  The layout changes
// no check and no size: the maps hold the same elements, aligned to the element, in either.
static int det_run(const char* what, const mgadet_desc_t* D, int32_t flags, void* stream, bool bwd) {
  if (flags & ~MGAMAPS_LAYOUT_NHWC) return fail(MGACBAM_E_ARG, "%s: flags=0x%x (0 or MGAMAPS_LAYOUT_NHWC)", what, flags);
  DetArgs A;
  DetLayout L;
  if (int e = det_check(what, D, A, L)) return e;
  if (int e = det_bind(what, D, A, L, bwd)) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  const int e = with_elem(D->dtype, [&](auto t) {
    return with_layout(flags & MGAMAPS_LAYOUT_NHWC, [&](auto l) {
      using T = elem_t<decltype(t)>;
      constexpr MapsLayout kL = decltype(l)::value;
      return bwd ? launch("k_det_bwd", k_det_bwd<T, kL>, A.nblk, kBlock, 0, st, A) : det_forward<T, kL>(A, st);
    });
  });
  if (!e) g_err[0] = 0;
  return e;
}
extern "C" int mgadet_forward(const mgadet_desc_t* D, void* stream) { return det_run("mgadet_forward", D, 0, stream, false); }
extern "C" int mgadet_backward(const mgadet_desc_t* D, void* stream) { return det_run("mgadet_backward", D, 0, stream, true); }
extern "C" int mgamaps_det_forward(const mgadet_desc_t* D, int32_t flags, void* stream) { return det_run("mgamaps_det_forward", D, flags, stream, false); }
extern "C" int mgamaps_det_backward(const mgadet_desc_t* D, int32_t flags, void* stream) { return det_run("mgamaps_det_backward", D, flags, stream, true); }
