// Host side of detmaps.cuh and labels.cuh for api_det.hip, api_nms.hip, api_match.hip and api_confusion.hip: what the maps and the labels of a
// descriptor are refused for, with the codes and texts each entry point has always given, and the DetMaps / LabelBatch the kernels get.  The
// callers check their own fields and call the maps' checks where each refusal has always come: several faults are refused for the same one.
#pragma once
#include "host.cuh"
#include "detmaps.cuh"
#include "labels.cuh"
#include "../../include/mgadet.h"           // MGADET_MAX_GT; mgatargets.h: MGACBAM_E_ARG
#include <math.h>

static int maps_levels(const char* what, int min_levels, int n_levels) {     // the level count: a descriptor's first refusal after a NULL one
  if (n_levels >= min_levels && n_levels <= kMapsLevelsMax) return 0;
  return fail(MGACBAM_E_LEVELS, "%s: n_levels=%d (%d .. %d)", what, n_levels, min_levels, kMapsLevelsMax);
}
// B, nc, then level by level the shape, the stride and the running anchor count -- which, times B where per_batch is set, stays below
// 2^31 --; then the kernel arguments' geometry (m.A: the levels' anchors): the unused levels zero, no pointer set.  n_levels has passed maps_levels.
static int maps_check(const char* what, int n_levels, const int32_t* H, const int32_t* W, const int32_t* stride, int B, int nc, bool per_batch, DetMaps& m) {
  if (B < 1 || nc < 1 || nc > 65536) return fail(MGACBAM_E_SHAPE, "%s: B=%d nc=%d", what, B, nc);
  long long anchors = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (H[l] < 1 || W[l] < 1) return fail(MGACBAM_E_SHAPE, "%s: level %d is %d x %d", what, l, H[l], W[l]);
    if (stride[l] < 1 || (l > 0 && stride[l] <= stride[l - 1]))
      return fail(MGACBAM_E_ARG, "%s: stride[%d]=%d (positive, strictly ascending)", what, l, stride[l]);
    anchors += static_cast<long long>(H[l]) * W[l];
    if (anchors * (per_batch ? B : 1) >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: %sanchors must stay below 2^31", what, per_batch ? "B * " : "");
  }
  m.n_levels = n_levels; m.B = B; m.nc = nc; m.no = 4 * kMapsReg + nc; m.A = static_cast<int>(anchors); m.a0[0] = 0;
  for (int l = 0; l < kMapsLevelsMax; ++l) {
    const bool on = l < n_levels;
    m.H[l] = on ? H[l] : 0; m.W[l] = on ? W[l] : 0; m.stride[l] = on ? static_cast<float>(stride[l]) : 0.f;
    m.a0[l + 1] = m.a0[l] + m.H[l] * m.W[l]; m.feat[l] = nullptr;
  }
  return 0;
}
// the maps' pointers, level by level: not NULL, aligned to the element; g_feats (or nullptr): the criterion's gradient maps, held to the same
static int maps_bind(const char* what, const void* const* feats, void* const* g_feats, int dtype, DetMaps& m) {
  const size_t es = elem_size(dtype);
  for (int l = 0; l < m.n_levels; ++l) {
    if (!feats[l] || (g_feats && !g_feats[l])) return fail(MGACBAM_E_NULL, "%s: level %d's feats%s is NULL", what, l, g_feats ? " or g_feats" : "");
    if (!aligned_to(feats[l], es) || (g_feats && !aligned_to(g_feats[l], es)))
      return fail(MGACBAM_E_ALIGN, "%s: level %d must be aligned to its element (%zu bytes)", what, l, es);
    m.feat[l] = feats[l];
  }
  return 0;
}
// the tail of a bind: every fp32 / int32 buffer 4-byte aligned (NULL, an optional one, passes), ws 16-byte aligned and large enough
template <size_t N>
static int check_words_and_ws(const char* what, const void* const (&words)[N], const void* ws, size_t want, size_t got) {
  for (const void* p : words)
    if (!aligned_to(p, 4)) return fail(MGACBAM_E_ALIGN, "%s: every fp32 / int32 buffer must be 4-byte aligned", what);
  if (!aligned_to(ws, 16)) return fail(MGACBAM_E_ALIGN, "%s: ws must be 16-byte aligned", what);
  return check_capacity(what, "ws", want, got);
}
// the ground truths an image may have and the descriptor's reserved word: the three stages' descriptors alike
static int labels_caps(const char* what, int m_cap, int reserved) {
  if (m_cap < 1 || m_cap > MGADET_MAX_GT) return fail(MGACBAM_E_ARG, "%s: m_cap=%d (1 .. %d)", what, m_cap, MGADET_MAX_GT);
  if (reserved != 0) return fail(MGACBAM_E_ARG, "%s: reserved=%d (0)", what, reserved);
  return 0;
}
// a validation stage's geometry (the matching, the confusion matrix); the caller checks the fields of its own after it
static int labels_check(const char* what, int B, int max_det, int n_cap, int m_cap, int reserved, float img_w, float img_h) {
  if (B < 1 || max_det < 1 || n_cap < 0) return fail(MGACBAM_E_SHAPE, "%s: B=%d max_det=%d n_cap=%d", what, B, max_det, n_cap);
  if (static_cast<long long>(B) * max_det >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: B * max_det must stay below 2^31", what);
  if (n_cap >= (1 << 29)) return fail(MGACBAM_E_SHAPE, "%s: n_cap=%d must stay below 2^29 (the kernels index bboxes, 4 words a row, with int)", what, n_cap);
  if (int e = labels_caps(what, m_cap, reserved)) return e;
  if (!(img_w > 0.f && img_h > 0.f) || !isfinite(img_w) || !isfinite(img_h))
    return fail(MGACBAM_E_ARG, "%s: img_w=%g img_h=%g (positive and finite)", what, img_w, img_h);
  return 0;
}
// the labels' pointers, NULL only with n_cap = 0; also: a buffer of the caller's under the same rule, as the text names it (", lab_out")
template <typename Desc>
static int labels_bind(const char* what, const Desc* D, LabelBatch& L, const char* also = "", bool also_null = false) {
  if (D->n_cap > 0 && (!D->batch_idx || !D->cls || !D->bboxes || also_null))
    return fail(MGACBAM_E_NULL, "%s: batch_idx, cls, bboxes%s must not be NULL with n_cap=%d", what, also, D->n_cap);
  L = LabelBatch{D->batch_idx, D->cls, D->bboxes, D->n, D->n_cap};
  return 0;
}
