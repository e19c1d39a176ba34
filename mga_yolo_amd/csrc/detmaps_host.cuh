// Host side of detmaps.cuh for api_det.hip and api_nms.hip: what the maps of a descriptor are refused for, and the DetMaps the kernels get.  The
// callers check their own fields and call these where each refusal has always come: several faults are refused for the same one as before.
#pragma once
#include "host.cuh"
#include "detmaps.cuh"
#include "../../include/mgatargets.h"       // MGACBAM_E_ARG

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
