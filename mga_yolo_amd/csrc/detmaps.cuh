// The Detect head's maps as the kernels see them: level l is (B, 64 + nc, H_l, W_l) -- four box sides of kMapsReg bins, then nc class logits --
// over up to kMapsLevelsMax levels.  The anchors are the cells' centres, numbered level after level and row-major within one; a box side is the
// softmax expectation over its bins, in grid units.  The ONE definition of that input: the criterion (det.cuh) and the post-process (nms.cuh)
// hold a DetMaps and decode through these functions, so validation decodes exactly the boxes the criterion assigned on.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kMapsLevelsMax = 4;              // = MGADET_MAX_LEVELS = MGANMS_MAX_LEVELS (api_det.hip and api_nms.hip assert it)
constexpr int kMapsReg = 16;                   // bins per box side

struct DetMaps {
  const void* feat[kMapsLevelsMax];            // (B, 64 + nc, H_l, W_l)
  int H[kMapsLevelsMax], W[kMapsLevelsMax];
  int a0[kMapsLevelsMax + 1];                  // anchors [a0[l], a0[l+1]) belong to level l
  float stride[kMapsLevelsMax];
  int n_levels, B, nc, no, A;                  // no = 4 * kMapsReg + nc channels; A anchors per image
};
struct DetBox { float x1, y1, x2, y2; };

__device__ __forceinline__ int maps_level(const DetMaps& m, int a) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < kMapsLevelsMax; ++i)
    if (i < m.n_levels && a >= m.a0[i]) l = i;
  return l;
}
// an anchor: its level, its cell's index in the level, its centre in grid units, the level's stride and plane size; from the cell (x = p % W,
// y = p / W) or from the anchor index
struct MapsAnchor { int l, p; float ax, ay, s; size_t hw; };
__device__ __forceinline__ MapsAnchor maps_cell(const DetMaps& m, int l, int p, int y, int x) {
  return MapsAnchor{l, p, static_cast<float>(x) + 0.5f, static_cast<float>(y) + 0.5f, m.stride[l], static_cast<size_t>(m.H[l]) * m.W[l]};
}
__device__ __forceinline__ MapsAnchor maps_anchor(const DetMaps& m, int a) {
  const int l = maps_level(m, a), p = a - m.a0[l];
  return maps_cell(m, l, p, p / m.W[l], p % m.W[l]);
}
// image b's channel 0 at the anchor, in elements from the level's start; channel c lies c * hw further on
__device__ __forceinline__ size_t maps_offset(const DetMaps& m, const MapsAnchor& t, int b) { return static_cast<size_t>(b) * m.no * t.hw + t.p; }
template <typename T>
__device__ __forceinline__ const T* maps_feat(const DetMaps& m, const MapsAnchor& t, int b) {
  return static_cast<const T*>(m.feat[t.l]) + maps_offset(m, t, b);
}
// one side's bins of an anchor: softmax probabilities, their expectation (loss.py:238, head.py: DFL) and the log of the sum of exponentials
template <typename T>
__device__ __forceinline__ void maps_side(const T* __restrict__ f, size_t hw, int side, float (&p)[kMapsReg], float& d, float& lse) {
  float m = -FLT_MAX;
#pragma unroll
  for (int j = 0; j < kMapsReg; ++j) { p[j] = to_f32<T>(f[(side * kMapsReg + j) * hw]); m = fmaxf(m, p[j]); }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < kMapsReg; ++j) { p[j] = expf(p[j] - m); sum += p[j]; }
  const float inv = 1.f / sum;
  d = 0.f;
#pragma unroll
  for (int j = 0; j < kMapsReg; ++j) { p[j] *= inv; d += p[j] * static_cast<float>(j); }
  lse = m + logf(sum);
}
// the expectation alone; the post-process decodes with four of these in one expression, which keeps every side's loads in flight at once
template <typename T>
__device__ __forceinline__ float maps_dist(const T* __restrict__ f, size_t hw, int side) {
  float p[kMapsReg], d, lse;
  maps_side<T>(f, hw, side, p, d, lse);
  return d;
}
// the decoded box of the anchor at (ax, ay), in grid units (tal.py:382-391), a side after the other: the criterion's form
template <typename T>
__device__ __forceinline__ DetBox maps_decode(const T* __restrict__ f, size_t hw, float ax, float ay) {
  float p[kMapsReg], d[4], lse;
#pragma unroll
  for (int s = 0; s < 4; ++s) maps_side<T>(f, hw, s, p, d[s], lse);
  return DetBox{ax - d[0], ay - d[1], ax + d[2], ay + d[3]};
}

}  // namespace mgacbam
