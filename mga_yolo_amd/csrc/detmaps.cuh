// The Detect head's maps as the kernels see them: level l is (B, 64 + nc, H_l, W_l) -- four box sides of kMapsReg bins, then nc class logits --
// over up to kMapsLevelsMax levels.  The anchors are the cells' centres, numbered level after level and row-major within one; a box side is the
// softmax expectation over its bins, in grid units.  The ONE definition of that input: the criterion (det.cuh) and the post-process (nms.cuh)
// hold a DetMaps and decode through these functions, so validation decodes exactly the boxes the criterion assigned on.
//
// The layout in memory is a compile-time parameter of every accessor (MapsLayout): NCHW, channel c of an anchor lies c * H_l * W_l elements
// on, or NHWC (torch's channels_last), where an anchor's 64 + nc channels are one contiguous row and consecutive anchors lie `no` elements
// apart.  The arithmetic is written once against a reader (at(c): channel c as fp32; side(s, v): the 16 bins of side s), so both layouts
// compute the same expressions in the same order and give the same bits.  NEVER is a byte outside a level read or written: a vector access
// is made only where the row's own address is 16-byte aligned, no pointer is aligned down.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kMapsLevelsMax = 4;              // = MGADET_MAX_LEVELS = MGANMS_MAX_LEVELS (api_det.hip and api_nms.hip assert it)
constexpr int kMapsReg = 16;                   // bins per box side
enum class MapsLayout { kNCHW, kNHWC };

struct DetMaps {
  const void* feat[kMapsLevelsMax];            // (B, 64 + nc, H_l, W_l), or (B, H_l, W_l, 64 + nc) in memory
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
// image b's channel 0 at the anchor, in elements from the level's start; NCHW: channel c lies c * hw further on, NHWC: c
template <MapsLayout L = MapsLayout::kNCHW>
__device__ __forceinline__ size_t maps_offset(const DetMaps& m, const MapsAnchor& t, int b) {
  if constexpr (L == MapsLayout::kNHWC) return (static_cast<size_t>(b) * t.hw + t.p) * m.no;
  else return static_cast<size_t>(b) * m.no * t.hw + t.p;
}

// ---- readers: an anchor's channels as fp32 -------------------------------------------------------------------------------------------
// channel planes `hw` elements apart: the NCHW maps, and a decoded prediction (nms.cuh)
template <typename T>
struct MapsPlanes {
  const T* __restrict__ f; size_t hw;
  __device__ __forceinline__ float at(int c) const { return to_f32<T>(f[c * hw]); }
  __device__ __forceinline__ void side(int s, float (&v)[kMapsReg]) const {
#pragma unroll
    for (int j = 0; j < kMapsReg; ++j) v[j] = at(s * kMapsReg + j);
  }
};
// an NHWC anchor's row in global memory, for the kernels that gather single anchors: a side's bins are 16 / sizeof(T) channels per load where
// the row starts on a 16-byte boundary (a side starts 64 or 32 bytes into it), one channel per load where it does not
template <typename T>
struct MapsRow {
  static constexpr int kVec = 16 / static_cast<int>(sizeof(T));
  const T* __restrict__ f;
  __device__ __forceinline__ bool aligned() const { return (reinterpret_cast<uintptr_t>(f) & 15) == 0; }
  __device__ __forceinline__ float at(int c) const { return to_f32<T>(f[c]); }
  __device__ __forceinline__ void side(int s, float (&v)[kMapsReg]) const {
    if (aligned()) {
#pragma unroll
      for (int j = 0; j < kMapsReg; j += kVec) {
        float x[kVec];
        load_vec<T, kVec>(f + s * kMapsReg + j, x);
#pragma unroll
        for (int e = 0; e < kVec; ++e) v[j + e] = x[e];
      }
    } else {
#pragma unroll
      for (int j = 0; j < kMapsReg; ++j) v[j] = at(s * kMapsReg + j);
    }
  }
  // fn(c, channel c0 + c) for c = 0 .. n - 1 IN THAT ORDER: single channels up to the first 16-byte boundary, vectors, single channels
  template <typename F>
  __device__ __forceinline__ void scan(int c0, int n, F fn) const {
    const T* p = f + c0;
    const int head = min(n, static_cast<int>(((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(p)) & 15u)) & 15u) / sizeof(T)));
    int c = 0;
    for (; c < head; ++c) fn(c, to_f32<T>(p[c]));
    for (; c + kVec <= n; c += kVec) {
      float x[kVec];
      load_vec<T, kVec>(p + c, x);
#pragma unroll
      for (int e = 0; e < kVec; ++e) fn(c + e, x[e]);
    }
    for (; c < n; ++c) fn(c, to_f32<T>(p[c]));
  }
};
// an anchor's row staged in LDS as fp32 (maps_stage_in below)
struct MapsStaged {
  const float* f;
  __device__ __forceinline__ float at(int c) const { return f[c]; }
  __device__ __forceinline__ void side(int s, float (&v)[kMapsReg]) const {
#pragma unroll
    for (int j = 0; j < kMapsReg; ++j) v[j] = f[s * kMapsReg + j];
  }
};
template <typename T, MapsLayout L> struct MapsReaderOf { using type = MapsPlanes<T>; };
template <typename T> struct MapsReaderOf<T, MapsLayout::kNHWC> { using type = MapsRow<T>; };
// the reader of image b's anchor in global memory
template <typename T, MapsLayout L = MapsLayout::kNCHW>
__device__ __forceinline__ typename MapsReaderOf<T, L>::type maps_feat(const DetMaps& m, const MapsAnchor& t, int b) {
  const T* f = static_cast<const T*>(m.feat[t.l]) + maps_offset<L>(m, t, b);
  if constexpr (L == MapsLayout::kNHWC) return MapsRow<T>{f};
  else return MapsPlanes<T>{f, t.hw};
}

// one side's bins of an anchor: softmax probabilities, their expectation (loss.py:238, head.py: DFL) and the log of the sum of exponentials
template <typename R>
__device__ __forceinline__ void maps_side(const R& f, int side, float (&p)[kMapsReg], float& d, float& lse) {
  float m = -FLT_MAX;
  f.side(side, p);
#pragma unroll
  for (int j = 0; j < kMapsReg; ++j) m = fmaxf(m, p[j]);
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
template <typename R>
__device__ __forceinline__ float maps_dist(const R& f, int side) {
  float p[kMapsReg], d, lse;
  maps_side(f, side, p, d, lse);
  return d;
}
// the decoded box of the anchor at (ax, ay), in grid units (tal.py:382-391), a side after the other: the criterion's form
template <typename R>
__device__ __forceinline__ DetBox maps_decode(const R& f, float ax, float ay) {
  float p[kMapsReg], d[4], lse;
#pragma unroll
  for (int s = 0; s < 4; ++s) maps_side(f, s, p, d[s], lse);
  return DetBox{ax - d[0], ay - d[1], ax + d[2], ay + d[3]};
}

// ---- NHWC: a run of consecutive anchors of (B, A) through LDS -------------------------------------------------------------------------
// In NHWC the anchors [i0, i1) of the flattened (B, A) are, within one (image, level), ONE contiguous range of elements.  The per-anchor sweeps
// of the criterion copy such a run into LDS with 16-byte loads -- consecutive lanes on consecutive pieces, so a load instruction covers whole
// cache lines --, do their per-anchor arithmetic against LDS, and the backward leaves its gradients the same way with 16-byte stores (in the
// words its inputs came in, as values of T: maps_stage_put).  A run is
// cut into segments at level and image boundaries; a segment's first and last elements up to the next 16-byte boundary are moved one at a
// time, so nothing outside [first element, last element] of the level is touched.  In LDS a row is fp32 at a pitch of `no | 1` words: an odd
// pitch puts the 64 lanes of a wave, one row each, on 64 different banks at every channel (no = 144 would be a 16-way conflict).
__device__ __forceinline__ int maps_stage_pitch(int no) { return no | 1; }

// calls fn(level, the segment's first element in elements from the level's start, elements, first LDS row) for every segment of the anchors
// [i0, i1) of (B, A)
template <typename F>
__device__ __forceinline__ void maps_segments(const DetMaps& m, long long i0, long long i1, F fn) {
  long long i = i0;
  while (i < i1) {                                             // uniform over the workgroup
    const int b = static_cast<int>(i / m.A), a = static_cast<int>(i % m.A), l = maps_level(m, a), p = a - m.a0[l];
    const long long end = min(i1, static_cast<long long>(b) * m.A + m.a0[l + 1]);
    const size_t hw = static_cast<size_t>(m.H[l]) * m.W[l];
    fn(l, (static_cast<size_t>(b) * hw + p) * m.no, static_cast<unsigned>(end - i) * static_cast<unsigned>(m.no), static_cast<int>(i - i0));
    i = end;
  }
}
// a segment's split: `head` single elements up to the first 16-byte boundary, `nvec` vectors, the rest single
template <typename T>
__device__ __forceinline__ void maps_split(const T* g, unsigned n, unsigned& head, unsigned& nvec) {
  head = min(n, static_cast<unsigned>(((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(g)) & 15u)) & 15u) / sizeof(T)));
  nvec = (n - head) / (16u / sizeof(T));
}
// global -> LDS: element e of the segment goes to row row0 + e / no, column e % no
template <typename T>
__device__ __forceinline__ void maps_stage_in(const T* __restrict__ g, unsigned n, int row0, int no, float* s, int tid) {
  constexpr unsigned kVec = 16 / sizeof(T);
  const unsigned pitch = static_cast<unsigned>(maps_stage_pitch(no)), uno = static_cast<unsigned>(no);
  unsigned head, nvec;
  maps_split(g, n, head, nvec);
  for (unsigned v = tid; v < nvec; v += kBlock) {
    const unsigned e = head + v * kVec;
    float x[kVec];
    load_vec<T, static_cast<int>(kVec)>(g + e, x);
    unsigned r = e / uno, c = e - r * uno;
#pragma unroll
    for (unsigned k = 0; k < kVec; ++k) {
      s[(row0 + r) * pitch + c] = x[k];
      if (++c == uno) { c = 0; ++r; }
    }
  }
  const unsigned body = head + nvec * kVec, single = head + (n - body);          // the single elements: the head, then the tail
  for (unsigned i = tid; i < single; i += kBlock) {
    const unsigned e = i < head ? i : body + (i - head);
    const unsigned r = e / uno, c = e - r * uno;
    s[(row0 + r) * pitch + c] = to_f32<T>(g[e]);
  }
}
// a value of T in a stage word, as the backward leaves its gradients there: rounded to T by the expression that forms it and stored as T,
// exactly as the NCHW kernel stores it to memory, so the compiler selects the same instructions for the rounding in both layouts (with
// half features it fuses an expression's last multiply-add and the conversion into one mixed-precision instruction of a single rounding)
template <typename T>
__device__ __forceinline__ void maps_stage_put(float* w, float v) {
  const T t = from_f32<T>(v);
  __builtin_memcpy(w, &t, sizeof(T));
}
template <typename T>
__device__ __forceinline__ T maps_stage_get(const float* w) {
  T t;
  __builtin_memcpy(&t, w, sizeof(T));
  return t;
}
// LDS -> global: the values of T that maps_stage_put left
template <typename T>
__device__ __forceinline__ void maps_stage_out(T* __restrict__ g, unsigned n, int row0, int no, const float* s, int tid) {
  constexpr unsigned kVec = 16 / sizeof(T);
  const unsigned pitch = static_cast<unsigned>(maps_stage_pitch(no)), uno = static_cast<unsigned>(no);
  unsigned head, nvec;
  maps_split(g, n, head, nvec);
  for (unsigned v = tid; v < nvec; v += kBlock) {
    const unsigned e = head + v * kVec;
    Pack<T, static_cast<int>(kVec)> x;
    unsigned r = e / uno, c = e - r * uno;
#pragma unroll
    for (unsigned k = 0; k < kVec; ++k) {
      x.v[k] = maps_stage_get<T>(s + (row0 + r) * pitch + c);
      if (++c == uno) { c = 0; ++r; }
    }
    *reinterpret_cast<Pack<T, static_cast<int>(kVec)>*>(g + e) = x;
  }
  const unsigned body = head + nvec * kVec, single = head + (n - body);
  for (unsigned i = tid; i < single; i += kBlock) {
    const unsigned e = i < head ? i : body + (i - head);
    const unsigned r = e / uno, c = e - r * uno;
    g[e] = maps_stage_get<T>(s + (row0 + r) * pitch + c);
  }
}

}  // namespace mgacbam
