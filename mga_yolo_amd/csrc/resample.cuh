// Bilinear resample of MaskSPADE's mask (include/mgaresample.h): a mask given at another resolution is brought to the feature's size before
// the block reads it (masked_spade.py:102-110: F.interpolate(mode="bilinear", align_corners=False)), and the block's dL/dmask goes back
// through the exact adjoint.  Both are a few hundred KB at most: one launch per direction covers every level of the call.
//   k_resample_fwd: one thread per destination pixel (four of a row where out_w % 4 == 0: one 16-byte store), four taps.
//   k_resample_bwd: one thread per SOURCE pixel i, gather form.  The operator is separable, so per axis the thread walks the contiguous
//                   range of destination indices j whose footprint may hold i -- the inverse map, two indices wider -- in ascending order, and
//                   the forward's own index function (bilinear_tap, common.cuh) decides membership and weight: i0(j) == i gives 1 - lam,
//                   i1(j) == i gives lam (both at the clamped last index).  No atomics, a fixed order: two runs give the same bits.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kResampleLevelsMax = 8;          // = MGACBAM_MAX_LEVELS (api_spade.hip asserts it)
struct ResampleLevel {
  const float* src;
  float* dst;
  int B, in_h, in_w, out_h, out_w;
  int vec;                                     // forward: destination pixels per thread, 4 (out_w % 4 == 0, dst 16-byte aligned) or 1
};
struct ResampleGroup {
  int n;
  int start[kResampleLevelsMax + 1];           // workgroup ids [start[l], start[l+1]) belong to level l
  ResampleLevel lv[kResampleLevelsMax];
};
__device__ __forceinline__ int resample_find_level(const ResampleGroup& g, int bid, int& local) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < kResampleLevelsMax; ++i)
    if (i < g.n && bid >= g.start[i]) l = i;
  local = bid - g.start[l];
  return l;
}

template <int VEC>
__device__ __forceinline__ void resample_fwd_px(const ResampleLevel& L, int t) {
  const int wq = L.out_w / VEC;
  if (t >= L.B * L.out_h * wq) return;
  const int xq = t % wq, r = t / wq;
  const int y = r % L.out_h, b = r / L.out_h;
  const float sh = static_cast<float>(L.in_h) / static_cast<float>(L.out_h), sw = static_cast<float>(L.in_w) / static_cast<float>(L.out_w);
  int y0, y1;
  float ly;
  bilinear_tap(sh, y, L.in_h, y0, y1, ly);
  const float* sb = L.src + static_cast<size_t>(b) * L.in_h * L.in_w;
  const float* r0 = sb + static_cast<size_t>(y0) * L.in_w;
  const float* r1 = sb + static_cast<size_t>(y1) * L.in_w;
  float out[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    int x0, x1;
    float lx;
    bilinear_tap(sw, xq * VEC + e, L.in_w, x0, x1, lx);
    // the FMAs are spelled out: left to contraction, the compiler fused the OTHER product in pixels 2 and 3 of the four-pixel path, so a
    // pixel's bits depended on the path its row took (tests/test_gpu_resample.py::test_misaligned_buffers_give_the_same_bits)
    const float top = fmaf(lx, r0[x1], (1.f - lx) * r0[x0]);
    const float bot = fmaf(lx, r1[x1], (1.f - lx) * r1[x0]);
    out[e] = fmaf(1.f - ly, top, ly * bot);
  }
  store_vec<float, VEC>(L.dst + (static_cast<size_t>(b) * L.out_h + y) * L.out_w + xq * VEC, out);
}

__global__ __launch_bounds__(kBlock) void k_resample_fwd(const ResampleGroup G) {
  int local;
  const int l = resample_find_level(G, blockIdx.x, local);
  const ResampleLevel& L = G.lv[l];
  const int t = local * kBlock + static_cast<int>(threadIdx.x);
  if (L.vec == 4) resample_fwd_px<4>(L, t);
  else resample_fwd_px<1>(L, t);
}

// the destination indices j of one axis whose footprint can hold source index i: f(j) in (i - 1, i + 1) inverts to the open interval
// ((i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5).  floor / ceil of its ends already lie one index outside it and the range takes one
// more each way: two indices of margin against the fp32 rounding of the ends (a range narrower by two at either end still passes every
// test, one narrower by three fails nearly all of them: DESIGN 7f-1)
__device__ __forceinline__ void resample_range(float inv_scale, int i, int n_out, int& lo, int& hi) {
  lo = max(static_cast<int>(floorf((static_cast<float>(i) - 0.5f) * inv_scale - 0.5f)) - 1, 0);
  hi = min(static_cast<int>(ceilf((static_cast<float>(i) + 1.5f) * inv_scale - 0.5f)) + 1, n_out - 1);
}
// weight of destination index j on source index i along one axis (0 when i is not in j's footprint)
__device__ __forceinline__ float resample_weight(float scale, int j, int n_in, int i) {
  int i0, i1;
  float lam;
  bilinear_tap(scale, j, n_in, i0, i1, lam);
  return (i0 == i ? 1.f - lam : 0.f) + (i1 == i ? lam : 0.f);
}

// L.src: dL/d(forward dst) (B,1,out_h,out_w); L.dst: dL/d(forward src) (B,1,in_h,in_w)
__global__ __launch_bounds__(kBlock) void k_resample_bwd(const ResampleGroup G) {
  int local;
  const int l = resample_find_level(G, blockIdx.x, local);
  const ResampleLevel& L = G.lv[l];
  const int t = local * kBlock + static_cast<int>(threadIdx.x);
  if (t >= L.B * L.in_h * L.in_w) return;
  const int xi = t % L.in_w, r = t / L.in_w;
  const int yi = r % L.in_h, b = r / L.in_h;
  const float sh = static_cast<float>(L.in_h) / static_cast<float>(L.out_h), sw = static_cast<float>(L.in_w) / static_cast<float>(L.out_w);
  const float ih = static_cast<float>(L.out_h) / static_cast<float>(L.in_h), iw = static_cast<float>(L.out_w) / static_cast<float>(L.in_w);
  int ylo, yhi, xlo, xhi;
  resample_range(ih, yi, L.out_h, ylo, yhi);
  resample_range(iw, xi, L.out_w, xlo, xhi);
  const float* gb = L.src + static_cast<size_t>(b) * L.out_h * L.out_w;
  float acc = 0.f;
  for (int yj = ylo; yj <= yhi; ++yj) {
    const float wy = resample_weight(sh, yj, L.in_h, yi);
    if (wy == 0.f) continue;
    const float* grow = gb + static_cast<size_t>(yj) * L.out_w;
    float row = 0.f;
    for (int xj = xlo; xj <= xhi; ++xj) {
      const float wx = resample_weight(sw, xj, L.in_w, xi);
      if (wx != 0.f) row += wx * grow[xj];
    }
    acc += wy * row;
  }
  L.dst[t] = acc;
}

}  // namespace mgacbam
