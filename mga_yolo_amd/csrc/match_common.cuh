// What the kernels of csrc/match.cuh and csrc/confusion.cuh share about (label, detection) pairs: the staging geometry, an image's live
// detection rows, the workgroup prefix and sum, and the reference's fp32 box_iou on one pair.  The labels themselves are csrc/labels.cuh's.
// Units that call match_iou are compiled with -ffp-contract=off (build.UNIT_FLAGS).
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kMatchMaxGt = 256;               // MGADET_MAX_GT
constexpr int kMatchWaves = kBlock / kWave;
constexpr int kMatchStage = 4;                 // label rows a thread looks at per staging chunk

// an image's live detection rows (Args: MatchArgs or CmArgs)
template <typename Args>
__device__ __forceinline__ int match_live_rows(const Args& A, int b) {
  const int c = A.count[b];
  return c < 0 ? 0 : (c > A.max_det ? A.max_det : c);
}

// Exclusive prefix of the threads' counts `c` over the workgroup, in thread order, and the workgroup's total: a shuffle scan per wave and
// the waves' totals through s_wave, kMatchWaves ints of LDS the caller does not touch between two calls.
__device__ __forceinline__ int match_block_offset(int c, int tid, int* s_wave, int& total) {
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  int incl = c;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += o;
  }
  __syncthreads();                                             // the previous call's readers are done with s_wave
  if (lane == kWave - 1) s_wave[wave] = incl;
  __syncthreads();
  int before = incl - c;
  total = 0;
#pragma unroll
  for (int w = 0; w < kMatchWaves; ++w) {
    const int t = s_wave[w];
    if (w < wave) before += t;
    total += t;
  }
  return before;
}

// U/utils/metrics.py:53-74 on one pair, every operation rounded once: the unit is compiled with -ffp-contract=off (build.UNIT_FLAGS), so
// no product here or in the label boxes is contracted into a fused multiply-add
__device__ __forceinline__ float match_iou(const float4 l, float area_l, const float4 d, float area_d) {
  const float iw = fmaxf(fminf(l.z, d.z) - fmaxf(l.x, d.x), 0.f), ih = fmaxf(fminf(l.w, d.w) - fmaxf(l.y, d.y), 0.f);
  const float inter = iw * ih;
  if (!(inter > 0.f)) return 0.f;                              // disjoint: 0 / den never beats a best IoU, so the division is skipped
  const float den = ((area_l + area_d) - inter) + 1e-7f;
  return inter / den;
}
__device__ __forceinline__ float match_area(const float4 q) {
  const float w = q.z - q.x, h = q.w - q.y;
  return w * h;
}

// whole-workgroup integer sum, the same value in every thread; s_sum: kMatchWaves words of LDS
__device__ __forceinline__ long long match_block_sum(long long v, int tid, long long* s_sum) {
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
  __syncthreads();
  if ((tid & (kWave - 1)) == 0) s_sum[tid / kWave] = v;
  __syncthreads();
  long long tot = 0;
#pragma unroll
  for (int w = 0; w < kMatchWaves; ++w) tot += s_sum[w];
  return tot;
}

}  // namespace mgacbam
