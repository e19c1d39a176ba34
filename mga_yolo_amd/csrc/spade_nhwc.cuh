// MaskSPADE on channels-last features: x / y / gy / gx and the saved gamma are dense (B,H,W,C); the mask, dL/dmask, the parameters and
// every statistic are the same memory in both layouts.  The rule of this file: a channels-last level gives, bit for bit, what the same
// data gives as an NCHW level.
//   k_spade_fwd / dw / dh / ew: the kernels of spade.cuh with NHWC = true.  Only their global accesses differ (vector accesses along C).
//   statistics and the backward's plane sums: the NCHW kernels give lane l of the wave that owns a (b,c) plane a fixed sequence of pixels
//     and combine the 64 lanes with wave_group_sum.  Here a workgroup owns a sample and 16 channels; thread (cq = tid & 3, vl = tid >> 2)
//     runs the sequence of VIRTUAL lane vl for the four channels 4 cq .. 4 cq + 3 (one vector load per pixel), the partials go to LDS as
//     [channel][64], and a wave loads a channel's 64 partials lane by lane and calls the same wave_group_sum: same terms, same tree.
//   batch norm in training: the NCHW kernel is one workgroup per channel whose thread v chains over b and i = v, v + 256, ... and whose
//     block_sum is wave_group_sum per wave, then red[0] + red[1] + red[2] + red[3].  Here a workgroup owns 16 channels and ONE of the four
//     virtual waves (64 virtual threads): it leaves that wave's sum per channel, 4 C floats, in the ctx weight-pack area (written by
//     k_spade_pack only after the statistics); k_spade_bn_fin_nhwc adds the four in block_sum's order.  Two such pairs: mean, then squares.
// No atomics, no in-launch hand-offs, no global scratch.
#pragma once
#include "spade.cuh"

namespace mgacbam {

constexpr int kSpNhCB = 16;          // channels of a workgroup of the reductions below


// part [16][64] -> wave w combines the channels w, w + 4, w + 8, w + 12; every lane of the wave returns with the channel's sum in out[j]
__device__ __forceinline__ void sp_nh_combine(const float* part, int wave, int lane, float (&out)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = wave_group_sum(part[(wave + 4 * j) * 64 + lane], 64);
}

// statistics.  Instance norm: workgroup = (sample, 16 channels), both passes.  Batch norm in training: workgroup = (16 channels, virtual
// wave), the sums only (SQ = false; k_spade_bn_sq_nhwc is the second pass).  Batch norm in eval: as k_spade_stats.
template <typename T, bool SQ>
__device__ __forceinline__ void sp_bn_part(const SpadeArgs& A, int local, float* part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cq = (tid & 3) * 4, vl = tid >> 2;
  const int cb = local >> 2, vw = local & 3, v = vw * 64 + vl, HW = A.HW;
  const T* x = static_cast<const T*>(A.x) + cb * kSpNhCB + cq;
  float mean[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (SQ) ld4(A.mean + cb * kSpNhCB + cq, mean);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < A.B; ++b) {
    const T* p = x + static_cast<size_t>(b) * HW * A.C;
    for (int i = v; i < HW; i += kBlock) {
      float xv[4];
      load_vec<T, 4>(p + static_cast<size_t>(i) * A.C, xv);
#pragma unroll
      for (int k = 0; k < 4; ++k) { if constexpr (SQ) s[k] = sp_sq(s[k], xv[k], mean[k]); else s[k] += xv[k]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) part[(cq + k) * 64 + vl] = s[k];
  __syncthreads();
  float r[4];
  sp_nh_combine(part, wave, lane, r);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) A.wpack[(cb * kSpNhCB + wave + 4 * j) * 4 + vw] = r[j];
  }
}
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spade_stats_nhwc(const Group<SpadeArgs> G) {
  __shared__ float part[kSpNhCB * 64];
  __shared__ float means[kSpNhCB];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cq = (tid & 3) * 4, vl = tid >> 2;
  const int HW = A.HW;
  if (!A.bn) {
    const int ncb = A.C / kSpNhCB, b = local / ncb, cb = local - b * ncb;
    const T* p = static_cast<const T*>(A.x) + static_cast<size_t>(b) * HW * A.C + cb * kSpNhCB + cq;
    const bool quads = (HW & 3) == 0;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (quads) {
      for (int i = vl * 4; i < HW; i += 256) {
        float v[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) load_vec<T, 4>(p + static_cast<size_t>(i + e) * A.C, v[e]);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float q4[4] = {v[0][k], v[1][k], v[2][k], v[3][k]}; s[k] = sp_sum4(s[k], q4); }
      }
    } else {
      for (int i = vl; i < HW; i += 64) {
        float v[4];
        load_vec<T, 4>(p + static_cast<size_t>(i) * A.C, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += v[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[(cq + k) * 64 + vl] = s[k];
    __syncthreads();
    float r[4];
    sp_nh_combine(part, wave, lane, r);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) means[wave + 4 * j] = sp_mean_of(r[j], HW);
    }
    __syncthreads();
    float mean[4], q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) mean[k] = means[cq + k];
    if (quads) {
      for (int i = vl * 4; i < HW; i += 256) {
        float v[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e) load_vec<T, 4>(p + static_cast<size_t>(i + e) * A.C, v[e]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int e = 0; e < 4; ++e) q[k] = sp_sq(q[k], v[e][k], mean[k]);
        }
      }
    } else {
      for (int i = vl; i < HW; i += 64) {
        float v[4];
        load_vec<T, 4>(p + static_cast<size_t>(i) * A.C, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = sp_sq(q[k], v[k], mean[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) part[(cq + k) * 64 + vl] = q[k];
    __syncthreads();
    sp_nh_combine(part, wave, lane, r);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ch = wave + 4 * j, plane = b * A.C + cb * kSpNhCB + ch;
        A.mean[plane] = means[ch];
        A.rstd[plane] = sp_rstd_of(sp_mean_of(r[j], HW), A.eps);
      }
    }
  } else if (A.train) {
    sp_bn_part<T, false>(A, local, part);
  } else {
    const int i = local * kBlock + tid;
    if (i >= A.B * A.C) return;
    const int c = i % A.C;
    A.mean[i] = A.rmean[c];
    A.rstd[i] = sp_rstd_of(A.rvar[c], A.eps);
  }
}
// batch norm in training only (the other levels of the group get no workgroup)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spade_bn_sq_nhwc(const Group<SpadeArgs> G) {
  __shared__ float part[kSpNhCB * 64];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  sp_bn_part<T, true>(A, local, part);
}
// SQ = false: mean of the channel into A.mean (every sample's copy).  SQ = true: rstd, the running statistics, num_batches_tracked.
template <bool SQ>
__global__ __launch_bounds__(kBlock) void k_spade_bn_fin_nhwc(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int c = local * kBlock + threadIdx.x;
  if (c >= A.C) return;
  float s = A.wpack[4 * c];
  for (int w = 1; w < kBlock / kWave; ++w) s += A.wpack[4 * c + w];
  const float n = static_cast<float>(A.B) * A.HW;
  if constexpr (SQ) {
    sp_bn_finish(A, c, A.mean[c], s, n);
  } else {
    const float mean = s / n;
    for (int b = 0; b < A.B; ++b) A.mean[b * A.C + c] = mean;
  }
}

// backward (i): the four per-plane sums; workgroup = (sample, 16 channels)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spade_bwd_reduce_nhwc(const Group<SpadeArgs> G) {
  __shared__ float part[4][kSpNhCB * 64];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cq = (tid & 3) * 4, vl = tid >> 2;
  const int ncb = A.C / kSpNhCB, b = local / ncb, cb = local - b * ncb;
  const int plane0 = b * A.C + cb * kSpNhCB;
  const size_t base = static_cast<size_t>(b) * A.HW * A.C + cb * kSpNhCB + cq;
  const T* x = static_cast<const T*>(A.x) + base;
  const T* gy = static_cast<const T*>(A.gy) + base;
  const T* gam = static_cast<const T*>(A.gamma) + base;
  float mean[4], rstd[4];
  ld4(A.mean + plane0 + cq, mean);
  ld4(A.rstd + plane0 + cq, rstd);
  float s[4][4] = {};
  for (int i = vl; i < A.HW; i += 64) {
    const size_t at = static_cast<size_t>(i) * A.C;
    float xv[4], gyv[4], gv[4];
    load_vec<T, 4>(gy + at, gyv);
    load_vec<T, 4>(x + at, xv);
    if (A.has_mask) {
      load_vec<T, 4>(gam + at, gv);
#pragma unroll
      for (int k = 0; k < 4; ++k) gv[k] = gyv[k] * gv[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) gv[k] = gyv[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) sp_red_terms(s[k], gyv[k], sp_xhat(xv[k], mean[k], rstd[k]), gv[k]);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int t = 0; t < 4; ++t) part[t][(cq + k) * 64 + vl] = s[k][t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float r[4];
    sp_nh_combine(part[t], wave, lane, r);
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) A.red[4 * static_cast<size_t>(plane0 + wave + 4 * j) + t] = r[j];
    }
  }
}

}  // namespace mgacbam
