// Channels-last (NHWC) forms of the MaskCBAM kernels that stream x, gy, y or gx (MGACBAM_LAYOUT_NHWC levels): the shared
// helpers (the argument blocks are FwdArgs / BwdArgs, args.cuh); the kernels are in nhwc_fwd.cuh and nhwc_bwd.cuh.
//
// In NHWC the two reductions of the block swap roles: the per-pixel reductions over C (max_c / mean_c of u, sum_c ca*gy*x, the
// dL/dmask sum) run along contiguous memory, and the per-(b,c) reductions over H*W become sums across pixels.  Every kernel below uses
// ONE thread layout: a workgroup owns a TILE of CH consecutive pixels of one sample (per-channel kernels: a CHUNK of rp tiles, rp from
// H*W so that a sample has at most kNhwcMaxChunks partials); CS lanes (a power of two <= 64, so a pixel's
// lanes sit in one wave) split the channels of a pixel, VEC channels per lane per access (16 B for fp32, fp16 / bf16 when C % 8 == 0),
// and the PR = 256 / CS rows of lanes take pixels p0 + k*PR + row, k < kNhwcNpx.  A lane walks channel groups lane, lane + CS, ...
// so any C works; per-pixel sums are wave shuffles over the CS lanes, per-channel sums go through LDS over the PR rows in row order.
//
//   forward  k_pool_nhwc   x (1 read)  -> per-chunk partials (sum x*s, sum x, masked max + first pixel, sum s) -> ws
//            k_pool_fin    ws          -> S/use/den/avg/mx/mavg/valid/amax (fixed-order fold, ties to the lowest pixel); k_mlp -> ca
//            k_chan_nhwc   x (1 read)  -> planes [max_c u, mean_c u, sigma(mask)], cidx
//            k_apply_nhwc  x (1 read)  -> prologue: k x k conv of the tile's pixels -> sa ; body: y (1 write)
//   backward k_bwd_reduce1_nhwc x, gy  -> per-chunk partials of A and D, g_pre      (then the layout-free k_bwd_convT / k_bwd_wsa)
//            k_bwd_reduce2_nhwc x      -> per-chunk partials of sum_hw x*([c == cidx] gp0 + gp1/C)
//            k_bwd_fold_nhwc           -> g_z, D (chunk order), per-channel-block partials of W2^T g_z   (then k_bwd_params)
//            k_bwd_apply_nhwc gy (+ x when dL/dmask is wanted) -> gx, gmask
//
// Tiles and chunks follow the level alone (C, H*W, element type): never B or the other levels of the call, so a sample's results do
// not depend on the batch or the call composition.  No in-launch hand-off, no float atomics: every cross-workgroup sum is a partial
// plus one fixed-order reader.
#pragma once
#include "args.cuh"
#include "common.cuh"

namespace mgacbam {

// pixels per thread per tile: 8, or 4 with 8-element (16 B fp16 / bf16) lanes, so a thread's loads of one channel group stay at
// 32 elements in flight
template <int VEC> struct NhwcNpx { static constexpr int value = VEC == 8 ? 4 : 8; };

// per-channel partials of a chunk: each thread holds N sums for the VEC channels of its group; rows are combined in row order
// through LDS and threads t < CS*VEC write channel j*CS*VEC + t.  red: N * 256 * VEC floats.
template <int N, int VEC>
__device__ __forceinline__ void nhwc_rows_sum(float (&v)[N][VEC], float* red, int tid) {
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[(q * kBlock + tid) * VEC + e] = v[q][e];
  __syncthreads();
}

}  // namespace mgacbam
