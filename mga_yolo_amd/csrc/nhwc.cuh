// Channels-last (NHWC) levels (MGACBAM_LAYOUT_NHWC): the ONE thread layout of the MaskCBAM kernels of nhwc_fwd.cuh / nhwc_bwd.cuh and
// the MaskECA kernels of eca_nhwc.cuh, as code.  (The argument blocks are FwdArgs / BwdArgs, args.cuh, and EcaFwdArgs / EcaBwdArgs.)
//
// In NHWC the two reductions of a block swap roles: the per-pixel reductions over C (max_c / mean_c of u, sum_c ca*gy*x, the dL/dmask
// sum) run along contiguous memory, and the per-(b,c) reductions over H*W become sums across pixels.
//
//   NhwcPos / nhwc_pos       a thread's place: CS lanes (a power of two <= 64, so a pixel's lanes sit in one wave) split the channels of
//                            a pixel, VEC channels per lane per access (16 B for fp32, fp16 / bf16 when C % 8 == 0); the PR = 256 / CS
//                            rows of lanes take different pixels
//   NhwcPix / nhwc_pixels    a thread's pixels of a TILE of CH = PR * NPX consecutive pixels of one sample: p0 + k*PR + row, k < NPX
//                            (k_chan_nhwc keeps its own test of the pixels: see there)
//   NhwcGroup                a lane's channel group of pass j: groups lane, lane + CS, ... so any C works -- nhwc_group_live for the
//                            streaming kernels (leave the loop past the last group), nhwc_group_clamped for the reducing ones
//   nhwc_rows_to_channels    per-channel sums of a pass: the PR rows meet in LDS and are added in row order by the channel's owner thread
//   nhwc_chunk_row_total     a per-row value (sum of s) over the rows, in row order
//   nhwc_chunk_fold          the fold kernels: a sample's chunk partials with a stride of 4 per wave, then waves 0..3 in order
//   per-pixel sums           wave_group_sum / wave_group_argmax over the CS lanes (common.cuh)
//
// Per-pixel kernels take one tile per workgroup; per-channel kernels a CHUNK of rp tiles, rp from H*W so that a sample has at most
// kNhwcMaxChunks partials (host.cuh: nhwc_geo).  Tiles and chunks follow the level alone (C, H*W, element type): never B or the other
// levels of the call, so a sample's results do not depend on the batch or the call composition.  No in-launch hand-off, no float atomics:
// every cross-workgroup sum is a partial plus one fixed-order reader.
//
//   forward  k_pool_nhwc   x (1 read)  -> per-chunk partials (sum x*s, sum x, masked max + first pixel, sum s) -> ws
//            k_pool_fin    ws          -> S/use/den/avg/mx/mavg/valid/amax (fixed-order fold, ties to the lowest pixel); k_mlp -> ca
//            k_chan_nhwc   x (1 read)  -> planes [max_c u, mean_c u, sigma(mask)], cidx
//            k_apply_nhwc  x (1 read)  -> prologue: k x k conv of the tile's pixels -> sa ; body: y (1 write)
//   backward k_bwd_reduce1_nhwc x, gy  -> per-chunk partials of A and D, g_pre      (then the layout-free k_bwd_convT / k_bwd_wsa)
//            k_bwd_reduce2_nhwc x      -> per-chunk partials of sum_hw x*([c == cidx] gp0 + gp1/C)
//            k_bwd_fold_nhwc           -> g_z, D (chunk order), per-channel-block partials of W2^T g_z   (then k_bwd_params)
//            k_bwd_apply_nhwc gy (+ x when dL/dmask is wanted) -> gx, gmask
//   (MaskECA: the table in eca_nhwc.cuh)
//
// A kernel's dynamic LDS is a small __host__ __device__ struct beside it (fields = offsets in floats, `total`): the kernel carves its
// pointers from it and the host asks lds_bytes() of the same struct.
#pragma once
#include "args.cuh"
#include "common.cuh"

namespace mgacbam {

// pixels per thread per tile: 8, or 4 with 8-element (16 B fp16 / bf16) lanes, so a thread's loads of one channel group stay at
// 32 elements in flight
template <int VEC> struct NhwcNpx { static constexpr int value = VEC == 8 ? 4 : 8; };

// bytes of a dynamic-LDS layout struct (what the launch asks for)
template <typename Lds>
__host__ __device__ inline size_t lds_bytes(const Lds& l) { return l.total * sizeof(float); }

// a thread's place in the workgroup
struct NhwcPos {
  int tid, CS, lane, row, PR;   // lane = tid % CS: the channel lane; row = tid / CS of the PR = 256 / CS pixel rows
  int nj, CV;                   // passes over the channel groups = ceil(ng / CS); channels per pass = CS * VEC
};
template <int VEC>
__device__ __forceinline__ NhwcPos nhwc_pos(const NhwcGeo& n) {
  NhwcPos t;
  t.tid = threadIdx.x; t.CS = n.cs; t.lane = t.tid & (t.CS - 1); t.row = t.tid >> n.lcs; t.PR = kBlock >> n.lcs;
  t.nj = (n.ng + t.CS - 1) / t.CS; t.CV = t.CS * VEC;
  return t;
}

// a thread's pixels of the tile that starts at p0: ok = inside the sample; pix = the pixel, 0 where it is not (a safe address to load).
// pix[k] is THE pixel index: every load takes it, whether the pixel is live or not.  live(k) is the same pixel for what happens only
// under ok[k] after the channel loop, a store to the pixel (k_apply_nhwc's y, k_eca_pool_nhwc's splane) or its index as a value
// (k_pool_nhwc's arg-max): formed again from p0 and the row, so that pix[] need not stay in registers across the loop for it.
template <int NPX> struct NhwcPix {
  int pix[NPX];
  bool ok[NPX];
  int p0, PR, row;
  __device__ __forceinline__ int live(int k) const { return p0 + k * PR + row; }
};
template <int NPX>
__device__ __forceinline__ NhwcPix<NPX> nhwc_pixels(const NhwcPos& t, int p0, int HW) {
  NhwcPix<NPX> P;
  P.p0 = p0; P.PR = t.PR; P.row = t.row;
#pragma unroll
  for (int k = 0; k < NPX; ++k) {
    const int p = P.live(k);
    P.ok[k] = p < HW;
    P.pix[k] = P.ok[k] ? p : 0;
  }
  return P;
}

// a lane's channel group of pass j: channels c0 .. c0 + VEC - 1
struct NhwcGroup { int cgi, c0; bool okc; };
// streaming kernels (no barrier inside the pass loop): `if (!nhwc_group_live<VEC>(t, n, j, cg)) break;`
template <int VEC>
__device__ __forceinline__ bool nhwc_group_live(const NhwcPos& t, const NhwcGeo& n, int j, NhwcGroup& cg) {
  cg.cgi = t.lane + j * t.CS; cg.okc = cg.cgi < n.ng; cg.c0 = cg.cgi * VEC;
  return cg.okc;
}
// reducing kernels: every thread must reach the barriers of the pass, so a lane past the last group loads the last group's channels
// (a safe address) and carries okc = false
template <int VEC>
__device__ __forceinline__ NhwcGroup nhwc_group_clamped(const NhwcPos& t, const NhwcGeo& n, int j) {
  NhwcGroup cg;
  cg.cgi = t.lane + j * t.CS; cg.okc = cg.cgi < n.ng; cg.c0 = min(cg.cgi, n.ng - 1) * VEC;
  return cg;
}

// every thread's N x VEC sums of a pass -> red (N * 256 * VEC floats), between two barriers
template <int N, int VEC>
__device__ __forceinline__ void nhwc_rows_sum(float (&v)[N][VEC], float* red, int tid) {
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q)
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[(q * kBlock + tid) * VEC + e] = v[q][e];
  __syncthreads();
}
// per-channel sums of pass j over the rows of the workgroup: nhwc_rows_sum, then thread u < CV owns channel c = j*CV + u and adds its
// PR rows in row order (element (row r, lane u / VEC, e = u % VEC) of sum q is red[q*256*VEC + r*CV + u]); sink(c, sums) takes the
// N sums.  (CV = 512 with 8-element lanes.)  k_pool_nhwc, whose third column is an arg-max, calls nhwc_rows_sum and walks the rows itself.
template <int N, int VEC, typename Sink>
__device__ __forceinline__ void nhwc_rows_to_channels(float (&acc)[N][VEC], float* red, const NhwcPos& t, int j, int C, Sink sink) {
  nhwc_rows_sum<N, VEC>(acc, red, t.tid);
  for (int u = t.tid; u < t.CV; u += kBlock) {
    const int c = j * t.CV + u;
    if (c < C) {
      float s[N];
#pragma unroll
      for (int q = 0; q < N; ++q) s[q] = 0.f;
      for (int r = 0; r < t.PR; ++r) {
#pragma unroll
        for (int q = 0; q < N; ++q) s[q] += red[q * kBlock * VEC + r * t.CV + u];
      }
      sink(c, s);
    }
  }
}

// a value every lane of a row holds (the row's sum of s over the chunk), added over the PR rows in row order: valid in thread 0.
// red: PR floats, free to write (the caller's barrier)
__device__ __forceinline__ float nhwc_chunk_row_total(float v, float* red, const NhwcPos& t) {
  if (t.lane == 0) red[t.row] = v;
  __syncthreads();
  float s = 0.f;
  if (t.tid == 0) for (int r = 0; r < t.PR; ++r) s += red[r];
  return s;
}

// The fold kernels (workgroup = (sample, kNhwcFoldC channels), thread = (channel tid % 64, wave tid / 64)): N sums over a sample's
// nchunk partials.  Wave w adds chunks w, w + 4, ... (term(q, s) adds chunk q's terms to s), the four results meet in s_part[n][tid] and
// wave 0 adds waves 1..3 in order: s is valid in wave 0.  side(tid) runs before the barrier, for a column that is not a sum
// (k_pool_fin's arg-max).
struct NhwcNoSide { __device__ __forceinline__ void operator()(int) const {} };
template <int N, typename Term, typename Side = NhwcNoSide>
__device__ __forceinline__ void nhwc_chunk_fold(float (&s)[N], float (*s_part)[kBlock], int nchunk, Term term, Side side = Side()) {
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = 0.f;
#pragma unroll 4
  for (int q = grp; q < nchunk; q += 4) term(q, s);
#pragma unroll
  for (int n = 0; n < N; ++n) s_part[n][tid] = s[n];
  side(tid);
  __syncthreads();
  if (grp != 0) return;
  for (int r = 1; r < 4; ++r) {
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] += s_part[n][r * 64 + lane];
  }
}

}  // namespace mgacbam
