// Channels-last (MGACBAM_LAYOUT_NHWC) forms of the MaskECA kernels: the thread layout of nhwc.cuh (NhwcPos, NhwcPix, NhwcGroup, the
// folds), the algebra of eca.cuh (eca_pooled_stats, eca_gate_w, eca_bwd_prologue, eca_gmask, eca_params_body).
//
//   forward   k_eca_pool_nhwc    x (1 read)        -> per-chunk partials of sum x*s and sum x per channel, sum s ; sigma(mask) plane
//             k_eca_fin          partials          -> S/use/den, mavg, avg (fixed-order fold, as k_pool_fin)
//             k_eca_apply_nhwc   x (1 read)        -> prologue: gate[c] = 1 + a*(sigmoid(conv1d(avg))[c] - 0.5) -> LDS ; y = x*gate (1 write)
//   backward  k_eca_reduce_nhwc  x, gy (1 read)    -> per-chunk partials of gg[b,c] = sum_hw gy*x
//             k_eca_fold         partials          -> gg (fixed-order fold)
//             k_eca_bwd_nhwc     gy (+x for gmask) -> prologue of k_eca_bwd ; gx = gy*g + g_avg*wA ; gmask ; the 16 role workgroups
//
// 3 E forward, 5 E backward (4 E without dL/dmask), 6 launches per step for all NHWC levels of a call.  A chunk workgroup sweeps its
// rp tiles once per pass of CS*VEC channels and keeps the running sums in registers: the rows meet in LDS once per pass, not once per
// tile.  Tiles and chunks follow the level alone (host.cuh nhwc_geo); no float atomics, no in-launch hand-off: every cross-workgroup
// sum is a partial plus one fixed-order reader.
#pragma once
#include "eca.cuh"
#include "nhwc.cuh"

namespace mgacbam {

__host__ __device__ inline size_t eca_nhwc_part_stride(int C) { return 2 * static_cast<size_t>(C) + 4; }

// ---------------------------------------------------------------------------------------------
// k_eca_pool_nhwc: workgroup = (sample, chunk of rp tiles).  The workgroup owns its pixels' sigma(mask) and their sum.
//   static LDS: red = NS x 256*VEC row sums of a pass
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC, bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_eca_pool_nhwc(const Group<EcaFwdArgs> G) {
  constexpr int NS = HAS_MASK ? 2 : 1;                                    // [sum x][sum x*s]
  __shared__ __align__(16) float red[NS * kBlock * VEC];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaFwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  const float* mb = HAS_MASK ? A.mask + static_cast<size_t>(b) * g.HW : nullptr;
  float* splane = A.c.splane + static_cast<size_t>(b) * g.HW;
  float* part = A.part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * eca_nhwc_part_stride(g.C);
  const int t0 = chunk * A.n.rp, t_end = min(t0 + A.n.rp, A.n.ntile);
  float ssum = 0.f;
  for (int j = 0; j < t.nj; ++j) {
    const NhwcGroup cg = nhwc_group_clamped<VEC>(t, A.n, j);
    float acc[NS][VEC];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
    for (int tile = t0; tile < t_end; ++tile) {
      const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
      float s[NPX];
      float xv[NPX][VEC];
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        load_vec<T, VEC>(xb + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, xv[k]);
        s[k] = 0.f;
        if (HAS_MASK && P.ok[k]) {
          const float m = mb[P.pix[k]];
          s[k] = g.use_sigmoid ? sigmoid_fast(m) : m;                     // masked_eca.py:146-147
        }
        if (j == 0 && P.ok[k]) {
          ssum += s[k];
          if (t.lane == 0) splane[P.live(k)] = s[k];                       // (zeros when there is no mask)
        }
      }
#pragma unroll
      for (int k = 0; k < NPX; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float v = (P.ok[k] && cg.okc) ? xv[k][e] : 0.f;
          acc[0][e] += v;
          if (HAS_MASK) acc[NS - 1][e] += v * s[k];
        }
    }
    // without a mask only sum x is formed (k_eca_fin reads nothing else)
    nhwc_rows_to_channels<NS, VEC>(acc, red, t, j, g.C, [&](int c, const float (&sum)[NS]) {
#pragma unroll
      for (int q = 0; q < NS; ++q) part[static_cast<size_t>(q) * g.C + c] = sum[q];
    });
  }
  // sum of s over the chunk (every lane of a row holds the row's sum)
  __syncthreads();
  const float S = nhwc_chunk_row_total(ssum, red, t);
  if (t.tid == 0) part[2 * g.C] = S;
}

// ---------------------------------------------------------------------------------------------
// k_eca_fin: workgroup = (sample, block of kNhwcFoldC channels): nhwc_chunk_fold over the chunk partials, then the statistics
// exactly as k_eca_pool defines them (eca_pooled_stats).
// ---------------------------------------------------------------------------------------------
template <bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_eca_fin(const Group<EcaFwdArgs> G) {
  __shared__ float s_part[2][kBlock];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaFwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  const int ncb = (g.C + kNhwcFoldC - 1) / kNhwcFoldC;
  const int b = local / ncb, cb = local - b * ncb;
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6, nch = A.n.nchunk;
  const size_t stride = eca_nhwc_part_stride(g.C);
  const float* wb = A.part + static_cast<size_t>(b) * nch * stride;
  float S = 0.f;                                                          // every workgroup of the sample forms S the same way
  if (HAS_MASK) {
    for (int q = lane; q < nch; q += 64) S += wb[q * stride + 2 * g.C];
    S = wave_group_sum(S, 64);
  }
  const int c = cb * kNhwcFoldC + lane;
  const int cc = min(c, g.C - 1);
  float sum[2];                                                           // [sum x*s][sum x]
  nhwc_chunk_fold<2>(sum, s_part, nch, [&](int q, float (&s)[2]) {
    const float* pq = wb + q * stride;
    s[1] += pq[cc];
    if (HAS_MASK) s[0] += pq[g.C + cc];
  });
  if (grp != 0 || c >= g.C) return;
  eca_pooled_stats<HAS_MASK>(A.c, g, b, c, S, sum[1], sum[0]);
}

// ---------------------------------------------------------------------------------------------
// k_eca_apply_nhwc: workgroup = (sample, tile).  Prologue: the sample's C gates into LDS (tile 0 also saves w); body: y = x * gate[c]
// ---------------------------------------------------------------------------------------------
struct EcaApplyNhwcLds {
  size_t gate;                 // [C] 1 + a*(w - 0.5)
  size_t total;
  __host__ __device__ explicit EcaApplyNhwcLds(const Geo& g) : gate(0), total(g.C) {}
};
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_eca_apply_nhwc(const Group<EcaFwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaFwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  T* yb = static_cast<T*>(A.y) + sb;
  const float a = softplusf_(*A.beta);
  float* s_gate = smem + EcaApplyNhwcLds(g).gate;
  const float* desc = eca_descriptor(A.c, g, A.mask != nullptr);
  for (int c = t.tid; c < g.C; c += kBlock) {
    const float w = eca_gate_w(desc + static_cast<size_t>(b) * g.C, A.w1d, g.k, g.C, c);
    s_gate[c] = 1.f + a * (w - 0.5f);                                     // masked_eca.py:190
    if (tile == 0) A.c.w[static_cast<size_t>(b) * g.C + c] = w;
  }
  __syncthreads();
  const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
  for (int j = 0; j < t.nj; ++j) {
    NhwcGroup cg;
    if (!nhwc_group_live<VEC>(t, A.n, j, cg)) break;
    float gv[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) gv[e] = s_gate[min(cg.c0 + e, g.C - 1)];
    float xv[NPX][VEC];
#pragma unroll
    for (int k = 0; k < NPX; ++k) load_vec<T, VEC>(xb + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, xv[k]);
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      float yv[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) yv[e] = xv[k][e] * gv[e];
      if (P.ok[k]) store_vec<T, VEC>(yb + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, yv);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_reduce_nhwc: per-chunk partials of gg[b,c] = sum_hw gy*x   (chunks as k_eca_pool_nhwc)
//   static LDS: red = 256*VEC row sums of a pass
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_eca_reduce_nhwc(const Group<EcaBwdArgs> G) {
  __shared__ __align__(16) float red[kBlock * VEC];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaBwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  float* part = A.part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * g.C;
  const int t0 = chunk * A.n.rp, t_end = min(t0 + A.n.rp, A.n.ntile);
  for (int j = 0; j < t.nj; ++j) {
    const NhwcGroup cg = nhwc_group_clamped<VEC>(t, A.n, j);
    float acc[1][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
    for (int tile = t0; tile < t_end; ++tile) {
      const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
      float xv[NPX][VEC], gv[NPX][VEC];
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        const size_t o = static_cast<size_t>(P.pix[k]) * g.C + cg.c0;
        load_vec<T, VEC>(xb + o, xv[k]);
        load_vec<T, VEC>(gb + o, gv[k]);
      }
#pragma unroll
      for (int k = 0; k < NPX; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[0][e] += (P.ok[k] && cg.okc) ? xv[k][e] * gv[k][e] : 0.f;
    }
    nhwc_rows_to_channels<1, VEC>(acc, red, t, j, g.C, [&](int c, const float (&sum)[1]) { part[c] = sum[0]; });
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_fold: workgroup = (sample, block of kNhwcFoldC channels): gg[b,c] = nhwc_chunk_fold over its chunk partials
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_eca_fold(const Group<EcaBwdArgs> G) {
  __shared__ float s_part[kBlock];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaBwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  const int ncb = (g.C + kNhwcFoldC - 1) / kNhwcFoldC;
  const int b = local / ncb, cb = local - b * ncb;
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  const int c = cb * kNhwcFoldC + lane, cc = min(c, g.C - 1);
  const float* pb = A.part + static_cast<size_t>(b) * A.n.nchunk * g.C + cc;
  float sum[1];
  nhwc_chunk_fold<1>(sum, &s_part, A.n.nchunk, [&](int q, float (&s)[1]) { s[0] += pb[static_cast<size_t>(q) * g.C]; });
  if (grp != 0 || c >= g.C) return;
  A.s.gg[static_cast<size_t>(b) * g.C + c] = sum[0];
}

// ---------------------------------------------------------------------------------------------
// k_eca_bwd_nhwc: gx = gy*g + g_avg*wA ; gmask = (use/den) * (sum_c g_avg*x - K_b) * s(1-s)      (eca.cuh k_eca_bwd, NHWC)
//   prologue per workgroup (its sample): eca_bwd_prologue
//   the level's first 16 workgroups are the parameter-gradient roles (eca_params_body: layout-free)
// ---------------------------------------------------------------------------------------------
struct EcaBwdNhwcLds {
  size_t gy1;                  // [C] a*gg*w(1-w), padded to 2 floats: q is float2, keep it 8-byte aligned
  size_t q;                    // [C] float2 {g, g_avg}
  size_t total;
  __host__ __device__ explicit EcaBwdNhwcLds(const Geo& g)
      : gy1(0), q(gy1 + ((static_cast<size_t>(g.C) + 1) & ~static_cast<size_t>(1))), total(q + 2 * static_cast<size_t>(g.C)) {}
};
template <typename T, int VEC, bool GMASK>
__global__ __launch_bounds__(kBlock) void k_eca_bwd_nhwc(const Group<EcaBwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[kEcaBwdRed];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaBwdArgs& A = G.lv[l];
  if (local < kEcaRoles) { eca_params_body(A, local, red); return; }     // 16 role ids keep the streaming ids XCD-aligned
  local -= kEcaRoles;
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const float a = softplusf_(*A.beta);
  const float Nf = static_cast<float>(g.HW);
  const bool has_mask = A.mask != nullptr;
  const EcaBwdNhwcLds L(g);
  float2* s_q = reinterpret_cast<float2*>(smem + L.q);
  const float kb = eca_bwd_prologue(A, b, a, smem + L.gy1, s_q, red);

  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  T* ob = static_cast<T*>(A.gx) + sb;
  const float use = A.c.use[b], den = A.c.den[b];
  const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
  float sv[NPX], wA[NPX], accp[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) {
    sv[k] = A.c.splane[static_cast<size_t>(b) * g.HW + P.pix[k]];
    wA[k] = has_mask ? (use * sv[k] / den + (1.f - use) / Nf) : 1.f / Nf;
    accp[k] = 0.f;
  }
  for (int j = 0; j < t.nj; ++j) {
    NhwcGroup cg;
    if (!nhwc_group_live<VEC>(t, A.n, j, cg)) break;
    float2 q[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[e] = s_q[min(cg.c0 + e, g.C - 1)];
    float gv[NPX][VEC], xv[NPX][VEC];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const size_t o = static_cast<size_t>(P.pix[k]) * g.C + cg.c0;
      load_vec<T, VEC>(gb + o, gv[k]);
      if (GMASK) load_vec<T, VEC>(xb + o, xv[k]);
    }
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      float ov[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        ov[e] = gv[k][e] * q[e].x + q[e].y * wA[k];
        if (GMASK) accp[k] += q[e].y * xv[k][e];
      }
      if (P.ok[k]) store_vec<T, VEC>(ob + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, ov);
    }
  }
  if (GMASK) {
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const float dot = wave_group_sum(accp[k], t.CS);                   // a pixel's lanes sit in one wave
      if (t.lane == 0 && P.ok[k]) A.gmask[static_cast<size_t>(b) * g.HW + P.pix[k]] = eca_gmask(g, use, den, dot, kb, sv[k]);
    }
  }
}

}  // namespace mgacbam
