// Backward kernels of channels-last (MGACBAM_LAYOUT_NHWC) levels: thread layout (NhwcPos, NhwcPix, NhwcGroup, the folds) and data
// flow in nhwc.cuh, algebra in bwd.cuh.
#pragma once
#include "bwd.cuh"
#include "nhwc.cuh"

namespace mgacbam {

// ---------------------------------------------------------------------------------------------
// k_bwd_reduce1_nhwc: workgroup = (sample, chunk of rp tiles).  Per chunk A[b,c] = sum_hw gy*x*sa and D[b,c] = sum_hw gy*(v - x)
//   (row sums in LDS in row order, added tile by tile into the chunk's running sums by the channel's one owner thread); per pixel
//   g_pre[b,hw] = a * sa(1-sa) * sum_c ca*gy*x.
// ---------------------------------------------------------------------------------------------
struct Reduce1NhwcLds {
  size_t ca;                   // [C] the sample's channel gate, padded to 4 floats
  size_t A, D;                 // [C] the chunk's running sums of A and of D, padded alike
  size_t red;                  // [2][256 * VEC] row sums of a pass
  size_t total;
  __host__ __device__ Reduce1NhwcLds(const Geo& g, int vec) {
    const size_t C4 = (static_cast<size_t>(g.C) + 3) & ~static_cast<size_t>(3);
    ca = 0; A = ca + C4; D = A + C4; red = D + C4; total = red + 2 * kBlock * vec;
  }
};
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_bwd_reduce1_nhwc(const Group<BwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  const float a = softplusf_(*A.p.beta);
  const Reduce1NhwcLds L(g, VEC);
  float *s_ca = smem + L.ca, *s_A = smem + L.A, *s_D = smem + L.D, *red = smem + L.red;
  for (int c = t.tid; c < g.C; c += kBlock) { s_ca[c] = A.c.ca[static_cast<size_t>(b) * g.C + c]; s_A[c] = 0.f; s_D[c] = 0.f; }
  float* part = A.s.A_part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * 3 * g.C;
  __syncthreads();
  const int t_end = min((chunk + 1) * A.n.rp, A.n.ntile);
  for (int tile = chunk * A.n.rp; tile < t_end; ++tile) {
    const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
    float sav[NPX], accp[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      sav[k] = P.ok[k] ? A.c.sa[static_cast<size_t>(b) * g.HW + P.pix[k]] : 0.f;
      accp[k] = 0.f;
    }
    for (int j = 0; j < t.nj; ++j) {
      const NhwcGroup cg = nhwc_group_clamped<VEC>(t, A.n, j);
      float cav[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) cav[e] = (cg.okc && cg.c0 + e < g.C) ? s_ca[cg.c0 + e] : 0.f;
      float xv[NPX][VEC], gv[NPX][VEC];
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        const size_t o = static_cast<size_t>(P.pix[k]) * g.C + cg.c0;
        load_vec<T, VEC>(xb + o, xv[k]);
        load_vec<T, VEC>(gb + o, gv[k]);
      }
      float acc[2][VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        const float live = (P.ok[k] && cg.okc) ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float p = xv[k][e] * gv[k][e] * live;
          accp[k] += cav[e] * p;
          acc[0][e] += p * sav[k];
          acc[1][e] += p * (cav[e] * sav[k] - 1.f);                      // gy*(v - x), summed directly (bwd.cuh)
        }
      }
      // (one owner thread per channel: fixed order over the tiles)
      nhwc_rows_to_channels<2, VEC>(acc, red, t, j, g.C, [&](int c, const float (&sum)[2]) { s_A[c] += sum[0]; s_D[c] += sum[1]; });
    }
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const float dot = wave_group_sum(accp[k], t.CS);
      // (the index as the kernel always formed it, a 64-bit sum whose uniform part stays in scalar registers: with
      //  b * HW + live(k) the compiler keeps 4 more VGPRs, a wave per SIMD at VEC 1 and 8)
      if (t.lane == 0 && P.ok[k])
        A.s.gpre[static_cast<size_t>(b) * g.HW + P.p0 + k * P.PR + P.row] = a * dot * sav[k] * (1.f - sav[k]);   // g_sa * sigmoid'
    }
  }
  __syncthreads();
  for (int c = t.tid; c < g.C; c += kBlock) { part[c] = s_A[c]; part[g.C + c] = s_D[c]; }
}

// ---------------------------------------------------------------------------------------------
// k_bwd_reduce2_nhwc: per-chunk partials of sum_hw x * ([c == cidx]*gp0 + gp1/C)  -> A_part[.., 2, c]  (chunks as k_bwd_reduce1_nhwc)
//   static LDS: red = 256 * VEC row sums of a pass
// ---------------------------------------------------------------------------------------------
struct Reduce2NhwcLds {
  size_t acc;                  // [C] the chunk's running sums
  size_t total;
  __host__ __device__ explicit Reduce2NhwcLds(const Geo& g) : acc(0), total(g.C) {}
};
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_bwd_reduce2_nhwc(const Group<BwdArgs> G) {
  __shared__ __align__(16) float red[kBlock * VEC];
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  const float invC = 1.f / static_cast<float>(g.C);
  const float* gp0 = A.s.gplanes + static_cast<size_t>(b) * 3 * g.HW;
  float* s_acc = smem + Reduce2NhwcLds(g).acc;
  for (int c = t.tid; c < g.C; c += kBlock) s_acc[c] = 0.f;
  float* part = A.s.A_part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * 3 * g.C + 2 * g.C;
  const int t_end = min((chunk + 1) * A.n.rp, A.n.ntile);
  for (int tile = chunk * A.n.rp; tile < t_end; ++tile) {
    const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
    float g0[NPX], g1[NPX];
    int ci[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      g0[k] = P.ok[k] ? gp0[P.pix[k]] : 0.f;
      g1[k] = P.ok[k] ? gp0[g.HW + P.pix[k]] * invC : 0.f;
      ci[k] = A.c.cidx[static_cast<size_t>(b) * g.HW + P.pix[k]];
    }
    for (int j = 0; j < t.nj; ++j) {
      const NhwcGroup cg = nhwc_group_clamped<VEC>(t, A.n, j);
      float xv[NPX][VEC];
#pragma unroll
      for (int k = 0; k < NPX; ++k) load_vec<T, VEC>(xb + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, xv[k]);
      float acc[1][VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float wgt = g1[k] + (ci[k] == cg.c0 + e ? g0[k] : 0.f);  // mean backward + max backward
          acc[0][e] += xv[k][e] * wgt;                                   // (g0 = g1 = 0 on pixels past the image)
        }
      }
      if (!cg.okc) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
      }
      // (one owner thread per channel: fixed order over the tiles)
      nhwc_rows_to_channels<1, VEC>(acc, red, t, j, g.C, [&](int c, const float (&sum)[1]) { s_acc[c] += sum[0]; });
    }
  }
  __syncthreads();
  for (int c = t.tid; c < g.C; c += kBlock) part[c] = s_acc[c];
}

// ---------------------------------------------------------------------------------------------
// k_bwd_fold_nhwc: workgroup = (sample, block of kNhwcFoldC channels): nhwc_chunk_fold over a channel's chunk partials of A, D and R.
//   g_ca = a*A + R, g_z = g_ca * ca(1-ca) -> s.gz ; D -> s.gbq ; pgh[b,cb,j] = sum_{c in block} W2[c,j] g_z[b,c] (channel order)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bwd_fold_nhwc(const Group<BwdArgs> G) {
  __shared__ float s_part[3][kBlock];
  __shared__ float s_gz[kNhwcFoldC];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  const int b = local / A.ncb, cb = local - b * A.ncb;
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
  const int c = cb * kNhwcFoldC + lane, cc = min(c, g.C - 1);
  const float a = softplusf_(*A.p.beta);
  const float* pb = A.s.A_part + static_cast<size_t>(b) * A.n.nchunk * 3 * g.C + cc;
  float sum[3];                                                          // [A][D][R]
  nhwc_chunk_fold<3>(sum, s_part, A.n.nchunk, [&](int q, float (&s)[3]) {
    const float* pq = pb + static_cast<size_t>(q) * 3 * g.C;
    s[0] += pq[0]; s[1] += pq[g.C]; s[2] += pq[2 * g.C];
  });
  if (grp == 0) {
    float gz = 0.f;
    if (c < g.C) {
      const size_t o = static_cast<size_t>(b) * g.C + c;
      const float ca = A.c.ca[o];
      gz = (a * sum[0] + sum[2]) * ca * (1.f - ca);
      A.s.gz[o] = gz;
      A.s.gbq[o] = sum[1];                                               // sum_hw gy*(v - x) for this (b,c)
    }
    s_gz[lane] = gz;
  }
  __syncthreads();
  const int h = g.hidden, nc = min(kNhwcFoldC, g.C - cb * kNhwcFoldC);
  for (int j = tid; j < h; j += kBlock) {
    float p = 0.f;
    for (int k2 = 0; k2 < nc; ++k2) p += A.p.w2[static_cast<size_t>(cb * kNhwcFoldC + k2) * h + j] * s_gz[k2];
    A.s.pgh[(static_cast<size_t>(b) * A.ncb + cb) * h + j] = p;
  }
}

// ---------------------------------------------------------------------------------------------
// k_bwd_apply_nhwc   (bwd.cuh k_bwd_apply, NHWC)
//   gx = gy*((1-a) + a*sa*ca) + ca*([c==cidx]*gp0 + gp1/C) + g_avg*wA + [hw==amax]*g_mx + g_mx_uni
//   gmask = (gp2 + (use/den) * (sum_c g_avg*x - K_b)) * s(1-s)
//   static LDS: red = block_sum's per-wave slots + K_b
// ---------------------------------------------------------------------------------------------
struct BwdApplyNhwcLds {
  size_t q;                    // [C] float4 {ca, g_avg, g_mx to the arg-max pixel, g_mx spread uniformly}
  size_t am;                   // [C] arg-max pixel (int), -1 where the channel has none
  size_t gh;                   // [2][hidden] hidden gradient of the avg and of the max branch
  size_t total;
  __host__ __device__ explicit BwdApplyNhwcLds(const Geo& g) : q(0), am(q + 4 * static_cast<size_t>(g.C)), gh(am + g.C), total(gh + 2 * g.hidden) {}
};
template <typename T, int VEC, bool GMASK>
__global__ __launch_bounds__(kBlock) void k_bwd_apply_nhwc(const Group<BwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[8];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const int tid = t.tid;
  const float a = softplusf_(*A.p.beta);
  const float Nf = static_cast<float>(g.HW);
  const bool has_mask = A.mask != nullptr;
  const int h = g.hidden;
  const BwdApplyNhwcLds L(g);
  float4* s_q = reinterpret_cast<float4*>(smem + L.q);
  int* s_am = reinterpret_cast<int*>(smem + L.am);
  float* s_gh = smem + L.gh;

  // ---- prologue: hidden gradient (channel-block partials in order), q[c], K_b ------------------------------------------------
  {
    const float* pg = A.s.pgh + static_cast<size_t>(b) * A.ncb * h;
    for (int j = tid; j < h; j += kBlock) {
      float p = 0.f;
      for (int q = 0; q < A.ncb; ++q) p += pg[q * h + j];
      s_gh[j] = relu_passes(A.c.h_avg[static_cast<size_t>(b) * h + j]) ? p : 0.f;
      s_gh[h + j] = relu_passes(A.c.h_mx[static_cast<size_t>(b) * h + j]) ? p : 0.f;
    }
  }
  __syncthreads();
  const float live = (has_mask && A.c.S[b] >= g.eps) ? 1.f : 0.f;     // clamp_min passes grad only when not clamped
  float kpart = 0.f;
  for (int c = tid; c < g.C; c += kBlock) {
    float ga = 0.f, gm = 0.f;
    for (int j = 0; j < h; ++j) { const float wv = A.p.w1[static_cast<size_t>(j) * g.C + c]; ga += wv * s_gh[j]; gm += wv * s_gh[h + j]; }
    const size_t o = static_cast<size_t>(b) * g.C + c;
    const int valid = A.c.valid[o];
    float4 q;
    q.x = A.c.ca[o];
    q.y = ga;                                                            // g_avg
    q.z = valid ? gm : 0.f;                                              // routed to the arg-max position
    q.w = valid ? 0.f : gm / Nf;                                         // GAP fallback: spread uniformly
    s_q[c] = q;
    s_am[c] = valid ? A.c.amax[o] : -1;
    kpart += ga * A.c.mavg[o] * live;
  }
  kpart = block_sum(kpart, tid, red);                                    // (its barriers publish s_q)
  if (tid == 0) red[7] = kpart;
  __syncthreads();
  const float kb = red[7];

  // ---- body ----------------------------------------------------------------------------------------------------------------
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  T* ob = static_cast<T*>(A.gx) + sb;
  const float use = A.c.use[b], den = A.c.den[b];
  const float invC = 1.f / static_cast<float>(g.C);
  const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
  float sav[NPX], g0[NPX], g1[NPX], wA[NPX], accp[NPX];
  int ci[NPX];
#pragma unroll
  for (int k = 0; k < NPX; ++k) {
    const size_t po = static_cast<size_t>(b) * g.HW + P.pix[k];
    sav[k] = a * A.c.sa[po];
    g0[k] = A.s.gplanes[static_cast<size_t>(b) * 3 * g.HW + P.pix[k]];
    g1[k] = A.s.gplanes[static_cast<size_t>(b) * 3 * g.HW + g.HW + P.pix[k]] * invC;
    const float sv = A.c.planes[(static_cast<size_t>(b) * 3 + 2) * g.HW + P.pix[k]];
    wA[k] = has_mask ? (use * sv / den + (1.f - use) / Nf) : 1.f / Nf;
    ci[k] = A.c.cidx[po];
    accp[k] = 0.f;
  }
  for (int j = 0; j < t.nj; ++j) {
    NhwcGroup cg;
    if (!nhwc_group_live<VEC>(t, A.n, j, cg)) break;
    float4 q[VEC];
    int am[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { const int c = min(cg.c0 + e, g.C - 1); q[e] = s_q[c]; am[e] = s_am[c]; }
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
        const int c = cg.c0 + e;
        float r = gv[k][e] * ((1.f - a) + sav[k] * q[e].x);
        r += q[e].x * ((ci[k] == c ? g0[k] : 0.f) + g1[k]);
        r += q[e].y * wA[k] + q[e].w;
        r += (am[e] == P.pix[k]) ? q[e].z : 0.f;
        ov[e] = r;
        if (GMASK) { if (c < g.C) accp[k] += q[e].y * xv[k][e]; }
      }
      if (P.ok[k]) store_vec<T, VEC>(ob + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, ov);
    }
  }
  if (GMASK) {
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      const float dot = wave_group_sum(accp[k], t.CS);
      if (t.lane == 0 && P.ok[k]) {
        const size_t po = static_cast<size_t>(b) * g.HW + P.pix[k];
        const float g2 = A.s.gplanes[(static_cast<size_t>(b) * 3 + 2) * g.HW + P.pix[k]];
        const float sv = A.c.planes[(static_cast<size_t>(b) * 3 + 2) * g.HW + P.pix[k]];
        const float gs = g2 + (use / den) * (dot - kb);
        A.gmask[po] = g.use_sigmoid ? gs * sv * (1.f - sv) : gs;
      }
    }
  }
}

}  // namespace mgacbam
