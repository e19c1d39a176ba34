// Backward kernels of channels-last (MGACBAM_LAYOUT_NHWC) levels: thread layout and data flow in nhwc.cuh, algebra in bwd.cuh.
#pragma once
#include "bwd.cuh"
#include "nhwc.cuh"

namespace mgacbam {

// ---------------------------------------------------------------------------------------------
// k_bwd_reduce1_nhwc: workgroup = (sample, chunk of rp tiles).  Per chunk A[b,c] = sum_hw gy*x*sa and D[b,c] = sum_hw gy*(v - x)
//   (row sums in LDS in row order, added tile by tile into the chunk's running sums by the channel's one owner thread); per pixel
//   g_pre[b,hw] = a * sa(1-sa) * sum_c ca*gy*x.
//   LDS: [C ca][C A][C D][2 * 256 * VEC row partials]
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_bwd_reduce1_nhwc(const Group<BwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  const float a = softplusf_(*A.p.beta);
  const int C4 = (g.C + 3) & ~3;
  float* s_ca = smem;
  float* s_acc = smem + C4;                                              // [C A][C D]
  float* red = s_acc + 2 * C4;
  for (int c = tid; c < g.C; c += kBlock) { s_ca[c] = A.c.ca[static_cast<size_t>(b) * g.C + c]; s_acc[c] = 0.f; s_acc[C4 + c] = 0.f; }
  float* part = A.s.A_part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * 3 * g.C;
  __syncthreads();
  const int nj = (A.n.ng + CS - 1) / CS, CV = CS * VEC;
  const int t_end = min((chunk + 1) * A.n.rp, A.n.ntile);
  for (int tile = chunk * A.n.rp; tile < t_end; ++tile) {
    const int p0 = tile * A.n.ch;
    bool okp[kNhwcNpx];
    float sav[kNhwcNpx], accp[kNhwcNpx];
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const int p = p0 + k * PR + row;
      okp[k] = p < g.HW;
      sav[k] = okp[k] ? A.c.sa[static_cast<size_t>(b) * g.HW + p] : 0.f;
      accp[k] = 0.f;
    }
    for (int j = 0; j < nj; ++j) {
      const int cgi = lane + j * CS;
      const bool okc = cgi < A.n.ng;
      const int c0 = min(cgi, A.n.ng - 1) * VEC;
      float cav[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) cav[e] = (okc && c0 + e < g.C) ? s_ca[c0 + e] : 0.f;
      float xv[kNhwcNpx][VEC], gv[kNhwcNpx][VEC];
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const size_t o = static_cast<size_t>(okp[k] ? p0 + k * PR + row : 0) * g.C + c0;
        load_vec<T, VEC>(xb + o, xv[k]);
        load_vec<T, VEC>(gb + o, gv[k]);
      }
      float acc[2][VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; }
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const float live = (okp[k] && okc) ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float p = xv[k][e] * gv[k][e] * live;
          accp[k] += cav[e] * p;
          acc[0][e] += p * sav[k];
          acc[1][e] += p * (cav[e] * sav[k] - 1.f);                      // gy*(v - x), summed directly (bwd.cuh)
        }
      }
      nhwc_rows_sum<2, VEC>(acc, red, tid);
      for (int t = tid; t < CV; t += kBlock) {                          // (CV = 512 with 8-element lanes)
        const int c = j * CV + t;
        if (c < g.C) {
          float As = 0.f, Ds = 0.f;
          for (int r = 0; r < PR; ++r) { const int o = r * CV + t; As += red[o]; Ds += red[kBlock * VEC + o]; }
          s_acc[c] += As; s_acc[C4 + c] += Ds;                          // (one owner thread per channel: fixed order over the tiles)
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const float t = wave_group_sum(accp[k], CS);
      if (lane == 0 && okp[k]) A.s.gpre[static_cast<size_t>(b) * g.HW + p0 + k * PR + row] = a * t * sav[k] * (1.f - sav[k]);   // g_sa * sigmoid'
    }
  }
  __syncthreads();
  for (int c = tid; c < g.C; c += kBlock) { part[c] = s_acc[c]; part[g.C + c] = s_acc[C4 + c]; }
}

// ---------------------------------------------------------------------------------------------
// k_bwd_reduce2_nhwc: per-chunk partials of sum_hw x * ([c == cidx]*gp0 + gp1/C)  -> A_part[.., 2, c]  (chunks as k_bwd_reduce1_nhwc)
//   LDS: [256 * VEC row partials] static ; [C running sums] dynamic
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_bwd_reduce2_nhwc(const Group<BwdArgs> G) {
  __shared__ __align__(16) float red[kBlock * VEC];
  extern __shared__ __align__(16) float s_acc[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  const float invC = 1.f / static_cast<float>(g.C);
  const float* gp0 = A.s.gplanes + static_cast<size_t>(b) * 3 * g.HW;
  for (int c = tid; c < g.C; c += kBlock) s_acc[c] = 0.f;
  float* part = A.s.A_part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * 3 * g.C + 2 * g.C;
  const int nj = (A.n.ng + CS - 1) / CS, CV = CS * VEC;
  const int t_end = min((chunk + 1) * A.n.rp, A.n.ntile);
  for (int tile = chunk * A.n.rp; tile < t_end; ++tile) {
    const int p0 = tile * A.n.ch;
    bool okp[kNhwcNpx];
    float g0[kNhwcNpx], g1[kNhwcNpx];
    int ci[kNhwcNpx];
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const int p = p0 + k * PR + row;
      okp[k] = p < g.HW;
      const int pp = okp[k] ? p : 0;
      g0[k] = okp[k] ? gp0[pp] : 0.f;
      g1[k] = okp[k] ? gp0[g.HW + pp] * invC : 0.f;
      ci[k] = A.c.cidx[static_cast<size_t>(b) * g.HW + pp];
    }
    for (int j = 0; j < nj; ++j) {
      const int cgi = lane + j * CS;
      const bool okc = cgi < A.n.ng;
      const int c0 = min(cgi, A.n.ng - 1) * VEC;
      float xv[kNhwcNpx][VEC];
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const int p = okp[k] ? p0 + k * PR + row : 0;
        load_vec<T, VEC>(xb + static_cast<size_t>(p) * g.C + c0, xv[k]);
      }
      float acc[1][VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float wgt = g1[k] + (ci[k] == c0 + e ? g0[k] : 0.f);     // mean backward + max backward
          acc[0][e] += xv[k][e] * wgt;                                   // (g0 = g1 = 0 on pixels past the image)
        }
      }
      if (!okc) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
      }
      nhwc_rows_sum<1, VEC>(acc, red, tid);
      for (int t = tid; t < CV; t += kBlock) {                          // (CV = 512 with 8-element lanes)
        const int c = j * CV + t;
        if (c < g.C) {
          float acc_c = 0.f;
          for (int r = 0; r < PR; ++r) acc_c += red[r * CV + t];
          s_acc[c] += acc_c;                                             // (one owner thread per channel: fixed order over the tiles)
        }
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < g.C; c += kBlock) part[c] = s_acc[c];
}

// ---------------------------------------------------------------------------------------------
// k_bwd_fold_nhwc: workgroup = (sample, block of kNhwcFoldC channels).  Its 4 waves fold a channel's chunk partials with a stride of 4
//   chunks; the 4 results are added in wave order (fixed order).  g_ca = a*A + R, g_z = g_ca * ca(1-ca) -> s.gz ; D -> s.gbq ;
//   pgh[b,cb,j] = sum_{c in block} W2[c,j] g_z[b,c] (channel order)
//   LDS: [3 x 256 wave partials][kNhwcFoldC g_z]
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
  {
    const float* pb = A.s.A_part + static_cast<size_t>(b) * A.n.nchunk * 3 * g.C + cc;
    float As = 0.f, Ds = 0.f, Rs = 0.f;
#pragma unroll 4
    for (int q = grp; q < A.n.nchunk; q += 4) {
      const float* pq = pb + static_cast<size_t>(q) * 3 * g.C;
      As += pq[0]; Ds += pq[g.C]; Rs += pq[2 * g.C];
    }
    s_part[0][tid] = As; s_part[1][tid] = Ds; s_part[2][tid] = Rs;
  }
  __syncthreads();
  if (grp == 0) {
    float As = s_part[0][lane], Ds = s_part[1][lane], Rs = s_part[2][lane];
    for (int r = 1; r < 4; ++r) { As += s_part[0][r * 64 + lane]; Ds += s_part[1][r * 64 + lane]; Rs += s_part[2][r * 64 + lane]; }
    float gz = 0.f;
    if (c < g.C) {
      const size_t o = static_cast<size_t>(b) * g.C + c;
      const float ca = A.c.ca[o];
      gz = (a * As + Rs) * ca * (1.f - ca);
      A.s.gz[o] = gz;
      A.s.gbq[o] = Ds;                                                   // sum_hw gy*(v - x) for this (b,c)
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
//   LDS: [C float4 q][C arg-max][2*hidden][256 scratch]
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC, bool GMASK>
__global__ __launch_bounds__(kBlock) void k_bwd_apply_nhwc(const Group<BwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[8];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const BwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, chunk)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const int p0 = chunk * A.n.ch;
  const float a = softplusf_(*A.p.beta);
  const float Nf = static_cast<float>(g.HW);
  const bool has_mask = A.mask != nullptr;
  const int h = g.hidden;
  float4* s_q = reinterpret_cast<float4*>(smem);
  int* s_am = reinterpret_cast<int*>(smem + 4 * g.C);
  float* s_gh = smem + 5 * g.C;

  // ---- prologue: hidden gradient (channel-block partials in order), q[c], K_b ------------------------------------------------
  {
    const float* pg = A.s.pgh + static_cast<size_t>(b) * A.ncb * h;
    for (int j = tid; j < h; j += kBlock) {
      float p = 0.f;
      for (int q = 0; q < A.ncb; ++q) p += pg[q * h + j];
      s_gh[j] = A.c.h_avg[static_cast<size_t>(b) * h + j] > 0.f ? p : 0.f;
      s_gh[h + j] = A.c.h_mx[static_cast<size_t>(b) * h + j] > 0.f ? p : 0.f;
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
  bool okp[kNhwcNpx];
  float sav[kNhwcNpx], g0[kNhwcNpx], g1[kNhwcNpx], wA[kNhwcNpx], accp[kNhwcNpx];
  int ci[kNhwcNpx], pix[kNhwcNpx];
#pragma unroll
  for (int k = 0; k < kNhwcNpx; ++k) {
    const int p = p0 + k * PR + row;
    okp[k] = row < PR && p < g.HW;
    pix[k] = okp[k] ? p : 0;
    const size_t po = static_cast<size_t>(b) * g.HW + pix[k];
    sav[k] = a * A.c.sa[po];
    g0[k] = A.s.gplanes[static_cast<size_t>(b) * 3 * g.HW + pix[k]];
    g1[k] = A.s.gplanes[static_cast<size_t>(b) * 3 * g.HW + g.HW + pix[k]] * invC;
    const float sv = A.c.planes[(static_cast<size_t>(b) * 3 + 2) * g.HW + pix[k]];
    wA[k] = has_mask ? (use * sv / den + (1.f - use) / Nf) : 1.f / Nf;
    ci[k] = A.c.cidx[po];
    accp[k] = 0.f;
  }
  const int nj = (A.n.ng + CS - 1) / CS;
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    if (cgi >= A.n.ng) break;
    const int c0 = cgi * VEC;
    float4 q[VEC];
    int am[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { const int c = min(c0 + e, g.C - 1); q[e] = s_q[c]; am[e] = s_am[c]; }
    float gv[kNhwcNpx][VEC], xv[kNhwcNpx][VEC];
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const size_t o = static_cast<size_t>(pix[k]) * g.C + c0;
      load_vec<T, VEC>(gb + o, gv[k]);
      if (GMASK) load_vec<T, VEC>(xb + o, xv[k]);
    }
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      float ov[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const int c = c0 + e;
        float r = gv[k][e] * ((1.f - a) + sav[k] * q[e].x);
        r += q[e].x * ((ci[k] == c ? g0[k] : 0.f) + g1[k]);
        r += q[e].y * wA[k] + q[e].w;
        r += (am[e] == pix[k]) ? q[e].z : 0.f;
        ov[e] = r;
        if (GMASK) { if (c < g.C) accp[k] += q[e].y * xv[k][e]; }
      }
      if (okp[k]) store_vec<T, VEC>(ob + static_cast<size_t>(pix[k]) * g.C + c0, ov);
    }
  }
  if (GMASK) {
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const float t = wave_group_sum(accp[k], CS);
      if (lane == 0 && okp[k]) {
        const size_t po = static_cast<size_t>(b) * g.HW + pix[k];
        const float g2 = A.s.gplanes[(static_cast<size_t>(b) * 3 + 2) * g.HW + pix[k]];
        const float sv = A.c.planes[(static_cast<size_t>(b) * 3 + 2) * g.HW + pix[k]];
        const float gs = g2 + (use / den) * (t - kb);
        A.gmask[po] = g.use_sigmoid ? gs * sv * (1.f - sv) : gs;
      }
    }
  }
}

}  // namespace mgacbam
