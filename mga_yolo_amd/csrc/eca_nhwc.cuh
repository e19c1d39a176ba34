// Channels-last (MGACBAM_LAYOUT_NHWC) forms of the MaskECA kernels: the thread layout of nhwc.cuh (a workgroup owns a TILE of CH
// consecutive pixels of one sample, CS lanes split a pixel's channels VEC at a time, per-pixel sums are wave shuffles, per-channel sums
// go through LDS in row order), the algebra of eca.cuh.
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

// rows of one pass -> channel sums: thread t < CS*VEC owns channel j*CS*VEC + t and adds the PR rows in row order
template <int N, int VEC>
__device__ __forceinline__ void eca_rows_to_channels(float (&acc)[N][VEC], float* red, int tid, int j, int CS, int PR, int C, float* out,
                                                     size_t out_stride) {
  nhwc_rows_sum<N, VEC>(acc, red, tid);
  const int CV = CS * VEC;
  for (int t = tid; t < CV; t += kBlock) {                                // (CV = 512 with 8-element lanes)
    const int c = j * CV + t;
    if (c < C) {
#pragma unroll
      for (int q = 0; q < N; ++q) {
        float s = 0.f;
        for (int r = 0; r < PR; ++r) s += red[q * kBlock * VEC + r * CV + t];
        out[q * out_stride + c] = s;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_pool_nhwc: workgroup = (sample, chunk of rp tiles).  The workgroup owns its pixels' sigma(mask) and their sum.
//   LDS: [2 x 256*VEC row sums]
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
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  const float* mb = HAS_MASK ? A.mask + static_cast<size_t>(b) * g.HW : nullptr;
  float* splane = A.c.splane + static_cast<size_t>(b) * g.HW;
  float* part = A.part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * eca_nhwc_part_stride(g.C);
  const int nj = (A.n.ng + CS - 1) / CS;
  const int t0 = chunk * A.n.rp, t_end = min(t0 + A.n.rp, A.n.ntile);
  float ssum = 0.f;
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    const bool okc = cgi < A.n.ng;
    const int c0 = min(cgi, A.n.ng - 1) * VEC;
    float acc[NS][VEC];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) acc[q][e] = 0.f;
    for (int tile = t0; tile < t_end; ++tile) {
      const int p0 = tile * A.n.ch;
      float s[kNhwcNpx];
      bool live[kNhwcNpx];
      float xv[kNhwcNpx][VEC];
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const int p = p0 + k * PR + row;
        const bool okp = p < g.HW;
        live[k] = okp && okc;
        load_vec<T, VEC>(xb + static_cast<size_t>(okp ? p : 0) * g.C + c0, xv[k]);
        s[k] = 0.f;
        if (HAS_MASK && okp) {
          const float m = mb[p];
          s[k] = g.use_sigmoid ? sigmoid_fast(m) : m;                     // masked_eca.py:146-147
        }
        if (j == 0 && okp) {
          ssum += s[k];
          if (lane == 0) splane[p] = s[k];                                // (zeros when there is no mask)
        }
      }
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float v = live[k] ? xv[k][e] : 0.f;
          acc[0][e] += v;
          if (HAS_MASK) acc[NS - 1][e] += v * s[k];
        }
    }
    // without a mask only sum x is formed (k_eca_fin reads nothing else)
    eca_rows_to_channels<NS, VEC>(acc, red, tid, j, CS, PR, g.C, part, g.C);
  }
  // sum of s over the chunk: rows in order (every lane of a row holds the row's sum)
  __syncthreads();
  if (lane == 0) red[row] = ssum;
  __syncthreads();
  if (tid == 0) { float t = 0.f; for (int r = 0; r < PR; ++r) t += red[r]; part[2 * g.C] = t; }
}

// ---------------------------------------------------------------------------------------------
// k_eca_fin: workgroup = (sample, block of kNhwcFoldC channels); its 4 waves fold the chunk partials of a channel with a stride of 4
// chunks, the 4 results are added in wave order.  Writes the statistics exactly as k_eca_pool defines them.
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
  float sxs = 0.f, sx = 0.f;
#pragma unroll 4
  for (int q = grp; q < nch; q += 4) {
    const float* pq = wb + q * stride;
    sx += pq[cc];
    if (HAS_MASK) sxs += pq[g.C + cc];
  }
  s_part[0][tid] = sxs; s_part[1][tid] = sx;
  __syncthreads();
  if (grp != 0 || c >= g.C) return;
  for (int r = 1; r < 4; ++r) { sxs += s_part[0][r * 64 + lane]; sx += s_part[1][r * 64 + lane]; }
  const float Nf = static_cast<float>(g.HW);
  const float use = (S / Nf >= g.thr) ? 1.f : 0.f;                        // masked_eca.py:152-153, 159
  const float den = fmaxf(S, g.eps);                                      // :156, 164
  const size_t o = static_cast<size_t>(b) * g.C + c;
  const float gap = sx / Nf;
  const float mavg = HAS_MASK ? sxs / den : gap;                          // :157, 165
  A.c.mavg[o] = mavg;
  A.c.avg[o] = HAS_MASK ? mavg * use + gap * (1.f - use) : gap;           // :161
  if (cb == 0 && lane == 0) {
    A.c.S[b] = HAS_MASK ? S : 0.f;
    A.c.use[b] = HAS_MASK ? use : 0.f;
    A.c.den[b] = HAS_MASK ? den : 1.f;
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_apply_nhwc: workgroup = (sample, tile).  Prologue: the sample's C gates into LDS (tile 0 also saves w); body: y = x * gate[c]
//   LDS: [C gate]
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(kBlock) void k_eca_apply_nhwc(const Group<EcaFwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaFwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const int p0 = tile * A.n.ch;
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  T* yb = static_cast<T*>(A.y) + sb;
  const float a = softplusf_(*A.beta);
  float* s_gate = smem;
  for (int c = tid; c < g.C; c += kBlock) {
    const float w = eca_gate_w(A.c.avg + static_cast<size_t>(b) * g.C, A.w1d, g.k, g.C, c);
    s_gate[c] = 1.f + a * (w - 0.5f);                                     // masked_eca.py:190
    if (tile == 0) A.c.w[static_cast<size_t>(b) * g.C + c] = w;
  }
  __syncthreads();
  int pix[kNhwcNpx];
  bool okp[kNhwcNpx];
#pragma unroll
  for (int k = 0; k < kNhwcNpx; ++k) {
    const int p = p0 + k * PR + row;
    okp[k] = p < g.HW;
    pix[k] = okp[k] ? p : 0;
  }
  const int nj = (A.n.ng + CS - 1) / CS;
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    if (cgi >= A.n.ng) break;
    const int c0 = cgi * VEC;
    float gv[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) gv[e] = s_gate[min(c0 + e, g.C - 1)];
    float xv[kNhwcNpx][VEC];
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) load_vec<T, VEC>(xb + static_cast<size_t>(pix[k]) * g.C + c0, xv[k]);
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      float yv[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) yv[e] = xv[k][e] * gv[e];
      if (okp[k]) store_vec<T, VEC>(yb + static_cast<size_t>(pix[k]) * g.C + c0, yv);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_reduce_nhwc: per-chunk partials of gg[b,c] = sum_hw gy*x   (chunks as k_eca_pool_nhwc)
//   LDS: [256*VEC row sums]
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
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  float* part = A.part + (static_cast<size_t>(b) * A.n.nchunk + chunk) * g.C;
  const int nj = (A.n.ng + CS - 1) / CS;
  const int t0 = chunk * A.n.rp, t_end = min(t0 + A.n.rp, A.n.ntile);
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    const bool okc = cgi < A.n.ng;
    const int c0 = min(cgi, A.n.ng - 1) * VEC;
    float acc[1][VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[0][e] = 0.f;
    for (int tile = t0; tile < t_end; ++tile) {
      const int p0 = tile * A.n.ch;
      float xv[kNhwcNpx][VEC], gv[kNhwcNpx][VEC];
      bool live[kNhwcNpx];
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const int p = p0 + k * PR + row;
        const bool okp = p < g.HW;
        live[k] = okp && okc;
        const size_t o = static_cast<size_t>(okp ? p : 0) * g.C + c0;
        load_vec<T, VEC>(xb + o, xv[k]);
        load_vec<T, VEC>(gb + o, gv[k]);
      }
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[0][e] += live[k] ? xv[k][e] * gv[k][e] : 0.f;
    }
    eca_rows_to_channels<1, VEC>(acc, red, tid, j, CS, PR, g.C, part, 0);
  }
}

// ---------------------------------------------------------------------------------------------
// k_eca_fold: workgroup = (sample, block of kNhwcFoldC channels): gg[b,c] = chunk partials folded as k_eca_fin folds its own
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
  float s = 0.f;
#pragma unroll 4
  for (int q = grp; q < A.n.nchunk; q += 4) s += pb[static_cast<size_t>(q) * g.C];
  s_part[tid] = s;
  __syncthreads();
  if (grp != 0 || c >= g.C) return;
  for (int r = 1; r < 4; ++r) s += s_part[r * 64 + lane];
  A.s.gg[static_cast<size_t>(b) * g.C + c] = s;
}

// ---------------------------------------------------------------------------------------------
// k_eca_bwd_nhwc: gx = gy*g + g_avg*wA ; gmask = (use/den) * (sum_c g_avg*x - K_b) * s(1-s)      (eca.cuh k_eca_bwd, NHWC)
//   prologue per workgroup (its sample): gy1 = a*gg*w(1-w) -> LDS; g_avg = conv1d^T(gy1) ; q[c] = {g, g_avg} ; K_b
//   the level's first 16 workgroups are the parameter-gradient roles (eca_params_body: layout-free)
//   LDS: [C gy1][2C q]
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC, bool GMASK>
__global__ __launch_bounds__(kBlock) void k_eca_bwd_nhwc(const Group<EcaBwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  __shared__ float red[8];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const EcaBwdArgs& A = G.lv[l];
  if (local < kEcaRoles) { eca_params_body(A, local, red); return; }     // 16 role ids keep the streaming ids XCD-aligned
  local -= kEcaRoles;
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const int p0 = tile * A.n.ch;
  const float a = softplusf_(*A.beta);
  const float Nf = static_cast<float>(g.HW);
  const bool has_mask = A.mask != nullptr;
  const int k = g.k, pad = k / 2;
  const int C2 = (g.C + 1) & ~1;                                         // q is float2: keep it 8-byte aligned
  float* s_gy1 = smem;
  float2* s_q = reinterpret_cast<float2*>(smem + C2);
  for (int c = tid; c < g.C; c += kBlock) {
    const size_t o = static_cast<size_t>(b) * g.C + c;
    const float w = A.c.w[o];
    s_gy1[c] = a * A.s.gg[o] * w * (1.f - w);
  }
  __syncthreads();
  const float live = (has_mask && A.c.S[b] >= g.eps) ? 1.f : 0.f;
  float kpart = 0.f;
  for (int c = tid; c < g.C; c += kBlock) {
    float ga = 0.f;
    for (int t = 0; t < k; ++t) {                                        // conv1d backward w.r.t. its input
      const int cc = c - t + pad;
      if (cc >= 0 && cc < g.C) ga += A.w1d[t] * s_gy1[cc];
    }
    const size_t o = static_cast<size_t>(b) * g.C + c;
    s_q[c] = make_float2(1.f + a * (A.c.w[o] - 0.5f), ga);
    kpart += ga * A.c.mavg[o] * live;
  }
  kpart = block_sum(kpart, tid, red);                                    // (its barriers publish s_q)
  if (tid == 0) red[7] = kpart;
  __syncthreads();
  const float kb = red[7];

  const size_t sb = static_cast<size_t>(b) * g.HW * g.C;
  const T* xb = static_cast<const T*>(A.x) + sb;
  const T* gb = static_cast<const T*>(A.gy) + sb;
  T* ob = static_cast<T*>(A.gx) + sb;
  const float use = A.c.use[b], den = A.c.den[b];
  bool okp[kNhwcNpx];
  int pix[kNhwcNpx];
  float sv[kNhwcNpx], wA[kNhwcNpx], accp[kNhwcNpx];
#pragma unroll
  for (int kk = 0; kk < kNhwcNpx; ++kk) {
    const int p = p0 + kk * PR + row;
    okp[kk] = p < g.HW;
    pix[kk] = okp[kk] ? p : 0;
    sv[kk] = A.c.splane[static_cast<size_t>(b) * g.HW + pix[kk]];
    wA[kk] = has_mask ? (use * sv[kk] / den + (1.f - use) / Nf) : 1.f / Nf;
    accp[kk] = 0.f;
  }
  const int nj = (A.n.ng + CS - 1) / CS;
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    if (cgi >= A.n.ng) break;
    const int c0 = cgi * VEC;
    float2 q[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[e] = s_q[min(c0 + e, g.C - 1)];
    float gv[kNhwcNpx][VEC], xv[kNhwcNpx][VEC];
#pragma unroll
    for (int kk = 0; kk < kNhwcNpx; ++kk) {
      const size_t o = static_cast<size_t>(pix[kk]) * g.C + c0;
      load_vec<T, VEC>(gb + o, gv[kk]);
      if (GMASK) load_vec<T, VEC>(xb + o, xv[kk]);
    }
#pragma unroll
    for (int kk = 0; kk < kNhwcNpx; ++kk) {
      float ov[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        ov[e] = gv[kk][e] * q[e].x + q[e].y * wA[kk];
        if (GMASK) accp[kk] += q[e].y * xv[kk][e];
      }
      if (okp[kk]) store_vec<T, VEC>(ob + static_cast<size_t>(pix[kk]) * g.C + c0, ov);
    }
  }
  if (GMASK) {
#pragma unroll
    for (int kk = 0; kk < kNhwcNpx; ++kk) {
      const float t = wave_group_sum(accp[kk], CS);                      // a pixel's lanes sit in one wave
      if (lane == 0 && okp[kk]) {
        const float gs = (use / den) * (t - kb);
        A.gmask[static_cast<size_t>(b) * g.HW + pix[kk]] = g.use_sigmoid ? gs * sv[kk] * (1.f - sv[kk]) : gs;
      }
    }
  }
}

}  // namespace mgacbam
