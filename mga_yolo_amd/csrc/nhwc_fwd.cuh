// Forward kernels of channels-last (MGACBAM_LAYOUT_NHWC) levels: thread layout (NhwcPos, NhwcPix, NhwcGroup, the folds) and data
// flow in nhwc.cuh.
#pragma once
#include "fwd.cuh"    // kSelLogit, mlp_gate_to_lds
#include "nhwc.cuh"
#include "tile.cuh"

namespace mgacbam {

// ---------------------------------------------------------------------------------------------
// k_pool_nhwc: workgroup = (sample, chunk of rp tiles).  Per tile and channel group the rows' sums meet in LDS in row order; the
// channel's owner thread adds them, tile by tile, to the chunk's running values in LDS; the chunk's partials then go to ws.
//   static LDS: red = 3 x 256*VEC row sums [sum x*s][sum x][max], redi = 256*VEC row arg-max pixels
// ---------------------------------------------------------------------------------------------
struct PoolNhwcLds {           // the chunk's running values
  size_t sxs, sx, mx;          // [C] sum x*s | [C] sum x | [C] masked max
  size_t idx;                  // [C] first arg-max pixel (int)
  size_t total;
  __host__ __device__ explicit PoolNhwcLds(const Geo& g) {
    const size_t C = g.C;
    sxs = 0; sx = sxs + C; mx = sx + C; idx = mx + C; total = idx + C;
  }
};
template <typename T, int VEC, bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_pool_nhwc(const Group<FwdArgs> G) {
  __shared__ __align__(16) float red[3 * kBlock * VEC];
  __shared__ __align__(16) int redi[kBlock * VEC];
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const FwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.nchunk, b, chunk)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const PoolNhwcLds L(g);
  float *s_sxs = smem + L.sxs, *s_sx = smem + L.sx, *s_mx = smem + L.mx;
  int* s_idx = reinterpret_cast<int*>(smem + L.idx);
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  float* part = A.ws + (static_cast<size_t>(b) * A.n.nchunk + chunk) * (4 * static_cast<size_t>(g.C) + 4);
  for (int c = t.tid; c < g.C; c += kBlock) { s_sxs[c] = 0.f; s_sx[c] = 0.f; s_mx[c] = -FLT_MAX; s_idx[c] = INT_MAX; }
  float ssum = 0.f;
  const int t_end = min((chunk + 1) * A.n.rp, A.n.ntile);
  for (int tile = chunk * A.n.rp; tile < t_end; ++tile) {
    const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, tile * A.n.ch, g.HW);
    float s[NPX];
    bool sel[NPX];
#pragma unroll
    for (int k = 0; k < NPX; ++k) {
      s[k] = 0.f; sel[k] = P.ok[k];
      if (HAS_MASK && P.ok[k]) {
        const float m = A.mask[static_cast<size_t>(b) * g.HW + P.pix[k]];
        s[k] = g.use_sigmoid ? sigmoid_fast(m) : m;                       // masked_cbam.py:93-94
        sel[k] = g.use_sigmoid ? m > kSelLogit : s[k] > 0.5f;             // masked_cbam.py:116 (fwd.cuh: kSelLogit)
        ssum += s[k];
      }
    }
    for (int j = 0; j < t.nj; ++j) {
      const NhwcGroup cg = nhwc_group_clamped<VEC>(t, A.n, j);
      float acc[3][VEC];                                                  // [sum x*s][sum x][max]
      int im[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) { acc[0][e] = 0.f; acc[1][e] = 0.f; acc[2][e] = -FLT_MAX; im[e] = INT_MAX; }
      float xv[NPX][VEC];
#pragma unroll
      for (int k = 0; k < NPX; ++k) load_vec<T, VEC>(xb + static_cast<size_t>(P.pix[k]) * g.C + cg.c0, xv[k]);
#pragma unroll
      for (int k = 0; k < NPX; ++k) {
        if (!P.ok[k] || !cg.okc) continue;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float v = xv[k][e];
          acc[1][e] += v;
          if (HAS_MASK) acc[0][e] += v * s[k];
          if (sel[k] && v > acc[2][e]) { acc[2][e] = v; im[e] = P.live(k); }   // pixels ascend along k: strict > keeps the first
        }
      }
      nhwc_rows_sum<3, VEC>(acc, red, t.tid);
      // (the arg-max pixel travels as an int: red's barrier pair above also orders these stores against the reads below)
#pragma unroll
      for (int e = 0; e < VEC; ++e) redi[t.tid * VEC + e] = im[e];
      __syncthreads();
      // nhwc_rows_to_channels' row walk with an arg-max as the third column
      for (int u = t.tid; u < t.CV; u += kBlock) {                        // (CV = 512 with 8-element lanes)
        const int c = j * t.CV + u;
        if (c < g.C) {
          float sxs = 0.f, sx = 0.f, vm = -FLT_MAX;
          int ix = INT_MAX;
          for (int r = 0; r < t.PR; ++r) {
            const int o = r * t.CV + u;                                   // element (row r, lane u / VEC, e = u % VEC)
            sxs += red[o]; sx += red[kBlock * VEC + o];
            argmax_combine(vm, ix, red[2 * kBlock * VEC + o], redi[o]);
          }
          s_sxs[c] += sxs; s_sx[c] += sx;                                 // (channel c has ONE owner thread: fixed order over the tiles)
          float cm = s_mx[c];
          int ci = s_idx[c];
          argmax_combine(cm, ci, vm, ix);
          s_mx[c] = cm; s_idx[c] = ci;
        }
      }
    }
  }
  __syncthreads();
  for (int c = t.tid; c < g.C; c += kBlock) {
    part[c] = s_sxs[c]; part[g.C + c] = s_sx[c]; part[2 * g.C + c] = s_mx[c];
    reinterpret_cast<int*>(part)[3 * g.C + c] = s_idx[c];
  }
  if (HAS_MASK) {
    const float S = nhwc_chunk_row_total(ssum, red, t);
    if (t.tid == 0) part[4 * g.C] = S;
  } else if (t.tid == 0) {
    part[4 * g.C] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------
// k_pool_fin: workgroup = (sample, block of kNhwcFoldC channels); nhwc_chunk_fold over the chunk partials, the arg-max column beside
// the sums (ties of the max go to the lower pixel: the first arg-max).  Writes the pooled statistics exactly as k_pool defines them;
// the shared MLP follows as k_mlp.
// ---------------------------------------------------------------------------------------------
template <bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_pool_fin(const Group<FwdArgs> G) {
  __shared__ float s_part[3][kBlock];
  __shared__ int s_pidx[kBlock];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const FwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  const int ncb = (g.C + kNhwcFoldC - 1) / kNhwcFoldC;
  const int b = local / ncb, cb = local - b * ncb;
  const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6, nch = A.n.nchunk;
  const size_t stride = 4 * static_cast<size_t>(g.C) + 4;
  const float* wb = A.ws + static_cast<size_t>(b) * nch * stride;
  float S = 0.f;                                                        // every workgroup of the sample forms S the same way
  if (HAS_MASK) {
    for (int q = lane; q < nch; q += 64) S += wb[q * stride + 4 * g.C];
    S = wave_group_sum(S, 64);
  }
  const int c = cb * kNhwcFoldC + lane;
  const int cc = min(c, g.C - 1);
  float sum[2], vm = -FLT_MAX;                                          // [sum x*s][sum x]
  int im = INT_MAX;
  nhwc_chunk_fold<2>(sum, s_part, nch,
                     [&](int q, float (&s)[2]) {
                       const float* pq = wb + q * stride;
                       s[0] += pq[cc]; s[1] += pq[g.C + cc];
                       argmax_combine(vm, im, pq[2 * g.C + cc], reinterpret_cast<const int*>(pq)[3 * g.C + cc]);
                     },
                     [&](int slot) { s_part[2][slot] = vm; s_pidx[slot] = im; });
  if (grp != 0 || c >= g.C) return;
  for (int r = 1; r < 4; ++r) argmax_combine(vm, im, s_part[2][r * 64 + lane], s_pidx[r * 64 + lane]);
  if (im == INT_MAX) im = 0;                                            // nothing selected: k_pool leaves index 0
  const float sxs = sum[0], sx = sum[1];
  const float Nf = static_cast<float>(g.HW);
  const float use = (S / Nf >= g.thr) ? 1.f : 0.f;                      // masked_cbam.py:97-98
  const float den = clamp_min_nan(S, g.eps);                            // masked_cbam.py:99
  const size_t o = static_cast<size_t>(b) * g.C + c;
  const float gap = sx / Nf;                                            // masked_cbam.py:101
  float avg, mavg, mxo;
  int valid;
  if (HAS_MASK) {
    mavg = sxs / den;                                                   // masked_cbam.py:100
    avg = mavg * use + gap * (1.f - use);                               // masked_cbam.py:102
    valid = isclosef_(vm, -FLT_MAX) ? 0 : 1;                            // masked_cbam.py:120
    mxo = valid ? vm : gap;                                             // masked_cbam.py:121
  } else {
    mavg = gap; avg = gap; valid = 1; mxo = vm;                         // masked_cbam.py:90-91, 107-108
  }
  A.c.avg[o] = avg; A.c.mavg[o] = mavg; A.c.mx[o] = mxo;
  A.c.valid[o] = valid; A.c.amax[o] = im;
  if (cb == 0 && lane == 0) {
    A.c.S[b] = HAS_MASK ? S : 0.f;
    A.c.use[b] = HAS_MASK ? use : 0.f;
    A.c.den[b] = HAS_MASK ? den : 1.f;
  }
}

// ---------------------------------------------------------------------------------------------
// k_chan_nhwc: per pixel max_c u (+ first arg-max channel), mean_c u, sigma(mask)           masked_cbam.py:130,135-138,146
//   NOT on the layer of nhwc.cuh: the kernel keeps its own statement of the layout.  Its okp carries a `row < PR` term that is never
//   false but that the compiler cannot prove; on NhwcPix, without the term, k_chan_nhwc<__half, 4> compiled to another number of waves
//   per SIMD, and with the term on the record other instantiations did.  Dropping the term is a speed change of its own.
// ---------------------------------------------------------------------------------------------
struct ChanNhwcLds {
  size_t ca;                   // [C] the sample's channel gate
  size_t total;
  __host__ __device__ explicit ChanNhwcLds(const Geo& g) : ca(0), total(g.C) {}
};
template <typename T, int VEC, bool HAS_MASK>
__global__ __launch_bounds__(kBlock) void k_chan_nhwc(const Group<FwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const FwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, chunk;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, chunk)) return;
  constexpr int kNhwcNpx = NhwcNpx<VEC>::value;
  const int tid = threadIdx.x, CS = A.n.cs, lane = tid & (CS - 1), row = tid >> A.n.lcs, PR = kBlock >> A.n.lcs;
  const int p0 = chunk * A.n.ch;
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  float* s_ca = smem + ChanNhwcLds(g).ca;
  for (int c = tid; c < g.C; c += kBlock) s_ca[c] = A.c.ca[static_cast<size_t>(b) * g.C + c];
  __syncthreads();
  bool okp[kNhwcNpx];
  float vmax[kNhwcNpx], vsum[kNhwcNpx];
  int vidx[kNhwcNpx];
#pragma unroll
  for (int k = 0; k < kNhwcNpx; ++k) {
    okp[k] = row < PR && p0 + k * PR + row < g.HW;
    vmax[k] = -INFINITY; vsum[k] = 0.f; vidx[k] = lane * VEC;
  }
  const int nj = (A.n.ng + CS - 1) / CS;
  for (int j = 0; j < nj; ++j) {
    const int cgi = lane + j * CS;
    if (cgi >= A.n.ng) break;
    const int c0 = cgi * VEC;
    float xv[kNhwcNpx][VEC];
#pragma unroll
    for (int k = 0; k < kNhwcNpx; ++k) {
      const int p = okp[k] ? p0 + k * PR + row : 0;
      load_vec<T, VEC>(xb + static_cast<size_t>(p) * g.C + c0, xv[k]);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int c = c0 + e;
      if (c >= g.C) break;
      const float cac = s_ca[c];
#pragma unroll
      for (int k = 0; k < kNhwcNpx; ++k) {
        const float u = xv[k][e] * cac;                                  // masked_cbam.py:130
        vsum[k] += u;
        if (u > vmax[k]) { vmax[k] = u; vidx[k] = c; }                   // channels ascend within a lane: strict > keeps the first
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kNhwcNpx; ++k) {
    vsum[k] = wave_group_sum(vsum[k], CS);
    wave_group_argmax(vmax[k], vidx[k], CS);                             // ties -> the lower channel
    if (lane == 0 && okp[k]) {
      const int p = p0 + k * PR + row;
      float* pl = A.c.planes + static_cast<size_t>(b) * 3 * g.HW + p;
      pl[0] = vmax[k];
      pl[g.HW] = vsum[k] / static_cast<float>(g.C);                      // masked_cbam.py:136
      float s = 0.f;
      if (HAS_MASK) { const float m = A.mask[static_cast<size_t>(b) * g.HW + p]; s = g.use_sigmoid ? sigmoid_fast(m) : m; }
      pl[2 * g.HW] = s;                                                  // masked_cbam.py:138,146 (zero plane without a mask)
      A.c.cidx[static_cast<size_t>(b) * g.HW + p] = vidx[k];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k_apply_nhwc: prologue = k x k conv + sigmoid for the tile's pixels (plane window staged in LDS, as k_apply); body = y
// ---------------------------------------------------------------------------------------------
struct ApplyNhwcLds {
  size_t wts;                  // [3*k*k] conv weights, padded to 4 floats
  size_t planes;               // [3][apply_rows][W + k - 1] plane window (apply_rows >= the tile's rows + halo: host bound for this tile size)
  size_t sa;                   // [CH] the tile's spatial gate
  size_t ca;                   // [C] the sample's channel gate
  size_t total;
  __host__ __device__ ApplyNhwcLds(const Geo& g, const Tune& t, const NhwcGeo& n, int k)
      : wts(0), planes(wts + ((3 * k * k + 3) & ~3)), sa(planes + 3 * static_cast<size_t>(t.apply_rows) * (g.W + k - 1)), ca(sa + n.ch),
        total(ca + g.C) {}
};
template <typename T, int VEC, int K>
__global__ __launch_bounds__(kBlock) void k_apply_nhwc(const Group<FwdArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const FwdArgs& A = G.lv[l];
  const Geo& g = A.g;
  int b, tile;
  if (!xcd_sample_part(local, g.B, A.n.ntile, b, tile)) return;
  constexpr int NPX = NhwcNpx<VEC>::value;
  const NhwcPos t = nhwc_pos<VEC>(A.n);
  const int tid = t.tid, CH = A.n.ch;
  const int p0 = tile * CH, p1 = min(p0 + CH, g.HW) - 1;
  const int k = K ? K : g.k, pad = k / 2;
  const int r0 = p0 / g.W, r1 = p1 / g.W;
  const int PW = g.W + k - 1, PH = (r1 - r0 + 1) + k - 1;
  const ApplyNhwcLds L(g, A.t, A.n, k);
  float *wts = smem + L.wts, *planes = smem + L.planes, *s_sa = smem + L.sa, *s_ca = smem + L.ca;
  for (int i = tid; i < 3 * k * k; i += kBlock) wts[i] = A.p.wsa[i];
  for (int c = tid; c < g.C; c += kBlock) s_ca[c] = A.c.ca[static_cast<size_t>(b) * g.C + c];
  const float* pl = A.c.planes + static_cast<size_t>(b) * 3 * g.HW;
  stage_window<12>(planes, 3, PH, PW, r0 - pad, -pad, g, [&](int p, int off) { return pl[static_cast<size_t>(p) * g.HW + off]; });
  __syncthreads();
  for (int tp = tid; tp < CH; tp += kBlock) {
    if (p0 + tp >= g.HW) break;
    const int p = p0 + tp;
    const int py = p / g.W, px = p - py * g.W;
    const float* origin = planes + (py - r0) * PW + px;
    float acc = 0.f;
    if (K) {
      constexpr int KK = K ? K : 1;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int ti = 0; ti < KK; ++ti) {
          const float* rw = origin + q * PH * PW + ti * PW;
          const float* wr = wts + (q * KK + ti) * KK;
#pragma unroll
          for (int tj = 0; tj < KK; ++tj) acc += wr[tj] * rw[tj];
        }
      }
    } else {
      for (int q = 0; q < 3; ++q)
        for (int ti = 0; ti < k; ++ti) {
          const float* rw = origin + q * PH * PW + ti * PW;
          const float* wr = wts + (q * k + ti) * k;
          for (int tj = 0; tj < k; ++tj) acc += wr[tj] * rw[tj];
        }
    }
    const float sa = sigmoidf_(acc);                                     // masked_cbam.py:147
    s_sa[tp] = sa;
    A.c.sa[static_cast<size_t>(b) * g.HW + p] = sa;
  }
  __syncthreads();
  const float a = softplusf_(*A.p.beta);                                 // masked_cbam.py:150-152
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  T* yb = static_cast<T*>(A.y) + static_cast<size_t>(b) * g.HW * g.C;
  const NhwcPix<NPX> P = nhwc_pixels<NPX>(t, p0, g.HW);
  float sav[NPX];
#pragma unroll
  for (int k2 = 0; k2 < NPX; ++k2) sav[k2] = P.ok[k2] ? s_sa[P.pix[k2] - p0] : 0.f;
  for (int j = 0; j < t.nj; ++j) {
    NhwcGroup cg;
    if (!nhwc_group_live<VEC>(t, A.n, j, cg)) break;
    float cav[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) cav[e] = s_ca[min(cg.c0 + e, g.C - 1)];
    float xv[NPX][VEC];
#pragma unroll
    for (int k2 = 0; k2 < NPX; ++k2) load_vec<T, VEC>(xb + static_cast<size_t>(P.pix[k2]) * g.C + cg.c0, xv[k2]);
#pragma unroll
    for (int k2 = 0; k2 < NPX; ++k2) {
      float yv[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float u = xv[k2][e] * cav[e];                             // masked_cbam.py:130
        const float v = u * sav[k2];                                     // masked_cbam.py:148
        yv[e] = xv[k2][e] + a * (v - xv[k2][e]);                         // masked_cbam.py:171
      }
      if (P.ok[k2]) store_vec<T, VEC>(yb + static_cast<size_t>(P.live(k2)) * g.C + cg.c0, yv);
    }
  }
}

}  // namespace mgacbam
