// MaskSPADE (mga_yolo/nn/modules/masked_spade.py): y = gamma(s) * norm(x) + beta(s) on the device.
//   s = sigmoid(mask) | mask,  h = relu(conv3x3(s; w0) + b0)  (hid planes),  gamma = conv3x3(h; wg) + bg,  beta = conv3x3(h; wb) + bb
// The block's arithmetic is the two hid -> C convolutions (1152 * C MACs per pixel).  They run on the matrix cores as implicit GEMMs over
// pixel tiles of kSpPx = 128 pixels (TH rows x TW columns, TW chosen per level so that the tiling wastes the fewest pixels): h of the tile
// (with its 1-pixel halo) is formed in LDS from the staged mask (2-pixel halo) and never reaches memory, nine shifted K = hid slabs feed
// the MFMAs, and the epilogue applies the normalisation and the FiLM to the accumulators and writes y once.
//
// One MMA step is K = 16 for every element type (mma16): fp32 features issue four v_mfma_f32_16x16x4_f32, fp16 / bf16 features ONE native
// v_mfma_f32_16x16x16_{f16,bf16} (the operand layouts of head.cuh).  Slot i of the lane group g = lane / 16 holds k = 4 g + i in BOTH operands, which is
// the native half layout and, for the four fp32 issues, a permutation of k applied to A and B alike.  Operands are the fp32 values the
// loads produced; the half forms round them to the feature type when the operand is formed, accumulation is fp32.
//   D: lane l, register v = row 4 (l / 16) + v, column l % 16.
//
// Backward, plain launches (no in-launch hand-offs): k_spade_bwd_reduce + k_spade_bwd_fin (the four per-plane sums, bias gradients and
// the normalisation's two means), k_spade_dw (split-K over pixel chunks, partials summed in a fixed order by k_spade_dw_fin),
// k_spade_dh (implicit transposed conv, ReLU mask, the 9 tap planes of ds and the dW0 / db0 partials), k_spade_gmask + k_spade_w0_fin,
// and k_spade_ew for gx.  Every reduction has a fixed order: results are bit-reproducible run to run.
#pragma once
#include "common.cuh"

namespace mgacbam {

typedef float sp_v4f32 __attribute__((ext_vector_type(4)));
typedef short sp_v4i16 __attribute__((ext_vector_type(4)));
typedef _Float16 sp_v4f16 __attribute__((ext_vector_type(4)));
typedef __bf16 sp_v4bf16 __attribute__((ext_vector_type(4)));

constexpr int kSpPx = 128;          // pixels of a tile = 8 N tiles of 16
constexpr int kSpNT = kSpPx / 16;
constexpr int kSpMaxHid = 64;
constexpr int kSpDhCC = 32;         // channels of g_gamma / g_beta staged per round of k_spade_dh
constexpr int kSpAStride = kSpPx + 4;

struct SpadeArgs {
  const void* x; const float* mask; void* y; void* gamma;      // gamma: ctx plane set (feature dtype) or null
  const void* gy; void* gx; float* gmask;
  const float* w0; const float* b0; const float* wg; const float* bg; const float* wb; const float* bb;
  float* rmean; float* rvar; long long* nbt;
  float* gw0; float* gb0; float* gwg; float* gbg; float* gwb; float* gbb;
  float* mean; float* rstd;          // ctx: [B*C] each (batch norm: the per-channel value repeated for every sample)
  float* wpack;                      // ctx: [2][9][C][hid]  (gamma | beta weights, tap-major: A operand of the forward)
  float* wpackT;                     // ctx: [2][9][hid][C]  (A operand of k_spade_dh)
  float* red;                        // scratch: [B*C][4] = sum g, sum g*xhat, sum gy*xhat, sum gy  (g = gy * gamma)
  float* stat;                       // scratch: [B*C][2] = mean g, mean g*xhat over the normalisation's set (0 for batch norm in eval)
  float* dwpart;                     // scratch: [nchunk][2][C][hid*9]
  float* u;                          // scratch: [B][9][HW] tap planes of ds
  float* w0part;                     // scratch: [B*tiles][hid*10]
  int B, C, H, W, HW, hid;
  int bn, train, use_sigmoid, has_mask;
  float eps, momentum;
  int TW, TH, ltw, tiles_x, tiles;   // pixel tiling (TW * TH = kSpPx, TW = 1 << ltw)
  int cblk, ncb;                     // forward: channels per workgroup, channel blocks
  int nchunk, tpc;                   // k_spade_dw: pixel chunks, tiles per chunk
};

template <typename T> struct SpMma {
  __device__ static __forceinline__ sp_v4f32 mma(const float (&a)[4], const float (&b)[4], sp_v4f32 c) {
    if constexpr (sizeof(T) == 2 && !__is_same(T, bf16_t)) {
      const sp_v4f16 ha = {static_cast<_Float16>(a[0]), static_cast<_Float16>(a[1]), static_cast<_Float16>(a[2]), static_cast<_Float16>(a[3])};
      const sp_v4f16 hb = {static_cast<_Float16>(b[0]), static_cast<_Float16>(b[1]), static_cast<_Float16>(b[2]), static_cast<_Float16>(b[3])};
      return __builtin_amdgcn_mfma_f32_16x16x16f16(ha, hb, c, 0, 0, 0);
    } else if constexpr (sizeof(T) == 2) {
      const sp_v4bf16 ha = {static_cast<__bf16>(a[0]), static_cast<__bf16>(a[1]), static_cast<__bf16>(a[2]), static_cast<__bf16>(a[3])};
      const sp_v4bf16 hb = {static_cast<__bf16>(b[0]), static_cast<__bf16>(b[1]), static_cast<__bf16>(b[2]), static_cast<__bf16>(b[3])};
      return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(sp_v4i16, ha), __builtin_bit_cast(sp_v4i16, hb), c, 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[i], c, 0, 0, 0);
      return c;
    }
  }
};
__device__ __forceinline__ void ld4(const float* p, float (&o)[4]) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

template <int N> __device__ __forceinline__ void ldn(const float* p, float (&o)[N]) {
#pragma unroll
  for (int k = 0; k < N; k += 4) { const float4 v = *reinterpret_cast<const float4*>(p + k); o[k] = v.x; o[k + 1] = v.y; o[k + 2] = v.z; o[k + 3] = v.w; }
}

// The per-element arithmetic that reads or writes a feature element, one function per expression.  The NCHW kernels here and the
// channels-last ones (NHWC = true, spade_nhwc.cuh) both call these, so an expression is contracted to FMAs the same way in either layout:
// a channels-last level gives the NCHW level's bits.
__device__ __forceinline__ float sp_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float sp_ggamma(float gy, float x, float mean, float rstd) { return gy * (x - mean) * rstd; }
__device__ __forceinline__ float sp_film(float gm, float xh, float beta) { return fmaf(gm, xh, beta); }
__device__ __forceinline__ float sp_gx_inner(float gv, float m1, float xh, float m2) { return gv - m1 - xh * m2; }
// The element a * b of an output of type T (k_spade_ew: xhat = (x - mean) * rstd, gx = rstd * inner).  For fp16 the compiler folds the
// product and the conversion of scalar code into ONE v_fma_mixlo_f16 -- the exact product rounded once -- but multiplies and then packs
// two conversions (two roundings, rarely another fp16) in vector code.  The folded form is what the NCHW kernel has always computed;
// it is spelled out here so that both layouts compute it whatever the code around it looks like.
template <typename T> __device__ __forceinline__ T sp_product_to(float a, float b) {
  if constexpr (__is_same(T, __half)) {
    unsigned r;                                              // (the instruction writes the low half; the high half is not used)
    asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return __builtin_bit_cast(__half, static_cast<unsigned short>(r));
  } else {
    return from_f32<T>(a * b);
  }
}
__device__ __forceinline__ void sp_red_terms(float (&s)[4], float gyv, float xh, float gv) {   // gv = gyv * gamma | gyv
  s[0] += gv; s[1] = fmaf(gv, xh, s[1]); s[2] = fmaf(gyv, xh, s[2]); s[3] += gyv;
}
__device__ __forceinline__ float sp_sum4(float s, const float (&v)[4]) { return s + ((v[0] + v[1]) + (v[2] + v[3])); }
__device__ __forceinline__ float sp_sq(float q, float x, float mean) { const float d = x - mean; return fmaf(d, d, q); }
__device__ __forceinline__ float sp_mean_of(float sum, int n) { return sum / n; }
__device__ __forceinline__ float sp_rstd_of(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// LDS carve shared by the tile kernels: w0s [hid*9] | b0s [hid] | s tile (TH+4)(TW+4), each rounded to 4 floats
__device__ __forceinline__ int sp_r4(int n) { return (n + 3) & ~3; }
struct SpTile { int b, y0, x0; };
__device__ __forceinline__ SpTile sp_tile(const SpadeArgs& A, int t) {
  const int b = t / A.tiles, tt = t - b * A.tiles;
  const int ty = tt / A.tiles_x, tx = tt - ty * A.tiles_x;
  return SpTile{b, ty * A.TH, tx * A.TW};
}
__device__ __forceinline__ void sp_stage_w0(const SpadeArgs& A, float* w0s) {
  for (int i = threadIdx.x; i < A.hid * 10; i += kBlock) w0s[i] = i < A.hid * 9 ? A.w0[i] : A.b0[i - A.hid * 9];
}
// s with a 2-pixel halo; 0 outside the image (the first convolution's zero padding)
__device__ __forceinline__ void sp_stage_s(const SpadeArgs& A, const SpTile& t, float* ss) {
  const int SW = A.TW + 4, n = (A.TH + 4) * SW;
  const float* m = A.mask + static_cast<size_t>(t.b) * A.HW;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const int r = i / SW, c = i - r * SW;
    const int yy = t.y0 + r - 2, xx = t.x0 + c - 2;
    float v = 0.f;
    if (yy >= 0 && yy < A.H && xx >= 0 && xx < A.W) {
      v = m[yy * A.W + xx];
      if (A.use_sigmoid) v = sigmoidf_(v);
    }
    ss[i] = v;
  }
}
// h with a 1-pixel halo, [halo pixel][HS]; 0 outside the image (the second convolutions' zero padding)
__device__ __forceinline__ void sp_form_h(const SpadeArgs& A, const SpTile& t, const float* w0s, const float* ss, float* hs, int HS) {
  const int SW = A.TW + 4, PW = A.TW + 2, n = (A.TH + 2) * PW * A.hid;
  const float* b0s = w0s + A.hid * 9;
  for (int i = threadIdx.x; i < n; i += kBlock) {
    const int ph = i / A.hid, j = i - ph * A.hid;
    const int r = ph / PW, c = ph - r * PW;
    const int yy = t.y0 + r - 1, xx = t.x0 + c - 1;
    float v = 0.f;
    if (yy >= 0 && yy < A.H && xx >= 0 && xx < A.W) {
      v = b0s[j];
#pragma unroll
      for (int k = 0; k < 9; ++k) v = fmaf(w0s[j * 9 + k], ss[(r + k / 3) * SW + c + k % 3], v);
      v = relu_nan(v);
    }
    hs[ph * HS + j] = v;
  }
}

// batch norm in training, the end of a channel: q = the channel's sum of centred squares over its n = B * HW values
__device__ __forceinline__ void sp_bn_finish(const SpadeArgs& A, int c, float mean, float q, float n) {
  const float var = q / n, rstd = sp_rstd_of(var, A.eps);
  for (int b = 0; b < A.B; ++b) { A.mean[b * A.C + c] = mean; A.rstd[b * A.C + c] = rstd; }
  A.rmean[c] = (1.f - A.momentum) * A.rmean[c] + A.momentum * mean;
  A.rvar[c] = (1.f - A.momentum) * A.rvar[c] + A.momentum * (q / (n - 1.f));
  if (c == 0 && A.nbt) *A.nbt += 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// statistics: mode 0 = per (b,c) plane (one wave each), 1 = batch norm in training (one workgroup per channel, running update),
// 2 = batch norm in eval (from the running statistics).  Two passes (mean, then the centred squares): no cancellation.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spade_stats(const Group<SpadeArgs> G) {
  __shared__ float red[8];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* x = static_cast<const T*>(A.x);
  const int HW = A.HW;
  if (!A.bn) {
    const int plane = local * 4 + wave;
    if (plane >= A.B * A.C) return;
    const T* p = x + static_cast<size_t>(plane) * HW;
    float s = 0.f;
    if ((HW & 3) == 0) {
      for (int i = lane * 4; i < HW; i += 256) { float v[4]; load_vec<T, 4>(p + i, v); s = sp_sum4(s, v); }
    } else {
      for (int i = lane; i < HW; i += 64) s += to_f32<T>(p[i]);
    }
    const float mean = sp_mean_of(wave_group_sum(s, 64), HW);
    float q = 0.f;
    if ((HW & 3) == 0) {
      for (int i = lane * 4; i < HW; i += 256) {
        float v[4]; load_vec<T, 4>(p + i, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) q = sp_sq(q, v[e], mean);
      }
    } else {
      for (int i = lane; i < HW; i += 64) q = sp_sq(q, to_f32<T>(p[i]), mean);
    }
    const float var = sp_mean_of(wave_group_sum(q, 64), HW);
    if (lane == 0) { A.mean[plane] = mean; A.rstd[plane] = sp_rstd_of(var, A.eps); }
  } else if (A.train) {
    const int c = local;
    const float n = static_cast<float>(A.B) * HW;
    float s = 0.f;
    for (int b = 0; b < A.B; ++b) {
      const T* p = x + (static_cast<size_t>(b) * A.C + c) * HW;
      for (int i = tid; i < HW; i += kBlock) s += to_f32<T>(p[i]);
    }
    s = block_sum(s, tid, red);
    __shared__ float mean_s;
    if (tid == 0) mean_s = s / n;
    __syncthreads();
    const float mean = mean_s;
    float q = 0.f;
    for (int b = 0; b < A.B; ++b) {
      const T* p = x + (static_cast<size_t>(b) * A.C + c) * HW;
      for (int i = tid; i < HW; i += kBlock) q = sp_sq(q, to_f32<T>(p[i]), mean);
    }
    q = block_sum(q, tid, red);
    if (tid == 0) sp_bn_finish(A, c, mean, q, n);
  } else {
    const int i = local * kBlock + tid;
    if (i >= A.B * A.C) return;
    const int c = i % A.C;
    A.mean[i] = A.rmean[c];
    A.rstd[i] = sp_rstd_of(A.rvar[c], A.eps);
  }
}

// wpack[w][t][c][j] = W_w[c][j][t], wpackT[w][t][j][c] likewise (w = 0: gamma, 1: beta)
__global__ __launch_bounds__(kBlock) void k_spade_pack(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int n = A.C * A.hid * 9;
  const int i = local * kBlock + threadIdx.x;
  if (i >= 2 * n) return;
  const int w = i / n, r = i - w * n;
  const int c = r / (A.hid * 9), jt = r - c * A.hid * 9, j = jt / 9, t = jt - j * 9;
  const float v = (w ? A.wb : A.wg)[r];
  A.wpack[((static_cast<size_t>(w) * 9 + t) * A.C + c) * A.hid + j] = v;
  A.wpackT[((static_cast<size_t>(w) * 9 + t) * A.hid + j) * A.C + c] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// forward: workgroup = (tile, channel block); wave w runs the 16-channel M tiles w, w + 4, ... of the block, gamma and beta of the same
// channels side by side (8 N tiles x 2 x 4 accumulator registers).  LDS: w0s | s | h [halo pixel][hid + 4].
// ---------------------------------------------------------------------------------------------------------------------------
// NHWC (here and in k_spade_ew / dw / dh): x / y / gy / gx and the saved gamma are (B,H,W,C).  Only the global accesses differ: the LDS
// images, the MFMA order and every sum after them are the NCHW ones.  The reductions of a channels-last level are in spade_nhwc.cuh.
template <typename T, bool SAVE, bool NHWC>
__global__ __launch_bounds__(kBlock) void k_spade_fwd(const Group<SpadeArgs> G) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ln = lane & 15;
  const int cb = local % A.ncb;
  const SpTile t = sp_tile(A, local / A.ncb);
  const int hid = A.hid, HS = hid + 4, PW = A.TW + 2;
  float* w0s = smem;
  float* ss = w0s + sp_r4(hid * 10);
  float* hs = ss + sp_r4((A.TH + 4) * (A.TW + 4));
  sp_stage_w0(A, w0s);
  sp_stage_s(A, t, ss);
  __syncthreads();
  sp_form_h(A, t, w0s, ss, hs, HS);
  __syncthreads();
  int poff[kSpNT];                                         // LDS offset of the lane's pixel of every N tile (tap 0,0)
#pragma unroll
  for (int nt = 0; nt < kSpNT; ++nt) { const int p = nt * 16 + ln; poff[nt] = ((p >> A.ltw) * PW + (p & (A.TW - 1))) * HS + 4 * g; }
  const T* x = static_cast<const T*>(A.x);
  T* y = static_cast<T*>(A.y);
  T* gsave = static_cast<T*>(A.gamma);
  const size_t wstride = static_cast<size_t>(9) * A.C * hid;
  for (int mt = wave; mt * 16 < A.cblk; mt += 4) {
    const int c0 = cb * A.cblk + mt * 16;
    if (c0 >= A.C) break;
    sp_v4f32 ag[kSpNT], ab[kSpNT];
#pragma unroll
    for (int nt = 0; nt < kSpNT; ++nt) { ag[nt] = sp_v4f32{0.f, 0.f, 0.f, 0.f}; ab[nt] = sp_v4f32{0.f, 0.f, 0.f, 0.f}; }
    for (int tap = 0; tap < 9; ++tap) {
      const int toff = ((tap / 3) * PW + tap % 3) * HS;
      const float* wa = A.wpack + (static_cast<size_t>(tap) * A.C + c0 + ln) * hid + 4 * g;
      for (int kk = 0; kk < hid; kk += 16) {
        float fa[4], fb[4];
        ld4(wa + kk, fa);
        ld4(wa + wstride + kk, fb);
#pragma unroll
        for (int nt = 0; nt < kSpNT; ++nt) {
          float hv[4];
          ld4(hs + poff[nt] + toff + kk, hv);
          ag[nt] = SpMma<T>::mma(fa, hv, ag[nt]);
          ab[nt] = SpMma<T>::mma(fb, hv, ab[nt]);
        }
      }
    }
    if constexpr (NHWC) {
      // the lane's four accumulator registers are four consecutive channels of one pixel: one vector access per tensor
      const int cq = c0 + 4 * g;
      const size_t plane = static_cast<size_t>(t.b) * A.C + cq;
      float mean[4], rstd[4], bgv[4], bbv[4];
      ld4(A.mean + plane, mean);
      ld4(A.rstd + plane, rstd);
#pragma unroll
      for (int v = 0; v < 4; ++v) { bgv[v] = A.bg[cq + v]; bbv[v] = A.bb[cq + v]; }   // (parameters: no alignment is asked of them)
#pragma unroll
      for (int nt = 0; nt < kSpNT; ++nt) {
        const int p = nt * 16 + ln;
        const int yy = t.y0 + (p >> A.ltw), xx = t.x0 + (p & (A.TW - 1));
        if (yy < A.H && xx < A.W) {
          const size_t at = (static_cast<size_t>(t.b) * A.HW + static_cast<size_t>(yy) * A.W + xx) * A.C + cq;
          float xv[4], yv[4], gm[4];
          load_vec<T, 4>(x + at, xv);
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            gm[v] = ag[nt][v] + bgv[v];
            yv[v] = sp_film(gm[v], sp_xhat(xv[v], mean[v], rstd[v]), ab[nt][v] + bbv[v]);
          }
          store_vec<T, 4>(y + at, yv);
          if constexpr (SAVE) store_vec<T, 4>(gsave + at, gm);
        }
      }
    } else {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int c = c0 + 4 * g + v;
        const size_t plane = static_cast<size_t>(t.b) * A.C + c;
        const float mean = A.mean[plane], rstd = A.rstd[plane], bgv = A.bg[c], bbv = A.bb[c];
#pragma unroll
        for (int nt = 0; nt < kSpNT; ++nt) {
          const int p = nt * 16 + ln;
          const int yy = t.y0 + (p >> A.ltw), xx = t.x0 + (p & (A.TW - 1));
          if (yy < A.H && xx < A.W) {
            const size_t at = plane * A.HW + static_cast<size_t>(yy) * A.W + xx;
            const float gm = ag[nt][v] + bgv;
            y[at] = from_f32<T>(sp_film(gm, sp_xhat(to_f32<T>(x[at]), mean, rstd), ab[nt][v] + bbv));
            if constexpr (SAVE) gsave[at] = from_f32<T>(gm);
          }
        }
      }
    }
  }
}

// element-wise passes.  MODE 0: y = xhat (forward without a mask).  MODE 1: gx = rstd * (g - m1 - xhat * m2), g = gy * gamma | gy.
template <typename T, int MODE, bool NHWC>
__global__ __launch_bounds__(kBlock) void k_spade_ew(const Group<SpadeArgs> G) {
  int local;
  const int l = find_level(G, blockIdx.x, local);
  const SpadeArgs& A = G.lv[l];
  const int nblk = G.start[l + 1] - G.start[l];
  const T* x = static_cast<const T*>(A.x);
  const T* gy = static_cast<const T*>(A.gy);
  const T* gam = static_cast<const T*>(A.gamma);
  T* out = static_cast<T*>(MODE == 0 ? A.y : A.gx);
  const size_t n = static_cast<size_t>(A.B) * A.C * A.HW;
  if constexpr (NHWC) {
    constexpr int V = 16 / sizeof(T);                        // channels per lane: one 16-byte access per tensor
    const size_t per = static_cast<size_t>(A.HW) * A.C;
    for (size_t iv = static_cast<size_t>(local) * kBlock + threadIdx.x; iv * V < n; iv += static_cast<size_t>(nblk) * kBlock) {
      const size_t i = iv * V;
      const size_t plane = (i / per) * A.C + i % A.C;
      float xv[V], mean[V], rstd[V];
      Pack<T, V> ov;
      load_vec<T, V>(x + i, xv);
      ldn<V>(A.mean + plane, mean);
      ldn<V>(A.rstd + plane, rstd);
      if constexpr (MODE == 0) {
#pragma unroll
        for (int e = 0; e < V; ++e) ov.v[e] = sp_product_to<T>(xv[e] - mean[e], rstd[e]);
      } else {
        float gv[V], st[2 * V];
        load_vec<T, V>(gy + i, gv);
        ldn<2 * V>(A.stat + 2 * plane, st);
        if (A.has_mask) {
          float gm[V];
          load_vec<T, V>(gam + i, gm);
#pragma unroll
          for (int e = 0; e < V; ++e) gv[e] *= gm[e];
        }
#pragma unroll
        for (int e = 0; e < V; ++e)
          ov.v[e] = sp_product_to<T>(rstd[e], sp_gx_inner(gv[e], st[2 * e], sp_xhat(xv[e], mean[e], rstd[e]), st[2 * e + 1]));
      }
      *reinterpret_cast<Pack<T, V>*>(out + i) = ov;
    }
  } else {
    for (size_t i = static_cast<size_t>(local) * kBlock + threadIdx.x; i < n; i += static_cast<size_t>(nblk) * kBlock) {
      const size_t plane = i / A.HW;
      if constexpr (MODE == 0) {
        out[i] = sp_product_to<T>(to_f32<T>(x[i]) - A.mean[plane], A.rstd[plane]);
      } else {
        const float xh = sp_xhat(to_f32<T>(x[i]), A.mean[plane], A.rstd[plane]);
        float gv = to_f32<T>(gy[i]);
        if (A.has_mask) gv *= to_f32<T>(gam[i]);
        out[i] = sp_product_to<T>(A.rstd[plane], sp_gx_inner(gv, A.stat[2 * plane], xh, A.stat[2 * plane + 1]));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward (i): per-plane sums, one wave per (b,c); then one thread per channel folds the samples in order
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_spade_bwd_reduce(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int lane = threadIdx.x & 63, plane = local * 4 + (threadIdx.x >> 6);
  if (plane >= A.B * A.C) return;
  const size_t base = static_cast<size_t>(plane) * A.HW;
  const T* x = static_cast<const T*>(A.x) + base;
  const T* gy = static_cast<const T*>(A.gy) + base;
  const T* gam = static_cast<const T*>(A.gamma) + base;
  const float mean = A.mean[plane], rstd = A.rstd[plane];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < A.HW; i += 64) {
    const float gyv = to_f32<T>(gy[i]), xh = sp_xhat(to_f32<T>(x[i]), mean, rstd);
    const float gv = A.has_mask ? gyv * to_f32<T>(gam[i]) : gyv;
    sp_red_terms(s, gyv, xh, gv);
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_group_sum(s[k], 64);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) A.red[4 * static_cast<size_t>(plane) + k] = s[k];
  }
}
__global__ __launch_bounds__(kBlock) void k_spade_bwd_fin(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int c = local * kBlock + threadIdx.x;
  if (c >= A.C) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int b = 0; b < A.B; ++b) {
    const float* r = A.red + 4 * (static_cast<size_t>(b) * A.C + c);
    s0 += r[0]; s1 += r[1]; s2 += r[2]; s3 += r[3];
  }
  if (A.has_mask) { A.gbg[c] = s2; A.gbb[c] = s3; }
  for (int b = 0; b < A.B; ++b) {
    const size_t plane = static_cast<size_t>(b) * A.C + c;
    float m1, m2;
    if (!A.bn) { m1 = A.red[4 * plane] / A.HW; m2 = A.red[4 * plane + 1] / A.HW; }
    else if (A.train) { const float n = static_cast<float>(A.B) * A.HW; m1 = s0 / n; m2 = s1 / n; }
    else { m1 = 0.f; m2 = 0.f; }
    A.stat[2 * plane] = m1; A.stat[2 * plane + 1] = m2;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward (ii): dW as a split-K GEMM over pixels.  Workgroup = (16-channel M tile, pixel chunk); rows = g_gamma | g_beta of the channels,
// columns = the 9 * hid / 16 (tap, 16 hidden) N tiles dealt round-robin to the four waves, K = the 128 pixels of a tile in 8 steps.
// LDS: w0s | s | h [halo pixel][hid] | ga [16][kSpAStride] | gb [16][kSpAStride]
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kSpDwQ = 9;            // N tiles per wave at hid = 64
template <typename T, bool NHWC>
__global__ __launch_bounds__(kBlock) void k_spade_dw(const Group<SpadeArgs> G) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ln = lane & 15;
  const int mt = local % (A.C / 16), chunk = local / (A.C / 16), c0 = mt * 16;
  const int hid = A.hid, HS = hid, PW = A.TW + 2, ntn = 9 * (hid / 16);
  float* w0s = smem;
  float* ss = w0s + sp_r4(hid * 10);
  float* hs = ss + sp_r4((A.TH + 4) * (A.TW + 4));
  float* ga = hs + sp_r4((A.TH + 2) * PW * HS);
  float* gb = ga + 16 * kSpAStride;
  sp_stage_w0(A, w0s);
  sp_v4f32 ag[kSpDwQ], ab[kSpDwQ];
#pragma unroll
  for (int q = 0; q < kSpDwQ; ++q) { ag[q] = sp_v4f32{0.f, 0.f, 0.f, 0.f}; ab[q] = sp_v4f32{0.f, 0.f, 0.f, 0.f}; }
  const T* x = static_cast<const T*>(A.x);
  const T* gy = static_cast<const T*>(A.gy);
  const int t_end = min(A.B * A.tiles, (chunk + 1) * A.tpc);
  for (int ti = chunk * A.tpc; ti < t_end; ++ti) {
    const SpTile t = sp_tile(A, ti);
    __syncthreads();                                       // the previous tile's operands are no longer read
    sp_stage_s(A, t, ss);
    if constexpr (NHWC) {
      constexpr int V = 16 / sizeof(T), CV = 16 / V;         // the 16 channels of a pixel are contiguous: CV 16-byte accesses
      for (int e = tid; e < kSpPx * CV; e += kBlock) {
        const int p = e / CV, cq = (e - p * CV) * V;
        const int yy = t.y0 + (p >> A.ltw), xx = t.x0 + (p & (A.TW - 1));
        float xv[V] = {}, gv[V] = {}, mean[V] = {}, rstd[V] = {};
        const bool in = yy < A.H && xx < A.W;
        if (in) {
          const size_t plane = static_cast<size_t>(t.b) * A.C + c0 + cq;
          const size_t at = (static_cast<size_t>(t.b) * A.HW + static_cast<size_t>(yy) * A.W + xx) * A.C + c0 + cq;
          load_vec<T, V>(gy + at, gv);
          load_vec<T, V>(x + at, xv);
          ldn<V>(A.mean + plane, mean);
          ldn<V>(A.rstd + plane, rstd);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
          ga[(cq + i) * kSpAStride + p] = in ? sp_ggamma(gv[i], xv[i], mean[i], rstd[i]) : 0.f;
          gb[(cq + i) * kSpAStride + p] = in ? gv[i] : 0.f;
        }
      }
    } else {
      for (int e = tid; e < 16 * kSpPx; e += kBlock) {
        const int c = e >> 7, p = e & (kSpPx - 1);
        const int yy = t.y0 + (p >> A.ltw), xx = t.x0 + (p & (A.TW - 1));
        float va = 0.f, vb = 0.f;
        if (yy < A.H && xx < A.W) {
          const size_t plane = static_cast<size_t>(t.b) * A.C + c0 + c;
          const size_t at = plane * A.HW + static_cast<size_t>(yy) * A.W + xx;
          vb = to_f32<T>(gy[at]);
          va = sp_ggamma(vb, to_f32<T>(x[at]), A.mean[plane], A.rstd[plane]);
        }
        ga[c * kSpAStride + p] = va;
        gb[c * kSpAStride + p] = vb;
      }
    }
    __syncthreads();
    sp_form_h(A, t, w0s, ss, hs, HS);
    __syncthreads();
    for (int ks = 0; ks < kSpNT; ++ks) {
      float fa[4], fb[4];
      ld4(ga + ln * kSpAStride + ks * 16 + 4 * g, fa);
      ld4(gb + ln * kSpAStride + ks * 16 + 4 * g, fb);
      int po[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int p = ks * 16 + 4 * g + i; po[i] = ((p >> A.ltw) * PW + (p & (A.TW - 1))) * HS + ln; }
#pragma unroll
      for (int q = 0; q < kSpDwQ; ++q) {
        const int ni = wave + 4 * q;
        if (ni < ntn) {
          const int tap = ni % 9, jt = ni / 9;
          const int off = ((tap / 3) * PW + tap % 3) * HS + jt * 16;
          float hv[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) hv[i] = hs[po[i] + off];
          ag[q] = SpMma<T>::mma(fa, hv, ag[q]);
          ab[q] = SpMma<T>::mma(fb, hv, ab[q]);
        }
      }
    }
  }
  const size_t n = static_cast<size_t>(A.C) * hid * 9;
  float* out = A.dwpart + static_cast<size_t>(chunk) * 2 * n;
#pragma unroll
  for (int q = 0; q < kSpDwQ; ++q) {
    const int ni = wave + 4 * q;
    if (ni < ntn) {
      const int tap = ni % 9, j = (ni / 9) * 16 + ln;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const size_t at = (static_cast<size_t>(c0 + 4 * g + v) * hid + j) * 9 + tap;
        out[at] = ag[q][v];
        out[n + at] = ab[q][v];
      }
    }
  }
}
__global__ __launch_bounds__(kBlock) void k_spade_dw_fin(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const size_t n = static_cast<size_t>(A.C) * A.hid * 9;
  const size_t i = static_cast<size_t>(local) * kBlock + threadIdx.x;
  if (i >= 2 * n) return;
  float s = 0.f;
  for (int ch = 0; ch < A.nchunk; ++ch) s += A.dwpart[static_cast<size_t>(ch) * 2 * n + i];
  if (i < n) A.gwg[i] = s; else A.gwb[i - n] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// backward (iii): dh[j][q] = sum_{tap, c} wg[c][j][tap] g_gamma[c][q - off(tap)] + the same with wb, g_beta: an implicit transposed
// convolution, M = hid (wave w = M tile w), N = the tile's 128 pixels, K = 2 C * 9.  g_gamma / g_beta are staged kSpDhCC channels at a
// time with a 1-pixel halo as [halo pixel][2][CC + 4].  Epilogue: ReLU mask from the re-formed pre-activation, dpre to LDS [j][128 + 4]
// (over the staging area), then the 9 tap planes u[t][p] = sum_j w0[j][t] dpre[j][p] and the tile's dW0 / db0 partials.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool NHWC>
__global__ __launch_bounds__(kBlock) void k_spade_dh(const Group<SpadeArgs> G) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, ln = lane & 15;
  const SpTile t = sp_tile(A, local);
  const int hid = A.hid, PW = A.TW + 2, SW = A.TW + 4, NPH = (A.TH + 2) * PW;
  const int CC = min(A.C, kSpDhCC), GS = 2 * (CC + 4);
  float* w0s = smem;
  float* ss = w0s + sp_r4(hid * 10);
  float* gs = ss + sp_r4((A.TH + 4) * SW);
  sp_stage_w0(A, w0s);
  sp_stage_s(A, t, ss);
  const T* x = static_cast<const T*>(A.x);
  const T* gy = static_cast<const T*>(A.gy);
  const bool active = wave * 16 < hid;
  sp_v4f32 acc[kSpNT], part[kSpNT];                        // acc: the rounds finished so far; part: the current round (K <= 18 * kSpDhCC)
#pragma unroll
  for (int nt = 0; nt < kSpNT; ++nt) acc[nt] = sp_v4f32{0.f, 0.f, 0.f, 0.f};
  int poff[kSpNT];                                         // the lane's pixel of every N tile at halo offset (2,2): minus the tap's (dy,dx)
#pragma unroll
  for (int nt = 0; nt < kSpNT; ++nt) { const int p = nt * 16 + ln; poff[nt] = (((p >> A.ltw) + 2) * PW + (p & (A.TW - 1)) + 2) * GS + 4 * g; }
  const size_t wstride = static_cast<size_t>(9) * hid * A.C;
  for (int cc0 = 0; cc0 < A.C; cc0 += CC) {
    const int cn = min(CC, A.C - cc0);                     // the last round holds 16 channels when C % 32 == 16
    __syncthreads();
    if constexpr (NHWC) {
      constexpr int V = 16 / sizeof(T);                      // the round's cn channels of a halo pixel are contiguous: cn / V 16-byte accesses
      const int cv = cn / V;
      for (int e = tid; e < NPH * cv; e += kBlock) {
        const int ph = e / cv, cq = (e - ph * cv) * V;
        const int r = ph / PW, cx = ph - r * PW;
        const int yy = t.y0 + r - 1, xx = t.x0 + cx - 1;
        float xv[V] = {}, gv[V] = {}, mean[V] = {}, rstd[V] = {};
        const bool in = yy >= 0 && yy < A.H && xx >= 0 && xx < A.W;
        if (in) {
          const size_t plane = static_cast<size_t>(t.b) * A.C + cc0 + cq;
          const size_t at = (static_cast<size_t>(t.b) * A.HW + static_cast<size_t>(yy) * A.W + xx) * A.C + cc0 + cq;
          load_vec<T, V>(gy + at, gv);
          load_vec<T, V>(x + at, xv);
          ldn<V>(A.mean + plane, mean);
          ldn<V>(A.rstd + plane, rstd);
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
          gs[ph * GS + cq + i] = in ? sp_ggamma(gv[i], xv[i], mean[i], rstd[i]) : 0.f;
          gs[ph * GS + CC + 4 + cq + i] = in ? gv[i] : 0.f;
        }
      }
    } else {
      for (int e = tid; e < cn * NPH; e += kBlock) {
        const int c = e / NPH, ph = e - c * NPH;
        const int r = ph / PW, cx = ph - r * PW;
        const int yy = t.y0 + r - 1, xx = t.x0 + cx - 1;
        float va = 0.f, vb = 0.f;
        if (yy >= 0 && yy < A.H && xx >= 0 && xx < A.W) {
          const size_t plane = static_cast<size_t>(t.b) * A.C + cc0 + c;
          const size_t at = plane * A.HW + static_cast<size_t>(yy) * A.W + xx;
          vb = to_f32<T>(gy[at]);
          va = sp_ggamma(vb, to_f32<T>(x[at]), A.mean[plane], A.rstd[plane]);
        }
        gs[ph * GS + c] = va;
        gs[ph * GS + CC + 4 + c] = vb;
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int nt = 0; nt < kSpNT; ++nt) part[nt] = sp_v4f32{0.f, 0.f, 0.f, 0.f};
      for (int tap = 0; tap < 9; ++tap) {
        const int toff = ((tap / 3) * PW + tap % 3) * GS;
        const float* wa = A.wpackT + (static_cast<size_t>(tap) * hid + wave * 16 + ln) * A.C + cc0 + 4 * g;
        for (int kk = 0; kk < cn; kk += 16) {
          float fa[4], fb[4];
          ld4(wa + kk, fa);
          ld4(wa + wstride + kk, fb);
#pragma unroll
          for (int nt = 0; nt < kSpNT; ++nt) {
            float va[4], vb[4];
            ld4(gs + poff[nt] - toff + kk, va);
            ld4(gs + poff[nt] - toff + CC + 4 + kk, vb);
            part[nt] = SpMma<T>::mma(fa, va, part[nt]);
            part[nt] = SpMma<T>::mma(fb, vb, part[nt]);
          }
        }
      }
      // K = 18 C runs to 18432 terms of mixed sign.  One running fp32 sum over all of them missed the element-wise bar on dL/dmask at
      // C = 1024 by 1.14x; rounds summed from zero and then added stay 5x inside it.  (C <= kSpDhCC: the one round is added to zero.)
#pragma unroll
      for (int nt = 0; nt < kSpNT; ++nt) acc[nt] += part[nt];
    }
  }
  __syncthreads();
  float* dp = gs;                                          // [hid][kSpAStride]
  if (active) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = wave * 16 + 4 * g + v;
#pragma unroll
      for (int nt = 0; nt < kSpNT; ++nt) {
        const int p = nt * 16 + ln;
        const int r = p >> A.ltw, cx = p & (A.TW - 1);
        float pre = w0s[hid * 9 + j];
#pragma unroll
        for (int k = 0; k < 9; ++k) pre = fmaf(w0s[j * 9 + k], ss[(r + 1 + k / 3) * SW + cx + 1 + k % 3], pre);
        const bool in = t.y0 + r < A.H && t.x0 + cx < A.W;
        dp[j * kSpAStride + p] = (in && relu_passes(pre)) ? acc[nt][v] : 0.f;
      }
    }
  }
  __syncthreads();
  float* u = A.u + static_cast<size_t>(t.b) * 9 * A.HW;
  for (int e = tid; e < 9 * kSpPx; e += kBlock) {
    const int tap = e >> 7, p = e & (kSpPx - 1);
    const int yy = t.y0 + (p >> A.ltw), xx = t.x0 + (p & (A.TW - 1));
    if (yy < A.H && xx < A.W) {
      float s = 0.f;
      for (int j = 0; j < hid; ++j) s = fmaf(w0s[j * 9 + tap], dp[j * kSpAStride + p], s);
      u[static_cast<size_t>(tap) * A.HW + yy * A.W + xx] = s;
    }
  }
  float* wp = A.w0part + static_cast<size_t>(local) * hid * 10;
  for (int e = tid; e < hid * 10; e += kBlock) {
    const int j = e / 10, k = e - j * 10;
    float s = 0.f;
    if (k < 9) {
      for (int p = 0; p < kSpPx; ++p) s = fmaf(dp[j * kSpAStride + p], ss[((p >> A.ltw) + 1 + k / 3) * SW + (p & (A.TW - 1)) + 1 + k % 3], s);
    } else {
      for (int p = 0; p < kSpPx; ++p) s += dp[j * kSpAStride + p];
    }
    wp[e] = s;
  }
}
// ds[q] = sum_t u[t][q - off(t)], gmask = ds * s (1 - s) | ds
__global__ __launch_bounds__(kBlock) void k_spade_gmask(const Group<SpadeArgs> G) {
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int i = local * kBlock + threadIdx.x;
  if (i >= A.B * A.HW) return;
  const int b = i / A.HW, q = i - b * A.HW, yy = q / A.W, xx = q - yy * A.W;
  const float* u = A.u + static_cast<size_t>(b) * 9 * A.HW;
  float ds = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int y2 = yy - (k / 3 - 1), x2 = xx - (k % 3 - 1);
    if (y2 >= 0 && y2 < A.H && x2 >= 0 && x2 < A.W) ds += u[static_cast<size_t>(k) * A.HW + y2 * A.W + x2];
  }
  if (A.use_sigmoid) { const float s = sigmoidf_(A.mask[i]); ds *= s * (1.f - s); }
  A.gmask[i] = ds;
}
// dW0 / db0: one workgroup per output sums the tiles' partials (fixed order)
__global__ __launch_bounds__(kBlock) void k_spade_w0_fin(const Group<SpadeArgs> G) {
  __shared__ float red[8];
  int local;
  const SpadeArgs& A = G.lv[find_level(G, blockIdx.x, local)];
  const int nt = A.B * A.tiles;
  float s = 0.f;
  for (int i = threadIdx.x; i < nt; i += kBlock) s += A.w0part[static_cast<size_t>(i) * A.hid * 10 + local];
  s = block_sum(s, threadIdx.x, red);
  if (threadIdx.x == 0) {
    const int j = local / 10, k = local - j * 10;
    if (k < 9) A.gw0[j * 9 + k] = s; else A.gb0[j] = s;
  }
}

}  // namespace mgacbam
