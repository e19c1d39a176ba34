// Channels-last (NHWC) forms of the three MGAMaskHead products that touch x or gx (MGAHEAD_LAYOUT_NHWC levels).  Everything else of
// the head is layout-free and shared with the NCHW path: z stays (B,hid,HW) fp32 in the ctx, g_a (B,hid,HW) in the scratch, so
// k_head_stats, k_head_out, k_head_bwd_act, k_head_bwd_fin and k_head_bwd_gwf run unchanged (head.cuh).
//
//   forward   k_head_gemm_nhwc  x (1 read)        -> z + per-workgroup (sum, M2) partials in the ctx `part` layout k_head_stats folds
//   backward  k_head_gx_nhwc    g_a, z (+ gx old)  -> gx[b,px,:] (+)= W1^T g_z[b,:,px]   (g_z formed on the fly, as k_head_gemm<GX>)
//             k_head_gw_nhwc    g_a, z, x (1 read) -> dW1 partials sum_px g_z[j,px] x[px,c] in the `gwpart` layout k_head_bwd_gwf sums
//
// In NHWC the 1x1 conv contracts over the CONTIGUOUS axis: a lane's four consecutive channels of one pixel are one 16-byte (fp32) /
// 8-byte (fp16 / bf16) load, and they are the four K values a lane supplies to the MFMA -- K runs in groups of 16 channels, lane (lk, ln)
// of step 4q + r taking channel 16q + 4lk + r (the `wperm` order of k_head_gemm's forward, now on both operands).  fp32:
// v_mfma_f32_16x16x4_f32, four per group; fp16 / bf16: one v_mfma_f32_16x16x16 per group (HalfMma, operands rounded as the NCHW forms
// round them).  CV = 4 when C % 4 == 0 (vector loads and stores along C), else 1 (per-element, bounds-checked: any C >= 1).
// Pixel tiles never depend on B or the other levels of the call; no float atomics: every cross-workgroup sum is a partial plus a
// fixed-order reader, so results are bitwise reproducible and, in eval mode, a sample's logits and gx do not depend on its batch.
#pragma once
#include "head.cuh"

namespace mgacbam {

constexpr int kHeadNhwcNP = 4;       // 16-pixel MFMA sub-tiles per wave: 64 pixels (the forward and gx waves)
constexpr int kHeadNhwcPx = 16 * kHeadNhwcNP;

// a lane's 4 consecutive channels c0..c0+3 of one row (zeros past C)
template <typename T, int CV>
__device__ __forceinline__ void load_c4(const T* p, int c0, int C, float (&v)[4]) {
  if constexpr (CV == 4) {
    if (c0 < C) load_vec<T, 4>(p + c0, v);
    else { v[0] = v[1] = v[2] = v[3] = 0.f; }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = c0 + r < C ? to_f32<T>(p[c0 + r]) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_head_gemm_nhwc:  z[b,j,px] = sum_c W1[j,c] x[b,px,c]   (M = hid, N = pixels, K = C)
//   Workgroup = 4 waves = MW (along M, MTW tiles each) x PW (along pixels, 64 each); tile = PW * 64 consecutive pixels of one sample.
//   A = W1 (lane: output row ln, its 4 channels of the group as one 16-byte load), B = x (lane: pixel r*16 + ln of sub-tile r, the same
//   4 channels), D: lane (lk, ln), register v = output 4lk + v, pixel r*16 + ln.  Batch statistics exactly as k_head_gemm<FWD>: per wave
//   (sum, M2 about its own mean) over 16 lanes, the PW waves combined pairwise (Chan) into one row of `part` per workgroup.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int CV, int MTW>
__device__ __forceinline__ void head_gemm_nhwc_body(const HeadArgs& A, const int wg, float* smem) {
  const HeadGeo& g = A.g;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, ln = lane & 15;
  constexpr int NP = kHeadNhwcNP;
  const int MT = g.hidp >> 4;
  const int MW = min(4, (MT + MTW - 1) / MTW);
  const int MWp = MW == 3 ? 4 : MW;
  const int PW = 4 / MWp;
  const int mw = wave % MWp, pw = wave / MWp;
  const int b = wg / A.tiles_per_sample, tile = wg - b * A.tiles_per_sample;
  const int wpx0 = tile * A.tile_px + pw * kHeadNhwcPx;        // first pixel of this wave
  float* s_sum = smem;                                          // [PW][2][hidp]
  const T* xb = static_cast<const T*>(A.x) + static_cast<size_t>(b) * g.HW * g.C;
  bool pok[NP];
  const T* xr[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int px = wpx0 + p * 16 + ln;
    pok[p] = px < g.HW;
    xr[p] = xb + static_cast<size_t>(pok[p] ? px : 0) * g.C;
  }
  const int n_wave = max(0, min(kHeadNhwcPx, g.HW - wpx0));
  const int nq = (g.C + 15) >> 4;                               // K groups of 16 channels
  const int mblk = MTW * MWp;
  for (int mt0 = 0; mt0 < MT; mt0 += mblk) {
    const int mtn = min(mblk, MT - mt0);
    v4f32 acc[MTW][NP];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[t][p] = v4f32{0.f, 0.f, 0.f, 0.f};
    constexpr int GQ = 2;                                       // groups per batch: both operands of a batch requested before its first MFMA
    for (int q0 = 0; q0 < nq; q0 += GQ) {
      float bv[GQ][NP][4], aw[GQ][MTW][4];
#pragma unroll
      for (int gi = 0; gi < GQ; ++gi) {
        const int c0 = (q0 + gi) * 16 + 4 * lk;                 // this lane's 4 channels of the group
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (pok[p]) load_c4<T, CV>(xr[p], c0, g.C, bv[gi][p]);
          else { bv[gi][p][0] = bv[gi][p][1] = bv[gi][p][2] = bv[gi][p][3] = 0.f; }
        }
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
          const int mt = mw * MTW + t;
          const int out = (mt0 + mt) * 16 + ln;
          if (mt < mtn && out < g.hid) load_c4<float, CV>(A.p.w1 + static_cast<size_t>(out) * g.C, c0, g.C, aw[gi][t]);
          else { aw[gi][t][0] = aw[gi][t][1] = aw[gi][t][2] = aw[gi][t][3] = 0.f; }
        }
      }
#pragma unroll
      for (int gi = 0; gi < GQ; ++gi) {
        if (q0 + gi < nq) {                                     // uniform
#pragma unroll
          for (int t = 0; t < MTW; ++t) {
            if (mw * MTW + t < mtn) {                           // uniform per wave
#pragma unroll
              for (int p = 0; p < NP; ++p) {
                if constexpr (HalfMma<T>::on) {
                  acc[t][p] = HalfMma<T>::mma(aw[gi][t][0], aw[gi][t][1], aw[gi][t][2], aw[gi][t][3],
                                              bv[gi][p][0], bv[gi][p][1], bv[gi][p][2], bv[gi][p][3], acc[t][p]);
                } else {
#pragma unroll
                  for (int r = 0; r < 4; ++r) acc[t][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[gi][t][r], bv[gi][p][r], acc[t][p], 0, 0, 0);
                }
              }
            }
          }
        }
      }
    }
    // ---- epilogue: z (16 lanes = 64 contiguous bytes of one row per sub-tile), tile statistics --------------------------------
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
      const int mt = mw * MTW + t;
      if (mt < mtn) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int out = (mt0 + mt) * 16 + lk * 4 + v;
          float s1 = 0.f;
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            s1 += acc[t][p][v];                                  // pixels past H*W were loaded as zeros: they add nothing
            if (out < g.hid && pok[p]) A.c.z[(static_cast<size_t>(b) * g.hid + out) * g.HW + wpx0 + p * 16 + ln] = acc[t][p][v];
          }
          if (g.training) {
            s1 = wave_group_sum(s1, 16);
            const float mw_ = n_wave > 0 ? s1 / static_cast<float>(n_wave) : 0.f;
            float m2 = 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
              if (pok[p]) { const float d = acc[t][p][v] - mw_; m2 += d * d; }
            }
            m2 = wave_group_sum(m2, 16);
            if (ln == 0) { s_sum[(pw * 2 + 0) * g.hidp + out] = s1; s_sum[(pw * 2 + 1) * g.hidp + out] = m2; }
          }
        }
      }
    }
  }
  if (g.training) {                                             // this tile's (sum, M2 about the tile mean) per output channel
    __syncthreads();
    float* part = A.c.part + static_cast<size_t>(wg) * 2 * g.hidp;
    for (int i = tid; i < g.hidp; i += kBlock) {
      float n = 0.f, S = 0.f, M2 = 0.f;
      for (int w = 0; w < PW; ++w) {                            // the pixel waves' partials, combined pairwise (Chan et al.), fixed order
        const float nb = static_cast<float>(max(0, min(kHeadNhwcPx, g.HW - (tile * A.tile_px + w * kHeadNhwcPx))));
        if (nb > 0.f) {
          const float Sb = s_sum[(w * 2 + 0) * g.hidp + i], Mb = s_sum[(w * 2 + 1) * g.hidp + i];
          if (n == 0.f) { S = Sb; M2 = Mb; n = nb; }
          else { const float d = Sb / nb - S / n; M2 += Mb + d * d * (n * nb / (n + nb)); S += Sb; n += nb; }
        }
      }
      part[i] = S; part[g.hidp + i] = M2;
    }
  }
}

template <typename T, int CV, int MTW>
__global__ __launch_bounds__(kBlock) void k_head_gemm_nhwc(const Group<HeadArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  head_gemm_nhwc_body<T, CV, MTW>(G.lv[l], local, smem);
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_head_gx_nhwc:  gx[b,px,c] (+)= sum_j W1[j,c] g_z[b,j,px]   (M = C, N = pixels, K = hid)
//   A = W1^T (lane: channel ln of the tile, its 4 hidden channels of the group: gathers of W1 rows, <= 64 KB, cache hits),
//   B = g_z (lane: pixel r*16 + ln, the same 4 hidden channels; g_a and z rows: 64 contiguous bytes per 16 lanes),
//   D: lane (lk, ln), register v = channel 4lk + v of pixel r*16 + ln -- a lane owns 4 CONSECUTIVE channels of a pixel: one 16-byte
//   (fp32) / 8-byte (fp16 / bf16) store along C, and one load of the old values when accumulating.
//   Workgroup = 4 waves = MW (along C, 2 tiles each) x PW (along pixels, 64 each), M in blocks of 16 * 2 * MW channels.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int CV>
__device__ __forceinline__ void head_gx_nhwc_body(const HeadArgs& A, const int wg, float* smem) {
  const HeadGeo& g = A.g;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lk = lane >> 4, ln = lane & 15;
  constexpr int NP = kHeadNhwcNP, MTW = 2;
  const int MT = g.cp >> 4;
  const int MW = min(4, (MT + MTW - 1) / MTW);
  const int MWp = MW == 3 ? 4 : MW;
  const int mw = wave % MWp, pw = wave / MWp;
  const int b = wg / A.gx_tiles_per_sample, tile = wg - b * A.gx_tiles_per_sample;
  const int wpx0 = tile * A.gx_tile_px + pw * kHeadNhwcPx;
  float* s_kst = smem;                                          // [5][hidp]: per-hidden-channel constants of g_z
  for (int i = tid; i < 5 * g.hidp; i += kBlock) s_kst[i] = A.s.kst[i];
  __syncthreads();
  bool pok[NP];
  int pxo[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int px = wpx0 + p * 16 + ln;
    pok[p] = px < g.HW;
    pxo[p] = pok[p] ? px : 0;
  }
  const float* gab = A.s.ga + static_cast<size_t>(b) * g.hid * g.HW;
  const float* zb = A.c.z + static_cast<size_t>(b) * g.hid * g.HW;
  T* gxb = static_cast<T*>(A.gx) + static_cast<size_t>(b) * g.HW * g.C;
  const int nq = (g.hid + 15) >> 4;
  const int mblk = MTW * MWp;
  for (int mt0 = 0; mt0 < MT; mt0 += mblk) {
    const int mtn = min(mblk, MT - mt0);
    v4f32 acc[MTW][NP];
#pragma unroll
    for (int t = 0; t < MTW; ++t)
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[t][p] = v4f32{0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < nq; ++q) {
      const int j0 = q * 16 + 4 * lk;                           // this lane's 4 hidden channels of the group
      float bv[NP][4], zq[NP][4], aw[MTW][4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + r;
        const bool jok = j < g.hid;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          bv[p][r] = 0.f; zq[p][r] = 0.f;
          if (jok && pok[p]) { bv[p][r] = gab[static_cast<size_t>(j) * g.HW + pxo[p]]; zq[p][r] = zb[static_cast<size_t>(j) * g.HW + pxo[p]]; }
        }
#pragma unroll
        for (int t = 0; t < MTW; ++t) {
          const int mt = mw * MTW + t;
          const int c = (mt0 + mt) * 16 + ln;
          aw[t][r] = (jok && mt < mtn && c < g.C) ? A.p.w1[static_cast<size_t>(j) * g.C + c] : 0.f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {                             // g_z = k_j (g_a - gbeta_j/n - zhat gamma'_j/n), zhat = (z - mean) rstd
        const int j = j0 + r;                                   // (< hidp; padding channels have zero constants)
        const float kj = s_kst[j], mean = s_kst[g.hidp + j], rstd = s_kst[2 * g.hidp + j];
        const float gbn = s_kst[3 * g.hidp + j], ggn = s_kst[4 * g.hidp + j];
#pragma unroll
        for (int p = 0; p < NP; ++p) bv[p][r] = kj * (bv[p][r] - gbn - (zq[p][r] - mean) * rstd * ggn);
      }
#pragma unroll
      for (int t = 0; t < MTW; ++t) {
        if (mw * MTW + t < mtn) {                               // uniform per wave
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            if constexpr (HalfMma<T>::on) {
              acc[t][p] = HalfMma<T>::mma(aw[t][0], aw[t][1], aw[t][2], aw[t][3], bv[p][0], bv[p][1], bv[p][2], bv[p][3], acc[t][p]);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[t][p] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[t][r], bv[p][r], acc[t][p], 0, 0, 0);
            }
          }
        }
      }
    }
    // ---- epilogue: a lane's 4 consecutive channels of each of its pixels (accumulating: a tile's old values are all requested before
    //      its first store) ------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < MTW; ++t) {
      const int mt = mw * MTW + t;
      const int c0 = (mt0 + mt) * 16 + lk * 4;
      if (mt < mtn && c0 < g.C) {
        float ov[NP][4];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          ov[p][0] = ov[p][1] = ov[p][2] = ov[p][3] = 0.f;
          if (A.accum_gx && pok[p]) load_c4<T, CV>(gxb + static_cast<size_t>(pxo[p]) * g.C, c0, g.C, ov[p]);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
          if (!pok[p]) continue;
#pragma unroll
          for (int v = 0; v < 4; ++v) ov[p][v] += acc[t][p][v];
          T* gp = gxb + static_cast<size_t>(pxo[p]) * g.C + c0;
          if constexpr (CV == 4) {
            store_vec_stream<T, 4>(gp, ov[p]);
          } else {
#pragma unroll
            for (int v = 0; v < 4; ++v)
              if (c0 + v < g.C) gp[v] = from_f32<T>(ov[p][v]);
          }
        }
      }
    }
  }
}

template <typename T, int CV>
__global__ __launch_bounds__(kBlock) void k_head_gx_nhwc(const Group<HeadArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  head_gx_nhwc_body<T, CV>(G.lv[l], local, smem);
}

// ---------------------------------------------------------------------------------------------------------------------------
// k_head_gw_nhwc:  partials of dW1[j,c] = sum_{b,px} g_z[b,j,px] x[b,px,c]   (M = hid, N = C, K = pixels)
//   K is the STRIDED axis of x here, so both operands go through LDS, as in k_head_bwd_gw2: workgroup = (block of kHeadCB = 64
//   channels, one of nshare pixel shares); per chunk of kHeadGwPx = 64 consecutive pixels of one sample
//     x   [64 px][64 channels]  pixel-major, as it lies in memory: a wave-load = 4 pixels x 16 lanes x 16 B (256 contiguous bytes per
//                               pixel: 64 fp32 channels);
//     g_z [64 hidden][64 px]    from g_a, z rows (a wave-load = 256 contiguous bytes of one row), formed while storing;
//   the next chunk's global loads are in flight during this chunk's MFMAs; wave w owns channel tile w and up to 4 hidden tiles.
//   Hidden sizes above 64 run in passes of 64 hidden channels (x re-read per pass).  B operand reads: 4 x ds_read_b32 (4 pixels of one
//   channel; 64 distinct banks per instruction at the 68-float pitch), A operand reads: ds_read_b128.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, int CV>
__device__ __forceinline__ void head_gw_nhwc_body(const HeadArgs& A, const int wg, float* smem) {
  const HeadGeo& g = A.g;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int lr = lane & 15, lq = lane >> 4;
  const int cb = wg / A.nshare, share = wg - cb * A.nshare;
  const int c0 = cb * kHeadCB;
  const int nch = (g.HW + kHeadGwPx - 1) / kHeadGwPx;           // chunks per sample
  const int total = g.B * nch;
  float* s_kst = smem;                                          // [5][hidp]
  float* s_x = smem + 5 * g.hidp;                               // [64 px][pitch]
  float* s_g = s_x + kHeadGwPx * kHeadGwPitch;                  // [64 hidden][pitch]
  for (int i = tid; i < 5 * g.hidp; i += kBlock) s_kst[i] = A.s.kst[i];
  __syncthreads();
  float* outp = A.s.gwpart + static_cast<size_t>(wg) * g.hidp * kHeadCB;
  const T* xg = static_cast<const T*>(A.x);
  for (int hb = 0; hb < g.hidp; hb += 64) {
    const int MT = min(64, g.hidp - hb) >> 4;                   // hidden tiles of this pass (1..4)
    float xv[4][4], gav[16], zvv[16];
    // staging roles -- x: lane = (channel group lr of 4 channels, pixel 16w + 4i + lq); g_z: lane = (pixel `lane`, hidden rows w + 4i)
    auto issue = [&](const int ch) {
      const int b = ch / nch, px0 = (ch - b * nch) * kHeadGwPx;
      const bool live = ch < total;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int px = px0 + wave * 16 + i * 4 + lq;
        if (live && px < g.HW) load_c4<T, CV>(xg + (static_cast<size_t>(b) * g.HW + px) * g.C, c0 + 4 * lr, g.C, xv[i]);
        else { xv[i][0] = xv[i][1] = xv[i][2] = xv[i][3] = 0.f; }
      }
      const int px = px0 + lane;
      const bool pok = live && px < g.HW;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = hb + wave + 4 * i;
        gav[i] = 0.f; zvv[i] = 0.f;
        if (wave + 4 * i < MT * 16 && pok && j < g.hid) {
          const size_t o = (static_cast<size_t>(b) * g.hid + j) * g.HW + px;
          gav[i] = A.s.ga[o]; zvv[i] = A.c.z[o];
        }
      }
    };
    auto to_lds = [&]() {
#pragma unroll
      for (int i = 0; i < 4; ++i) store_vec<float, 4>(s_x + (wave * 16 + i * 4 + lq) * kHeadGwPitch + 4 * lr, xv[i]);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int jl = wave + 4 * i;
        if (jl < MT * 16) {                                     // uniform
          const int j = hb + jl;                                // (< hidp; padding rows have zero constants and load zeros)
          const float kj = s_kst[j], mean = s_kst[g.hidp + j], rstd = s_kst[2 * g.hidp + j], gbn = s_kst[3 * g.hidp + j], ggn = s_kst[4 * g.hidp + j];
          s_g[jl * kHeadGwPitch + lane] = kj * (gav[i] - gbn - (zvv[i] - mean) * rstd * ggn);
        }
      }
    };
    v4f32 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = v4f32{0.f, 0.f, 0.f, 0.f};
    int ch = share;
    issue(ch);
    for (; ch < total; ch += A.nshare) {                        // (uniform over the workgroup)
      __syncthreads();                                          // everyone is done reading the previous chunk
      to_lds();
      __syncthreads();
      issue(ch + A.nshare);                                     // in flight during the MFMAs below (a chunk past the end loads nothing)
#pragma unroll
      for (int sp = 0; sp < kHeadGwPx / 16; ++sp) {             // 16 pixels = 4 K steps
        float bq[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bq[r] = s_x[(sp * 16 + 4 * lq + r) * kHeadGwPitch + wave * 16 + lr];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          if (t < MT) {                                         // uniform
            float aq[4];
            load_vec<float, 4>(s_g + (t * 16 + lr) * kHeadGwPitch + sp * 16 + 4 * lq, aq);
            if constexpr (HalfMma<T>::on) {
              acc[t] = HalfMma<T>::mma(aq[0], aq[1], aq[2], aq[3], bq[0], bq[1], bq[2], bq[3], acc[t]);
            } else {
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(aq[r], bq[r], acc[t], 0, 0, 0);
            }
          }
        }
      }
    }
    // D layout: lane l, register v: row (hidden) 4*(l/16)+v, column (channel) l%16; wave w owns channel tile w
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (t < MT) {
#pragma unroll
        for (int v = 0; v < 4; ++v) outp[static_cast<size_t>(hb + t * 16 + lq * 4 + v) * kHeadCB + wave * 16 + lr] = acc[t][v];
      }
    }
    __syncthreads();                                            // the next pass re-stages s_g / s_x
  }
}

template <typename T, int CV>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void k_head_gw_nhwc(const Group<HeadArgs> G) {
  extern __shared__ __align__(16) float smem[];
  int local;
  const int l = find_level(G, blockIdx.x, local);
  head_gw_nhwc_body<T, CV>(G.lv[l], local, smem);
}

}  // namespace mgacbam
