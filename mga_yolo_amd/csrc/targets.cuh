// The multi-scale segmentation targets (include/mgatargets.h): block counts of a binary mask at every stride of a call, in one launch.
//   k_tgt_pool  : strides (8), (8,16), (8,16,32).  A wave owns a 64 x 64 pixel tile = 8 x 8 cells of 8 x 8 pixels, one cell per lane; the
//                 lane's six bits interleave the cell's column and row bits (x0 y0 x1 y1 x2 y2), so the four lanes of a quad are one
//                 16-cell and the sixteen lanes of a DPP row one 32-cell: the 16-count is two quad_perm adds of the 8-counts, the
//                 32-count a row_half_mirror and a row_mirror add more.  Every source element is read once -- eight 8-byte loads per
//                 lane (uint8) or sixteen 16-byte ones (fp32) where base and W allow it, element loads otherwise.  Integer counts:
//                 no order to keep, no atomics.
//   k_tgt_cells : any other stride list, one thread per destination cell of every level.
//   k_tgt_close3: MGATGT_CLOSE3 -- a 16 x 16 tile of a level with its 2-cell halo in LDS, dilated, then eroded.  A neighbour outside the
//                 level enters as the operation's neutral element (0 for the max, 1 for the min), i.e. it is ignored.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kTgtLevelsMax = 4;               // = MGATGT_MAX_LEVELS (api_targets.hip asserts it)
constexpr int kTgtTile = 64;                   // pixels per side of a wave's tile in k_tgt_pool
constexpr int kTgtCloseTile = 16;              // cells per side of a workgroup's tile in k_tgt_close3 (16 x 16 = kBlock threads)

struct TgtArgs {
  const void* src;                             // (B, H, W)
  float* dst[kTgtLevelsMax];                   // where the pooled level goes: the caller's dst, or its place in scratch before a closing
  int stride[kTgtLevelsMax], oh[kTgtLevelsMax], ow[kTgtLevelsMax];
  long long cell_start[kTgtLevelsMax + 1];     // k_tgt_cells: threads [cell_start[l], cell_start[l+1]) belong to level l
  int n, B, H, W;
  int tiles_y, tiles_x;                        // k_tgt_pool: wave tiles per sample
  int maxpool;                                 // 0: count / stride^2, 1: count > 0
};

struct TgtCloseArgs {
  const float* src[kTgtLevelsMax];             // the unclosed level (in scratch)
  float* dst[kTgtLevelsMax];
  int oh[kTgtLevelsMax], ow[kTgtLevelsMax], tiles_x[kTgtLevelsMax], tiles[kTgtLevelsMax];     // tiles: per sample
  int start[kTgtLevelsMax + 1];                // workgroup ids [start[l], start[l+1]) belong to level l
  int n;
};

template <int CTRL>
__device__ __forceinline__ int dpp_addi(int v) {   // the in-row steps of wave_group_sum (common.cuh) on an integer
  return v + __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// bytes of an 8-byte word that are not zero
__device__ __forceinline__ int tgt_nonzero_bytes(unsigned long long x) {
  constexpr unsigned long long k7f = 0x7f7f7f7f7f7f7f7full;
  return __popcll((((x & k7f) + k7f) | x) & ~k7f);
}

__device__ __forceinline__ float tgt_value(int count, int stride, int maxpool) {
  if (maxpool) return count > 0 ? 1.f : 0.f;
  return static_cast<float>(count) * (1.f / static_cast<float>(stride * stride));      // a power of two: exact
}

// foreground pixels of the 8 x 8 cell whose first pixel is (y0, x0) of sample `s` (H x W); pixels past H or W count as background
template <typename T, bool VEC>
__device__ __forceinline__ int tgt_count_cell(const T* __restrict__ s, int y0, int x0, int H, int W) {
  int cnt = 0;
  if constexpr (VEC && sizeof(T) == 1) {                     // W % 8 == 0: a cell's columns are all inside or all outside
    if (x0 < W) {
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (y0 + r < H) cnt += tgt_nonzero_bytes(*reinterpret_cast<const unsigned long long*>(s + static_cast<size_t>(y0 + r) * W + x0));
    }
  } else if constexpr (VEC) {                                // fp32, W % 4 == 0: each half of a cell's row is inside or outside
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (y0 + r >= H) continue;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int x = x0 + 4 * h;
        if (x >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(s + static_cast<size_t>(y0 + r) * W + x);
        cnt += (v.x > 0.f) + (v.y > 0.f) + (v.z > 0.f) + (v.w > 0.f);
      }
    }
  } else {
    for (int r = 0; r < 8; ++r) {
      if (y0 + r >= H) break;
      const T* row = s + static_cast<size_t>(y0 + r) * W;
      for (int c = 0; c < 8; ++c)
        if (x0 + c < W) cnt += row[x0 + c] > T(0);
    }
  }
  return cnt;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kBlock) void k_tgt_pool(const TgtArgs A) {
  const int lane = static_cast<int>(threadIdx.x) & (kWave - 1);
  const long long wave = static_cast<long long>(blockIdx.x) * (kBlock / kWave) + (threadIdx.x / kWave);
  const int per = A.tiles_y * A.tiles_x;
  if (wave >= static_cast<long long>(A.B) * per) return;     // whole waves leave: every lane of a wave that stays takes part in the sums
  const int b = static_cast<int>(wave / per), t = static_cast<int>(wave % per);
  const int cx = (t % A.tiles_x) * 8 + ((lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4));
  const int cy = (t / A.tiles_x) * 8 + (((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4));
  const T* s = static_cast<const T*>(A.src) + static_cast<size_t>(b) * A.H * A.W;
  const int c8 = tgt_count_cell<T, VEC>(s, cy * 8, cx * 8, A.H, A.W);     // 0 for a cell outside the image
  if (cy < A.oh[0] && cx < A.ow[0])
    A.dst[0][(static_cast<size_t>(b) * A.oh[0] + cy) * A.ow[0] + cx] = tgt_value(c8, 8, A.maxpool);
  if (A.n < 2) return;
  const int c16 = dpp_addi<0x4E>(dpp_addi<0xB1>(c8));         // quad_perm [1,0,3,2], [2,3,0,1]: every lane of a quad holds its 16-cell
  if ((lane & 3) == 0 && (cy >> 1) < A.oh[1] && (cx >> 1) < A.ow[1])
    A.dst[1][(static_cast<size_t>(b) * A.oh[1] + (cy >> 1)) * A.ow[1] + (cx >> 1)] = tgt_value(c16, 16, A.maxpool);
  if (A.n < 3) return;
  const int c32 = dpp_addi<0x140>(dpp_addi<0x141>(c16));      // row_half_mirror, row_mirror: every lane of a row of 16 holds its 32-cell
  if ((lane & 15) == 0 && (cy >> 2) < A.oh[2] && (cx >> 2) < A.ow[2])
    A.dst[2][(static_cast<size_t>(b) * A.oh[2] + (cy >> 2)) * A.ow[2] + (cx >> 2)] = tgt_value(c32, 32, A.maxpool);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_tgt_cells(const TgtArgs A) {
  const long long t = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= A.cell_start[A.n]) return;
  int l = 0;
#pragma unroll
  for (int i = 1; i < kTgtLevelsMax; ++i)
    if (i < A.n && t >= A.cell_start[i]) l = i;
  const long long local = t - A.cell_start[l];
  const int st = A.stride[l], oh = A.oh[l], ow = A.ow[l];
  const int x = static_cast<int>(local % ow), y = static_cast<int>((local / ow) % oh), b = static_cast<int>(local / (static_cast<long long>(ow) * oh));
  const T* s = static_cast<const T*>(A.src) + static_cast<size_t>(b) * A.H * A.W;
  const int y1 = min(y * st + st, A.H), x1 = min(x * st + st, A.W);
  int cnt = 0;
  for (int yy = y * st; yy < y1; ++yy) {
    const T* row = s + static_cast<size_t>(yy) * A.W;
    for (int xx = x * st; xx < x1; ++xx) cnt += row[xx] > T(0);
  }
  A.dst[l][local] = tgt_value(cnt, st, A.maxpool);
}

__global__ __launch_bounds__(kBlock) void k_tgt_close3(const TgtCloseArgs A) {
  constexpr int T = kTgtCloseTile, MW = T + 4, DW = T + 2;
  __shared__ float m[MW * MW];                 // the tile with a 2-cell halo; outside the level: 0, the max's neutral element
  __shared__ float d[DW * DW];                 // its dilation with a 1-cell halo; outside the level: 1, the min's neutral element
  int l = 0;
#pragma unroll
  for (int i = 1; i < kTgtLevelsMax; ++i)
    if (i < A.n && static_cast<int>(blockIdx.x) >= A.start[i]) l = i;
  const int local = static_cast<int>(blockIdx.x) - A.start[l];
  const int oh = A.oh[l], ow = A.ow[l];
  const int b = local / A.tiles[l], tile = local % A.tiles[l];
  const int y0 = (tile / A.tiles_x[l]) * T, x0 = (tile % A.tiles_x[l]) * T;
  const float* src = A.src[l] + static_cast<size_t>(b) * oh * ow;
  const int tid = static_cast<int>(threadIdx.x);
  for (int i = tid; i < MW * MW; i += kBlock) {
    const int y = y0 - 2 + i / MW, x = x0 - 2 + i % MW;
    m[i] = (y >= 0 && y < oh && x >= 0 && x < ow) ? src[static_cast<size_t>(y) * ow + x] : 0.f;
  }
  __syncthreads();
  for (int i = tid; i < DW * DW; i += kBlock) {
    const int r = i / DW, c = i % DW;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    float v = 1.f;
    if (y >= 0 && y < oh && x >= 0 && x < ow) {
      v = 0.f;
#pragma unroll
      for (int dr = 0; dr < 3; ++dr)
#pragma unroll
        for (int dc = 0; dc < 3; ++dc) v = fmaxf(v, m[(r + dr) * MW + c + dc]);
    }
    d[i] = v;
  }
  __syncthreads();
  const int ly = tid / T, lx = tid % T;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= oh || x >= ow) return;
  float v = 1.f;
#pragma unroll
  for (int dr = 0; dr < 3; ++dr)
#pragma unroll
    for (int dc = 0; dc < 3; ++dc) v = fminf(v, d[(ly + dr) * DW + lx + dc]);
  A.dst[l][(static_cast<size_t>(b) * oh + y) * ow + x] = v;
}

}  // namespace mgacbam
