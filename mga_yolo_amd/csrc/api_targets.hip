// libmgacbam.so, C ABI (include/mgatargets.h): the multi-scale segmentation targets from the batch's full-resolution masks
#include "host.cuh"
#include "targets.cuh"

#include "../../include/mgatargets.h"

static_assert(kTgtLevelsMax == MGATGT_MAX_LEVELS, "TgtArgs holds every level a call may carry");
static_assert(sizeof(mgatgt_desc_t) == 104, "the descriptor's layout (mirrored by _lib.TargetsDesc)");

// the scratch of a closing: every level's unclosed fp32 image, in level order
struct TgtLayout { size_t level[MGATGT_MAX_LEVELS]; size_t total; };

// Everything a descriptor is checked for that does not involve a pointer; fills the kernel arguments' geometry and the scratch layout.
// chain: the strides are a prefix of (8, 16, 32) -- k_tgt_pool
static int tgt_check(const char* what, const mgatgt_desc_t* D, TgtArgs& A, TgtLayout& L, bool& chain) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (D->n_levels < 1 || D->n_levels > MGATGT_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "%s: n_levels=%d (1 .. %d)", what, D->n_levels, MGATGT_MAX_LEVELS);
  if (D->B < 1 || D->H < 1 || D->W < 1 || static_cast<long long>(D->B) * D->H * D->W >= (1ll << 31))
    return fail(MGACBAM_E_SHAPE, "%s: B=%d H=%d W=%d (each >= 1, B*H*W < 2^31)", what, D->B, D->H, D->W);
  if (D->src_dtype != MGATGT_SRC_U8 && D->src_dtype != MGATGT_SRC_F32) return fail(MGACBAM_E_DTYPE, "%s: src_dtype %d", what, D->src_dtype);
  if (D->method != MGATGT_AVGPOOL && D->method != MGATGT_MAXPOOL) return fail(MGACBAM_E_ARG, "%s: method %d", what, D->method);
  if (D->flags & ~MGATGT_CLOSE3) return fail(MGACBAM_E_ARG, "%s: flags 0x%x (MGATGT_CLOSE3 is the only one)", what, D->flags);
  if ((D->flags & MGATGT_CLOSE3) && D->method != MGATGT_MAXPOOL)
    return fail(MGACBAM_E_ARG, "%s: MGATGT_CLOSE3 closes binary levels: it goes with MGATGT_MAXPOOL only", what);
  chain = D->n_levels <= 3;
  for (int l = 0; l < D->n_levels; ++l) {
    const int s = D->stride[l];
    if (s < 2 || s > 64 || (s & (s - 1)) != 0) return fail(MGACBAM_E_ARG, "%s: stride[%d]=%d (a power of two in 2 .. 64)", what, l, s);
    if (l > 0 && s <= D->stride[l - 1]) return fail(MGACBAM_E_ARG, "%s: stride[%d]=%d after %d (strictly ascending)", what, l, s, D->stride[l - 1]);
    chain = chain && s == (8 << l);
  }
  A.n = D->n_levels; A.B = D->B; A.H = D->H; A.W = D->W;
  A.maxpool = D->method == MGATGT_MAXPOOL;
  A.tiles_y = (D->H + kTgtTile - 1) / kTgtTile; A.tiles_x = (D->W + kTgtTile - 1) / kTgtTile;
  Carver cv;
  A.cell_start[0] = 0;
  for (int l = 0; l < MGATGT_MAX_LEVELS; ++l) {
    const bool on = l < D->n_levels;
    A.stride[l] = on ? D->stride[l] : 0;
    A.oh[l] = on ? (D->H + D->stride[l] - 1) / D->stride[l] : 0;
    A.ow[l] = on ? (D->W + D->stride[l] - 1) / D->stride[l] : 0;
    const size_t cells = static_cast<size_t>(D->B) * A.oh[l] * A.ow[l];
    A.cell_start[l + 1] = A.cell_start[l] + static_cast<long long>(cells);
    L.level[l] = cv.take(cells);
    A.dst[l] = nullptr;
  }
  L.total = (D->flags & MGATGT_CLOSE3) ? cv.total : 0;
  return 0;
}

extern "C" size_t mgatgt_scratch_bytes(const mgatgt_desc_t* desc) {
  TgtArgs A;
  TgtLayout L;
  bool chain;
  if (tgt_check("mgatgt_scratch_bytes", desc, A, L, chain)) return 0;
  g_err[0] = 0;
  return L.total;
}

template <typename T>
static auto tgt_pool_kernel(bool chain, bool vec) {
  if (!chain) return k_tgt_cells<T>;
  return vec ? k_tgt_pool<T, true> : k_tgt_pool<T, false>;
}

extern "C" int mgatgt_forward(const mgatgt_desc_t* D, void* stream) {
  const char* what = "mgatgt_forward";
  TgtArgs A;
  TgtLayout L;
  bool chain;
  if (int e = tgt_check(what, D, A, L, chain)) return e;
  const bool close3 = (D->flags & MGATGT_CLOSE3) != 0, f32 = D->src_dtype == MGATGT_SRC_F32;
  if (!D->src) return fail(MGACBAM_E_NULL, "%s: src is NULL", what);
  if (f32 && !aligned_to(D->src, 4)) return fail(MGACBAM_E_ALIGN, "%s: an fp32 src must be 4-byte aligned", what);
  for (int l = 0; l < D->n_levels; ++l) {
    if (!D->dst[l]) return fail(MGACBAM_E_NULL, "%s: dst[%d] is NULL", what, l);
    if (!aligned_to(D->dst[l], 4)) return fail(MGACBAM_E_ALIGN, "%s: dst[%d] must be 4-byte aligned", what, l);
  }
  if (close3) {
    if (!D->scratch) return fail(MGACBAM_E_NULL, "%s: MGATGT_CLOSE3 needs scratch", what);
    if (!aligned_to(D->scratch, 16)) return fail(MGACBAM_E_ALIGN, "%s: scratch must be 16-byte aligned", what);
    if (int e = check_capacity(what, "scratch", L.total, D->scratch_bytes)) return e;
  }
  A.src = D->src;
  for (int l = 0; l < D->n_levels; ++l) A.dst[l] = close3 ? at(D->scratch, L.level[l]) : D->dst[l];
  // the wide loads need every row of every sample to start on their boundary: the base address and W decide
  const bool vec = f32 ? (aligned_to(D->src, 16) && D->W % 4 == 0) : (aligned_to(D->src, 8) && D->W % 8 == 0);
  const long long threads = chain ? static_cast<long long>(D->B) * A.tiles_y * A.tiles_x * kWave : A.cell_start[D->n_levels];
  const long long grid = (threads + kBlock - 1) / kBlock;
  if (grid >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: the call's grid is too large", what);
  TgtCloseArgs Cl;
  long long cgrid = 0;
  if (close3) {
    Cl.n = D->n_levels;
    for (int l = 0; l < MGATGT_MAX_LEVELS; ++l) {
      const bool on = l < D->n_levels;
      Cl.src[l] = on ? A.dst[l] : nullptr; Cl.dst[l] = on ? D->dst[l] : nullptr;
      Cl.oh[l] = A.oh[l]; Cl.ow[l] = A.ow[l];
      Cl.tiles_x[l] = (A.ow[l] + kTgtCloseTile - 1) / kTgtCloseTile;
      Cl.tiles[l] = Cl.tiles_x[l] * ((A.oh[l] + kTgtCloseTile - 1) / kTgtCloseTile);
      Cl.start[l] = static_cast<int>(cgrid);
      cgrid += static_cast<long long>(D->B) * Cl.tiles[l];
      if (cgrid >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: the closing's grid is too large", what);
    }
    Cl.start[MGATGT_MAX_LEVELS] = static_cast<int>(cgrid);
  }
  const hipStream_t st = static_cast<hipStream_t>(stream);
  auto pool = f32 ? tgt_pool_kernel<float>(chain, vec) : tgt_pool_kernel<unsigned char>(chain, vec);
  if (int e = launch(chain ? "k_tgt_pool" : "k_tgt_cells", pool, grid, kBlock, 0, st, A)) return e;
  if (close3)
    if (int e = launch("k_tgt_close3", k_tgt_close3, cgrid, kBlock, 0, st, Cl)) return e;
  g_err[0] = 0;
  return 0;
}
