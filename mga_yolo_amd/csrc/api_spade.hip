// libmgacbam.so, C ABI (include/mgaspade.h): MaskSPADE
#include "host.cuh"
#include "../../include/mgaspade.h"
#include "spade_nhwc.cuh"
#include "resample.cuh"

constexpr int kSpMaxC = 1024;
constexpr int kSpDwTarget = 512;     // workgroups k_spade_dw aims for: (C / 16) M tiles x pixel chunks

struct SpTiling { int TW, TH, ltw, tiles_x, tiles; };
// TW in {4, 8, 16, 32} (TH = 128 / TW): the choice that pads the level's H x W the least, the widest rows on a tie
static SpTiling sp_tiling(int H, int W) {
  SpTiling best{};
  long long best_px = -1;
  for (int ltw = 5; ltw >= 2; --ltw) {
    const int TW = 1 << ltw, TH = kSpPx / TW;
    const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;
    const long long px = static_cast<long long>(tx) * ty;
    if (best_px < 0 || px < best_px) { best_px = px; best = SpTiling{TW, TH, ltw, tx, tx * ty}; }
  }
  return best;
}
struct SpLayout { size_t mean, rstd, wpack, wpackT, gamma, base; };
static SpLayout sp_ctx_layout(int B, int C, int hidden) {
  SpLayout L;
  Carver cv;
  const size_t BC = static_cast<size_t>(B) * C, nw = static_cast<size_t>(2) * 9 * C * hidden;
  L.mean = cv.take(BC); L.rstd = cv.take(BC); L.wpack = cv.take(nw); L.wpackT = cv.take(nw);
  L.gamma = cv.total; L.base = cv.total;
  return L;
}
static size_t sp_gamma_bytes(int B, int C, int H, int W, size_t elem) { return align16(static_cast<size_t>(B) * C * H * W * elem); }
struct SpScratch { size_t red, stat, dwpart, u, w0part, total; int nchunk, tpc; };
static SpScratch sp_scratch_layout(int B, int C, int H, int W, int hidden) {
  const SpTiling t = sp_tiling(H, W);
  const int total = B * t.tiles;
  int nchunk = std::max(1, std::min(total, kSpDwTarget / (C / 16)));
  const int tpc = (total + nchunk - 1) / nchunk;
  nchunk = (total + tpc - 1) / tpc;
  SpScratch L;
  Carver cv;
  const size_t BC = static_cast<size_t>(B) * C;
  L.red = cv.take(4 * BC); L.stat = cv.take(2 * BC);
  L.dwpart = cv.take(static_cast<size_t>(nchunk) * 2 * C * hidden * 9);
  L.u = cv.take(static_cast<size_t>(B) * 9 * H * W);
  L.w0part = cv.take(static_cast<size_t>(total) * hidden * 10);
  L.total = cv.total; L.nchunk = nchunk; L.tpc = tpc;
  return L;
}
static int sp_check_shape(const char* what, int B, int C, int H, int W, int hidden) {
  if (int e = check_shape(B, C, H, W, hidden, 3)) return e;
  if (hidden % 16 || hidden > kSpMaxHid) return fail(MGACBAM_E_SHAPE, "%s: hidden=%d must be a multiple of 16 and <= %d", what, hidden, kSpMaxHid);
  if (C % 16 || C > kSpMaxC) return fail(MGACBAM_E_SHAPE, "%s: C=%d must be a multiple of 16 and <= %d", what, C, kSpMaxC);
  if (static_cast<long long>(B) * C * H * W >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: tensor too large B=%d C=%d H=%d W=%d", what, B, C, H, W);
  return 0;
}
extern "C" size_t mgaspade_ctx_bytes(int B, int C, int H, int W, int hidden) {
  if (sp_check_shape("mgaspade_ctx_bytes", B, C, H, W, hidden)) return 0;
  return sp_ctx_layout(B, C, hidden).base + sp_gamma_bytes(B, C, H, W, 4);
}
extern "C" size_t mgaspade_scratch_bytes(int B, int C, int H, int W, int hidden) {
  if (sp_check_shape("mgaspade_scratch_bytes", B, C, H, W, hidden)) return 0;
  return sp_scratch_layout(B, C, H, W, hidden).total;
}

static size_t sp_head_floats(const SpadeArgs& a) { return ((a.hid * 10 + 3) & ~3) + (((a.TH + 4) * (a.TW + 4) + 3) & ~3); }
static size_t sp_nph(const SpadeArgs& a) { return static_cast<size_t>(a.TH + 2) * (a.TW + 2); }
static size_t sp_fwd_smem(const SpadeArgs& a) { return (sp_head_floats(a) + sp_nph(a) * (a.hid + 4)) * sizeof(float); }
static size_t sp_dw_smem(const SpadeArgs& a) { return (sp_head_floats(a) + ((sp_nph(a) * a.hid + 3) & ~size_t(3)) + 2 * 16 * kSpAStride) * sizeof(float); }
static size_t sp_dh_smem(const SpadeArgs& a) {
  const size_t cc = std::min(a.C, kSpDhCC);
  return (sp_head_floats(a) + std::max(sp_nph(a) * 2 * (cc + 4), static_cast<size_t>(a.hid) * kSpAStride)) * sizeof(float);
}
// dynamic LDS above 48 KB: the kernel's limit is raised first (an attribute of the function: no stream work, no allocation)
// Done once per (device, kernel) and size reached, so a warmed-up call -- the state a stream capture starts from -- makes no runtime call here.
template <typename K>
static void sp_allow_lds(K kernel, size_t smem) {
  if (smem <= 48 * 1024) return;
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> allowed;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  const auto key = std::make_pair(dev, reinterpret_cast<const void*>(kernel));
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = allowed[key];
  if (have >= smem) return;
  if (hipFuncSetAttribute(key.second, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(smem)) == hipSuccess) have = smem;
}

// What MaskSPADE groups by (host.cuh: the signature of a family).  keep: the forward keeps gamma in the ctx (0 in the backward);
// gmask: dL/dmask is wanted (the backward; 0 in the forward)
struct SpadeSig {
  int dtype, has_mask, nhwc, keep, gmask, weight;
  bool operator==(const SpadeSig& o) const { return dtype == o.dtype && has_mask == o.has_mask && nhwc == o.nhwc && keep == o.keep && gmask == o.gmask; }
};
// everything a level is checked for before the first launch, and its kernel arguments
static int sp_level(const char* what, const mgaspade_level_t& L, bool bwd, SpadeArgs& A, SpadeSig& sig) {
  if (!L.x || !L.ctx) return fail(MGACBAM_E_NULL, "%s: x / ctx is NULL", what);
  if (!bwd && !L.y) return fail(MGACBAM_E_NULL, "%s: y is NULL", what);
  if (bwd && (!L.gy || !L.gx || !L.scratch)) return fail(MGACBAM_E_NULL, "%s: gy / gx / scratch is NULL", what);
  if (L.flags != 0 && L.flags != MGASPADE_LAYOUT_NHWC)
    return fail(MGACBAM_E_SHAPE, "%s: flags=0x%x (0 or MGASPADE_LAYOUT_NHWC; every other bit is reserved)", what, L.flags);
  if (int e = sp_check_shape(what, L.B, L.C, L.H, L.W, L.hidden)) return e;
  if (int e = check_dtype(what, L.dtype)) return e;
  if (L.norm_type != MGASPADE_NORM_IN && L.norm_type != MGASPADE_NORM_BN) return fail(MGACBAM_E_SHAPE, "%s: norm_type %d", what, L.norm_type);
  const bool bn = L.norm_type == MGASPADE_NORM_BN;
  if (bn && (!L.running_mean || !L.running_var)) return fail(MGACBAM_E_NULL, "%s: batch norm needs running_mean / running_var", what);
  if (!(L.eps >= 0.f)) return fail(MGACBAM_E_SHAPE, "%s: eps=%g", what, L.eps);
  const long long per = bn && L.training ? static_cast<long long>(L.B) * L.H * L.W : static_cast<long long>(L.H) * L.W;
  if (!bwd && (!bn || L.training) && per < 2) return fail(MGACBAM_E_SHAPE, "%s: the normalisation needs more than one value per channel", what);
  if (L.mask && (!L.w0 || !L.b0 || !L.wg || !L.bg || !L.wb || !L.bb)) return fail(MGACBAM_E_NULL, "%s: NULL parameter pointer", what);
  if (bwd && L.mask && (!L.gw0 || !L.gb0 || !L.gwg || !L.gbg || !L.gwb || !L.gbb)) return fail(MGACBAM_E_NULL, "%s: NULL parameter-gradient pointer", what);
  if (bwd && L.gmask && !L.mask) return fail(MGACBAM_E_NULL, "%s: gmask requested but mask is NULL", what);
  if (!aligned_to(L.x, 16) || !aligned_to(L.ctx, 16) || (!bwd && !aligned_to(L.y, 16)) ||
      (bwd && (!aligned_to(L.gy, 16) || !aligned_to(L.gx, 16) || !aligned_to(L.scratch, 16))) || (L.mask && !aligned_to(L.mask, 16)))
    return fail(MGACBAM_E_ALIGN, "%s: x / y / gy / gx / ctx / scratch / mask must be 16-byte aligned", what);
  const SpLayout CL = sp_ctx_layout(L.B, L.C, L.hidden);
  const bool gamma_kept = L.mask && (bwd || L.save_gamma);
  if (int e = check_capacity(what, "ctx", CL.base + (gamma_kept ? sp_gamma_bytes(L.B, L.C, L.H, L.W, elem_size(L.dtype)) : 0), L.ctx_bytes)) return e;
  const SpScratch SL = sp_scratch_layout(L.B, L.C, L.H, L.W, L.hidden);
  if (bwd) if (int e = check_capacity(what, "scratch", SL.total, L.scratch_bytes)) return e;
  const SpTiling t = sp_tiling(L.H, L.W);
  A = SpadeArgs{};
  A.x = L.x; A.mask = L.mask; A.y = L.y; A.gy = L.gy; A.gx = L.gx; A.gmask = L.gmask;
  A.w0 = L.w0; A.b0 = L.b0; A.wg = L.wg; A.bg = L.bg; A.wb = L.wb; A.bb = L.bb;
  A.rmean = L.running_mean; A.rvar = L.running_var; A.nbt = L.num_batches_tracked;
  A.gw0 = L.gw0; A.gb0 = L.gb0; A.gwg = L.gwg; A.gbg = L.gbg; A.gwb = L.gwb; A.gbb = L.gbb;
  A.mean = at(L.ctx, CL.mean); A.rstd = at(L.ctx, CL.rstd); A.wpack = at(L.ctx, CL.wpack); A.wpackT = at(L.ctx, CL.wpackT);
  A.gamma = gamma_kept ? at<void>(L.ctx, CL.gamma) : nullptr;
  if (bwd) {
    A.red = at(L.scratch, SL.red); A.stat = at(L.scratch, SL.stat); A.dwpart = at(L.scratch, SL.dwpart); A.u = at(L.scratch, SL.u);
    A.w0part = at(L.scratch, SL.w0part);
  }
  A.B = L.B; A.C = L.C; A.H = L.H; A.W = L.W; A.HW = L.H * L.W; A.hid = L.hidden;
  A.bn = bn; A.train = L.training ? 1 : 0; A.use_sigmoid = L.use_sigmoid_mask ? 1 : 0; A.has_mask = L.mask ? 1 : 0;
  A.eps = L.eps; A.momentum = L.momentum;
  A.TW = t.TW; A.TH = t.TH; A.ltw = t.ltw; A.tiles_x = t.tiles_x; A.tiles = t.tiles;
  // channels per forward workgroup: halved while the grid is small, always whole 16-channel M tiles (the last block may hold fewer)
  int cblk = std::min(L.C, 256);
  while (cblk > 64 && static_cast<long long>(L.B) * t.tiles * ((L.C + cblk - 1) / cblk) < 512) cblk = (cblk / 2 + 15) & ~15;
  A.cblk = cblk; A.ncb = (L.C + cblk - 1) / cblk;
  A.nchunk = SL.nchunk; A.tpc = SL.tpc;
  sig = SpadeSig{};
  sig.dtype = L.dtype; sig.has_mask = L.mask != nullptr; sig.nhwc = L.flags == MGASPADE_LAYOUT_NHWC;
  if (bwd) sig.gmask = L.gmask != nullptr; else sig.keep = gamma_kept;
  sig.weight = L.C;
  return 0;
}
static int sp_ew_blocks(const SpadeArgs& a) {
  const long long n = (static_cast<long long>(a.B) * a.C * a.HW + kBlock - 1) / kBlock;
  return static_cast<int>(std::min<long long>(n, 4096));
}
static int sp_plane_blocks(const SpadeArgs& a) { return (a.B * a.C + 3) / 4; }

static int sp_pack_blocks(const SpadeArgs& a) { return (2 * a.C * a.hid * 9 + kBlock - 1) / kBlock; }

// Channels-last levels (SpadeSig::nhwc: launch groups of their own) run the same launches with the kernels' NHWC instantiations; tiling, grids
// of the tile kernels, ctx and scratch are the NCHW ones.  Their reductions (spade_nhwc.cuh) take 16 channels of a sample per workgroup.
static int sp_nhwc_plane_blocks(const SpadeArgs& a) { return a.B * (a.C / kSpNhCB); }
static int sp_nhwc_bn_blocks(const SpadeArgs& a) { return a.bn && a.train ? (a.C / kSpNhCB) * (kBlock / kWave) : 0; }
static int sp_nhwc_bn_fin_blocks(const SpadeArgs& a) { return a.bn && a.train ? (a.C + kBlock - 1) / kBlock : 0; }
static int sp_stats_nhwc(Group<SpadeArgs>& G, const SpadeSig& sig, hipStream_t st) {
  auto stats = with_elem(sig.dtype, [](auto t) { return k_spade_stats_nhwc<elem_t<decltype(t)>>; });
  auto stat_blocks = [](const SpadeArgs& a) { return !a.bn ? sp_nhwc_plane_blocks(a) : a.train ? sp_nhwc_bn_blocks(a) : (a.B * a.C + kBlock - 1) / kBlock; };
  if (int e = launch_group("k_spade_stats_nhwc", stats, G, stat_blocks, 0, st)) return e;
  bool bn_train = false;
  for (int l = 0; l < G.n; ++l) bn_train = bn_train || (G.lv[l].bn && G.lv[l].train);
  if (!bn_train) return 0;
  // batch norm in training (the other levels get no workgroup): the mean from the four parked sums, the centred squares, then rstd and
  // the running statistics.  The sums are parked in ctx where k_spade_pack, which runs after this, writes the weight packs.
  if (int e = launch_group("k_spade_bn_fin_nhwc", k_spade_bn_fin_nhwc<false>, G, sp_nhwc_bn_fin_blocks, 0, st)) return e;
  auto sq = with_elem(sig.dtype, [](auto t) { return k_spade_bn_sq_nhwc<elem_t<decltype(t)>>; });
  if (int e = launch_group("k_spade_bn_sq_nhwc", sq, G, sp_nhwc_bn_blocks, 0, st)) return e;
  return launch_group("k_spade_bn_fin_nhwc", k_spade_bn_fin_nhwc<true>, G, sp_nhwc_bn_fin_blocks, 0, st);
}
// T x layout: f(Ty<T>, std::bool_constant<NHWC>)
template <typename F>
static auto with_elem_layout(const SpadeSig& sig, F f) {
  return with_elem(sig.dtype, [&](auto t) { return with_bool(sig.nhwc, [&](auto n) { return f(t, n); }); });
}

static int sp_forward_group(SpadeArgs* lv, int n, const SpadeSig& sig, hipStream_t st) {
  Group<SpadeArgs> G = make_group(lv, n);
  if (sig.nhwc) {
    if (int e = sp_stats_nhwc(G, sig, st)) return e;
  } else {
    auto stats = with_elem(sig.dtype, [](auto t) { return k_spade_stats<elem_t<decltype(t)>>; });
    auto stat_blocks = [](const SpadeArgs& a) { return !a.bn ? sp_plane_blocks(a) : a.train ? a.C : (a.B * a.C + kBlock - 1) / kBlock; };
    if (int e = launch_group("k_spade_stats", stats, G, stat_blocks, 0, st)) return e;
  }
  if (!sig.has_mask) {
    auto ew = with_elem_layout(sig, [](auto t, auto l) { return k_spade_ew<elem_t<decltype(t)>, 0, decltype(l)::value>; });
    return launch_group("k_spade_ew", ew, G, sp_ew_blocks, 0, st);
  }
  if (int e = launch_group("k_spade_pack", k_spade_pack, G, sp_pack_blocks, 0, st)) return e;
  auto fwd = with_elem_layout(sig, [&](auto t, auto l) {
    return with_bool(sig.keep, [](auto keep) { return k_spade_fwd<elem_t<decltype(t)>, keep.value, decltype(l)::value>; }); });
  sp_allow_lds(fwd, group_smem(G, sp_fwd_smem));
  return launch_group("k_spade_fwd", fwd, G, [](const SpadeArgs& a) { return a.B * a.tiles * a.ncb; }, sp_fwd_smem, st);
}

static int sp_backward_group(SpadeArgs* lv, int n, const SpadeSig& sig, hipStream_t st) {
  Group<SpadeArgs> G = make_group(lv, n);
  if (sig.nhwc) {
    auto reduce = with_elem(sig.dtype, [](auto t) { return k_spade_bwd_reduce_nhwc<elem_t<decltype(t)>>; });
    if (int e = launch_group("k_spade_bwd_reduce_nhwc", reduce, G, sp_nhwc_plane_blocks, 0, st)) return e;
  } else {
    auto reduce = with_elem(sig.dtype, [](auto t) { return k_spade_bwd_reduce<elem_t<decltype(t)>>; });
    if (int e = launch_group("k_spade_bwd_reduce", reduce, G, sp_plane_blocks, 0, st)) return e;
  }
  if (int e = launch_group("k_spade_bwd_fin", k_spade_bwd_fin, G, [](const SpadeArgs& a) { return (a.C + kBlock - 1) / kBlock; }, 0, st)) return e;
  if (sig.has_mask) {
    auto dw = with_elem_layout(sig, [](auto t, auto l) { return k_spade_dw<elem_t<decltype(t)>, decltype(l)::value>; });
    sp_allow_lds(dw, group_smem(G, sp_dw_smem));
    if (int e = launch_group("k_spade_dw", dw, G, [](const SpadeArgs& a) { return (a.C / 16) * a.nchunk; }, sp_dw_smem, st)) return e;
    if (int e = launch_group("k_spade_dw_fin", k_spade_dw_fin, G, sp_pack_blocks, 0, st)) return e;
    auto dh = with_elem_layout(sig, [](auto t, auto l) { return k_spade_dh<elem_t<decltype(t)>, decltype(l)::value>; });
    sp_allow_lds(dh, group_smem(G, sp_dh_smem));
    if (int e = launch_group("k_spade_dh", dh, G, [](const SpadeArgs& a) { return a.B * a.tiles; }, sp_dh_smem, st)) return e;
    if (int e = launch_group("k_spade_w0_fin", k_spade_w0_fin, G, [](const SpadeArgs& a) { return a.hid * 10; }, 0, st)) return e;
    if (sig.gmask)
      if (int e = launch_group("k_spade_gmask", k_spade_gmask, G,
                               [](const SpadeArgs& a) { return (a.B * a.HW + kBlock - 1) / kBlock; }, 0, st)) return e;
  }
  auto ew = with_elem_layout(sig, [](auto t, auto l) { return k_spade_ew<elem_t<decltype(t)>, 1, decltype(l)::value>; });
  return launch_group("k_spade_ew", ew, G, sp_ew_blocks, 0, st);
}

static int sp_run(const char* what, const mgaspade_level_t* levels, int n_levels, void* stream, bool bwd) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<SpadeArgs, SpadeSig>(levels, n_levels, false, [&](const mgaspade_level_t& L, SpadeArgs& A, SpadeSig& s) { return sp_level(what, L, bwd, A, s); },
      [&](SpadeArgs* g, int m, const SpadeSig& s) { return bwd ? sp_backward_group(g, m, s, st) : sp_forward_group(g, m, s, st); });
}
extern "C" int mgaspade_forward(const mgaspade_level_t* levels, int n_levels, void* stream) {
  return sp_run("mgaspade_forward", levels, n_levels, stream, false);
}
extern "C" int mgaspade_backward(const mgaspade_level_t* levels, int n_levels, void* stream) {
  return sp_run("mgaspade_backward", levels, n_levels, stream, true);
}

// ------------------------------------------------------------------------------------------------
// the mask resample of the static plans (include/mgaresample.h): one launch per direction for every level of the call
// ------------------------------------------------------------------------------------------------
static_assert(kResampleLevelsMax == MGACBAM_MAX_LEVELS, "ResampleGroup holds every level a call may carry");
constexpr int kResampleMaxSize = 65536;     // per axis: the adjoint's inverse map is fp32 arithmetic, exact enough (one index) far beyond this

// everything a call is checked for before its launch, and the kernel's arguments; returns the grid in `grid`
static int resample_group(const char* what, const mgaspade_resample_level_t* levels, int n_levels, bool bwd, ResampleGroup& G, int& grid) {
  if (!levels) return fail(MGACBAM_E_NULL, "%s: levels is NULL", what);
  if (n_levels < 1 || n_levels > MGACBAM_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "%s: n_levels=%d", what, n_levels);
  G.n = n_levels;
  grid = 0;
  for (int l = 0; l < n_levels; ++l) {
    const mgaspade_resample_level_t& L = levels[l];
    if (!L.src || !L.dst) return fail(MGACBAM_E_NULL, "%s: level %d: src / dst is NULL", what, l);
    const int dims[5] = {L.B, L.in_h, L.in_w, L.out_h, L.out_w};
    for (int d : dims)
      if (d < 1 || d > kResampleMaxSize)
        return fail(MGACBAM_E_SHAPE, "%s: level %d: B=%d in=%dx%d out=%dx%d (every size in 1..%d)", what, l, L.B, L.in_h, L.in_w, L.out_h, L.out_w,
                    kResampleMaxSize);
    const long long n_in = static_cast<long long>(L.B) * L.in_h * L.in_w, n_out = static_cast<long long>(L.B) * L.out_h * L.out_w;
    if (n_in >= (1ll << 31) || n_out >= (1ll << 31))
      return fail(MGACBAM_E_SHAPE, "%s: level %d: tensor too large B=%d in=%dx%d out=%dx%d", what, l, L.B, L.in_h, L.in_w, L.out_h, L.out_w);
    if (!aligned_to(L.src, 4) || !aligned_to(L.dst, 4)) return fail(MGACBAM_E_ALIGN, "%s: level %d: fp32 buffers must be 4-byte aligned", what, l);
    ResampleLevel& A = G.lv[l];
    A.src = L.src; A.dst = L.dst; A.B = L.B; A.in_h = L.in_h; A.in_w = L.in_w; A.out_h = L.out_h; A.out_w = L.out_w;
    A.vec = (!bwd && L.out_w % 4 == 0 && aligned_to(L.dst, 16)) ? 4 : 1;
    const long long threads = bwd ? n_in : n_out / A.vec;
    const long long blocks = (threads + kBlock - 1) / kBlock;
    if (grid + blocks >= (1ll << 31)) return fail(MGACBAM_E_SHAPE, "%s: the call's grid is too large", what);
    G.start[l] = grid;
    grid += static_cast<int>(blocks);
  }
  for (int l = n_levels; l <= kResampleLevelsMax; ++l) G.start[l] = grid;
  return 0;
}
static int resample_run(const char* what, const mgaspade_resample_level_t* levels, int n_levels, void* stream, bool bwd) {
  ResampleGroup G;
  int grid;
  if (int e = resample_group(what, levels, n_levels, bwd, G, grid)) return e;
  if (int e = launch(bwd ? "k_resample_bwd" : "k_resample_fwd", bwd ? k_resample_bwd : k_resample_fwd, grid, kBlock, 0,
                     static_cast<hipStream_t>(stream), G)) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgaspade_resample_forward(const mgaspade_resample_level_t* levels, int n_levels, void* stream) {
  return resample_run("mgaspade_resample_forward", levels, n_levels, stream, false);
}
extern "C" int mgaspade_resample_backward(const mgaspade_resample_level_t* levels, int n_levels, void* stream) {
  return resample_run("mgaspade_resample_backward", levels, n_levels, stream, true);
}
