// libmgacbam.so, C ABI (include/mgacbam.h): MaskECA, the nearest resize and the ProbMaskGater gate
#include "host.cuh"
#include "eca.cuh"
#include "eca_nhwc.cuh"
#include "resize.cuh"
#include "gater.cuh"

// ------------------------------------------------------------------------------------------------
// MaskECA
// ------------------------------------------------------------------------------------------------
struct EcaCtxLayout { size_t S, use, den, avg, mavg, w, splane, total; };
static EcaCtxLayout eca_ctx_layout(int B, int C, int H, int W) {
  const size_t HW = static_cast<size_t>(H) * W, BC = static_cast<size_t>(B) * C;
  EcaCtxLayout L;
  Carver cv;
  L.S = cv.take(B); L.use = cv.take(B); L.den = cv.take(B);
  L.avg = cv.take(BC); L.mavg = cv.take(BC); L.w = cv.take(BC);
  L.splane = cv.take(B * HW);
  L.total = cv.total;
  return L;
}
static EcaCtx eca_ctx_ptrs(const void* p, int B, int C, int H, int W) {
  const EcaCtxLayout L = eca_ctx_layout(B, C, H, W);
  return EcaCtx{at(p, L.S), at(p, L.use), at(p, L.den), at(p, L.avg), at(p, L.mavg), at(p, L.w), at(p, L.splane)};
}
// Channels-last levels (MGACBAM_LAYOUT_NHWC, eca_nhwc.cuh) carry their chunk partials as a TAIL of the same buffers: the forward's pool
// partials after the ctx fields (whose layout stays as it is), the backward's gg partials after gg in scratch.  vec: nhwc_vec of the level.
constexpr int kEcaNhwcMaxC = 4096;                 // k_eca_bwd_nhwc keeps 3 floats per channel in LDS
static size_t eca_nhwc_ctx_tail(int B, int C, int H, int W, int vec) {
  return align16(static_cast<size_t>(B) * nhwc_geo(C, H, W, vec).nchunk * eca_nhwc_part_stride(C) * sizeof(float));
}
static size_t eca_nhwc_scratch_tail(int B, int C, int H, int W, int vec) {
  return align16(static_cast<size_t>(B) * nhwc_geo(C, H, W, vec).nchunk * C * sizeof(float));
}
static size_t eca_ctx_need(int B, int C, int H, int W, bool nhwc, int vec) {
  return eca_ctx_layout(B, C, H, W).total + (nhwc ? eca_nhwc_ctx_tail(B, C, H, W, vec) : 0);
}
static size_t eca_gg_bytes(int B, int C) { return align16(static_cast<size_t>(B) * C * 4); }
static size_t eca_scratch_need(int B, int C, int H, int W, bool nhwc, int vec) {
  return eca_gg_bytes(B, C) + (nhwc ? eca_nhwc_scratch_tail(B, C, H, W, vec) : 0);
}
// An NCHW level's backward (k_eca_bwd) keeps 3 floats per channel and 256 * vec combine floats in dynamic LDS beside its static red[]; a
// workgroup may ask for 64 KB in all.  kEcaNchwMaxC is the widest C that fits at vec 4 (the larger request), and the limit of every
// NCHW level whatever its vec: the forward refuses what the backward could not launch, and the size queries answer 0.
constexpr size_t kLdsPerWorkgroup = 64 * 1024;
constexpr size_t eca_bwd_smem(int C, int vec) { return (3 * static_cast<size_t>(C) + kBlock * vec) * sizeof(float); }
constexpr size_t eca_bwd_lds(int C, int vec) { return eca_bwd_smem(C, vec) + kEcaBwdRed * sizeof(float); }
constexpr int kEcaNchwMaxC = static_cast<int>((kLdsPerWorkgroup - eca_bwd_lds(0, 4)) / (eca_bwd_smem(1, 4) - eca_bwd_smem(0, 4)));
static_assert(eca_bwd_lds(kEcaNchwMaxC, 4) <= kLdsPerWorkgroup && eca_bwd_lds(kEcaNchwMaxC + 1, 4) > kLdsPerWorkgroup, "kEcaNchwMaxC");
static_assert(kEcaNchwMaxC >= kEcaNhwcMaxC, "a channels_last feature wider than kEcaNhwcMaxC is copied to NCHW");
static int eca_check_flags(const char* what, int flags, int C) {
  if (flags & ~MGACBAM_LAYOUT_NHWC) return fail(MGACBAM_E_SHAPE, "%s: unknown flag bits 0x%x (MGACBAM_LAYOUT_NHWC is the only one)", what, flags);
  if ((flags & MGACBAM_LAYOUT_NHWC) && C > kEcaNhwcMaxC)
    return fail(MGACBAM_E_SHAPE, "%s: a channels-last level takes C <= %d, got C=%d", what, kEcaNhwcMaxC, C);
  if (!(flags & MGACBAM_LAYOUT_NHWC) && C > kEcaNchwMaxC)
    return fail(MGACBAM_E_SHAPE, "%s: an NCHW level takes C <= %d (its backward keeps 3 floats per channel in the %zu bytes of LDS a workgroup "
                "may ask for), got C=%d", what, kEcaNchwMaxC, kLdsPerWorkgroup, C);
  return 0;
}
extern "C" size_t mgacbam_eca_ctx_bytes(int B, int C, int H, int W) {
  if (check_shape(B, C, H, W, 1, 3) || eca_check_flags("mgacbam_eca_ctx_bytes", 0, C)) return 0;
  return eca_ctx_layout(B, C, H, W).total;
}
extern "C" size_t mgacbam_eca_scratch_bytes(int B, int C, int H, int W) {
  if (check_shape(B, C, H, W, 1, 3) || eca_check_flags("mgacbam_eca_scratch_bytes", 0, C)) return 0;
  return eca_gg_bytes(B, C);
}
// the layout-aware queries take no element type: the answer covers every one (fp32 and fp16 / bf16 chunk differently)
extern "C" size_t mgacbam_eca_ctx_bytes_flags(int B, int C, int H, int W, int flags) {
  if (check_shape(B, C, H, W, 1, 3) || eca_check_flags("mgacbam_eca_ctx_bytes_flags", flags, C)) return 0;
  const bool nhwc = (flags & MGACBAM_LAYOUT_NHWC) != 0;
  return std::max(eca_ctx_need(B, C, H, W, nhwc, nhwc_vec(C, MGACBAM_F32)), eca_ctx_need(B, C, H, W, nhwc, nhwc_vec(C, MGACBAM_F16)));
}
extern "C" size_t mgacbam_eca_scratch_bytes_flags(int B, int C, int H, int W, int flags) {
  if (check_shape(B, C, H, W, 1, 3) || eca_check_flags("mgacbam_eca_scratch_bytes_flags", flags, C)) return 0;
  const bool nhwc = (flags & MGACBAM_LAYOUT_NHWC) != 0;
  return std::max(eca_scratch_need(B, C, H, W, nhwc, nhwc_vec(C, MGACBAM_F32)), eca_scratch_need(B, C, H, W, nhwc, nhwc_vec(C, MGACBAM_F16)));
}
static Geo eca_geo(int B, int C, int H, int W, const mgacbam_eca_params_t& p) {
  Geo g;
  g.B = B; g.C = C; g.H = H; g.W = W; g.HW = H * W; g.hidden = 1; g.k = p.k;
  g.use_sigmoid = p.use_sigmoid_mask; g.thr = p.tiny_thr; g.eps = p.eps; g.proj_h = 0;
  return g;
}

static int eca_check_params(const mgacbam_eca_params_t& p) {
  if (!p.w || !p.beta) return fail(MGACBAM_E_NULL, "eca: NULL parameter pointer");
  if (p.k < 1 || p.k > 15 || (p.k & 1) == 0) return fail(MGACBAM_E_SHAPE, "eca: conv1d kernel k=%d must be odd and in 1..15", p.k);
  return 0;
}
// What MaskECA groups by (host.cuh: the signature of a family).  gmask: dL/dmask is wanted (the backward; 0 in the forward); vec: along
// H*W, or along C for a channels-last level
struct EcaSig {
  int dtype, vec, has_mask, gmask, nhwc, weight;
  bool operator==(const EcaSig& o) const { return dtype == o.dtype && vec == o.vec && has_mask == o.has_mask && gmask == o.gmask && nhwc == o.nhwc; }
};
// One level of either direction (Level: mgacbam_eca_fwd_level_t / mgacbam_eca_bwd_level_t, Args: EcaFwdArgs / EcaBwdArgs) and layout:
// validated (NULL, parameters, shape, dtype, flags, alignment, capacity), then its kernel arguments; a channels-last level (sig.nhwc)
// also gets its chunk geometry and the partials' tail of ctx / scratch.
template <typename Level, typename Args>
static int eca_level(const char* what, const Level& L, Args& A, EcaSig& sig) {
  constexpr bool bwd = std::is_same_v<Args, EcaBwdArgs>;
  if constexpr (bwd) {
    if (!L.x || !L.gy || !L.ctx || !L.scratch || !L.gx || !L.gw || !L.gbeta) return fail(MGACBAM_E_NULL, "%s: NULL pointer", what);
    if (L.gmask && !L.mask) return fail(MGACBAM_E_NULL, "%s: gmask requested but mask is NULL", what);
  } else {
    if (!L.x || !L.y || !L.ctx) return fail(MGACBAM_E_NULL, "%s: x / y / ctx is NULL", what);
  }
  if (int e = eca_check_params(L.p)) return e;
  if (int e = check_shape(L.B, L.C, L.H, L.W, 1, L.p.k)) return e;
  if (int e = check_dtype(what, L.dtype)) return e;
  if (int e = eca_check_flags(what, L.flags, L.C)) return e;
  const bool nhwc = (L.flags & MGACBAM_LAYOUT_NHWC) != 0;
  const int VEC = level_vec(nhwc, L.C, L.H, L.W, L.dtype);
  const size_t need = VEC * elem_size(L.dtype);
  if constexpr (bwd) {
    if (!aligned_to(L.x, need) || !aligned_to(L.gy, need) || !aligned_to(L.gx, need) || !aligned_to(L.ctx, 16) ||
        !aligned_to(L.scratch, 16) || (L.gmask && !aligned_to(L.gmask, 16)))
      return fail(MGACBAM_E_ALIGN, "%s%s: x/gy/gx must be %zu-byte aligned, ctx/scratch/gmask 16-byte", what, nhwc ? " (NHWC)" : "", need);
    if (int e = check_capacity(what, "ctx", eca_ctx_need(L.B, L.C, L.H, L.W, nhwc, VEC), L.ctx_bytes)) return e;
    if (int e = check_capacity(what, "scratch", eca_scratch_need(L.B, L.C, L.H, L.W, nhwc, VEC), L.scratch_bytes)) return e;
    A.x = L.x; A.mask = L.mask; A.gy = L.gy; A.gx = L.gx; A.gmask = L.gmask; A.gw = L.gw; A.gbeta = L.gbeta;
    A.s.gg = static_cast<float*>(L.scratch);
  } else {
    if (!aligned_to(L.x, need) || !aligned_to(L.y, need) || !aligned_to(L.ctx, 16) || (L.mask && !aligned_to(L.mask, 16)))
      return fail(MGACBAM_E_ALIGN, "%s%s: x/y must be %zu-byte aligned, ctx and mask 16-byte", what, nhwc ? " (NHWC)" : "", need);
    if (int e = check_capacity(what, "ctx", eca_ctx_need(L.B, L.C, L.H, L.W, nhwc, VEC), L.ctx_bytes)) return e;
    A.x = L.x; A.mask = L.mask; A.y = L.y;
  }
  A.c = eca_ctx_ptrs(L.ctx, L.B, L.C, L.H, L.W);
  A.w1d = L.p.w; A.beta = L.p.beta;
  A.g = eca_geo(L.B, L.C, L.H, L.W, L.p);
  A.t = choose_tune(L.B, L.C, L.H, L.W, 7);
  A.n = NhwcGeo{}; A.part = nullptr;
  sig = EcaSig{};
  sig.dtype = L.dtype; sig.vec = VEC; sig.has_mask = L.mask != nullptr; sig.nhwc = nhwc;
  if constexpr (bwd) { sig.gmask = L.gmask != nullptr; A.nt = nhwc ? 0 : chan_tiles(A.t, L.H, L.W, VEC); }
  sig.weight = nhwc ? L.C : L.C * A.t.chan_tx;
  if (nhwc) {
    A.n = nhwc_geo(L.C, L.H, L.W, VEC);
    if constexpr (bwd) A.part = at(L.scratch, eca_gg_bytes(L.B, L.C));
    else A.part = at(L.ctx, eca_ctx_layout(L.B, L.C, L.H, L.W).total);
  }
  return 0;
}

static int eca_forward_group_nhwc(EcaFwdArgs* lv, int n, const EcaSig& sig, hipStream_t st);
static int eca_forward_group(EcaFwdArgs* lv, int n, const EcaSig& sig, hipStream_t st) {
  if (sig.nhwc) return eca_forward_group_nhwc(lv, n, sig, st);
  const int cpt = group_cpt(lv, n);
  for (int l = 0; l < n; ++l) lv[l].t.pool_cpt = cpt;
  Group<EcaFwdArgs> G = make_group(lv, n);
  auto sweeps = [&](const EcaFwdArgs& a) { return sweep_blocks(a, a.t.pool_tx, cpt); };
  auto pool = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_cpt(cpt, [&](auto c) {
    return with_bool(sig.has_mask, [&](auto m) { return k_eca_pool<elem_t<decltype(t)>, v.value, c.value, m.value>; }); }); });
  if (int e = launch_group("k_eca_pool", pool, G, sweeps, 0, st)) return e;
  auto apply = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
    return with_cpt(cpt, [&](auto c) { return k_eca_apply<elem_t<decltype(t)>, v.value, c.value>; }); });
  return launch_group("k_eca_apply", apply, G, sweeps, 0, st);
}

// channels-last levels: k_eca_pool_nhwc, k_eca_fin, k_eca_apply_nhwc
static int eca_forward_group_nhwc(EcaFwdArgs* lv, int n, const EcaSig& sig, hipStream_t st) {
  Group<EcaFwdArgs> G = make_group(lv, n);
  auto pool = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
    return with_bool(sig.has_mask, [&](auto m) { return k_eca_pool_nhwc<elem_t<decltype(t)>, v.value, m.value>; }); });
  if (int e = launch_group("k_eca_pool_nhwc", pool, G, [](const EcaFwdArgs& a) { return xcd_grid(a.g.B, a.n.nchunk); }, 0, st)) return e;
  auto fin = with_bool(sig.has_mask, [](auto m) { return k_eca_fin<m.value>; });
  if (int e = launch_group("k_eca_fin", fin, G, [](const EcaFwdArgs& a) { return nhwc_fold_blocks(a.g); }, 0, st)) return e;
  auto apply = with_elem_vec8(sig.dtype, sig.vec, [](auto t, auto v) { return k_eca_apply_nhwc<elem_t<decltype(t)>, v.value>; });
  return launch_group("k_eca_apply_nhwc", apply, G, [](const EcaFwdArgs& a) { return xcd_grid(a.g.B, a.n.ntile); },
                      [](const EcaFwdArgs& a) { return lds_bytes(EcaApplyNhwcLds(a.g)); }, st);
}

extern "C" int mgacbam_eca_forward(const mgacbam_eca_fwd_level_t* levels, int n_levels, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<EcaFwdArgs, EcaSig>(levels, n_levels, true,
      [](const mgacbam_eca_fwd_level_t& L, EcaFwdArgs& A, EcaSig& s) { return eca_level("eca forward", L, A, s); },
      [&](EcaFwdArgs* g, int m, const EcaSig& s) { return eca_forward_group(g, m, s, st); });
}

static int eca_backward_group_nhwc(EcaBwdArgs* lv, int n, const EcaSig& sig, hipStream_t st);
static int eca_backward_group(EcaBwdArgs* lv, int n, const EcaSig& sig, hipStream_t st) {
  if (sig.nhwc) return eca_backward_group_nhwc(lv, n, sig, st);
  const int cpt = group_cpt(lv, n);
  for (int l = 0; l < n; ++l) lv[l].t.pool_cpt = cpt;
  Group<EcaBwdArgs> G = make_group(lv, n);
  auto reduce = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
    return with_cpt(cpt, [&](auto c) { return k_eca_reduce<elem_t<decltype(t)>, v.value, c.value>; }); });
  if (int e = launch_group("k_eca_reduce", reduce, G, [&](const EcaBwdArgs& a) { return sweep_blocks(a, a.t.pool_tx, cpt); }, 0, st)) return e;
  auto bwd = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
    return with_bool(sig.gmask, [&](auto gm) { return k_eca_bwd<elem_t<decltype(t)>, v.value, gm.value>; }); });
  return launch_group("k_eca_bwd", bwd, G, [](const EcaBwdArgs& a) { return kEcaRoles + xcd_grid(a.g.B, a.nt); },
                      [&](const EcaBwdArgs& a) { return eca_bwd_smem(a.g.C, sig.vec); }, st);
}

// channels-last levels: k_eca_reduce_nhwc, k_eca_fold, k_eca_bwd_nhwc (+ the layout-free role workgroups)
static int eca_backward_group_nhwc(EcaBwdArgs* lv, int n, const EcaSig& sig, hipStream_t st) {
  Group<EcaBwdArgs> G = make_group(lv, n);
  auto reduce = with_elem_vec8(sig.dtype, sig.vec, [](auto t, auto v) { return k_eca_reduce_nhwc<elem_t<decltype(t)>, v.value>; });
  if (int e = launch_group("k_eca_reduce_nhwc", reduce, G, [](const EcaBwdArgs& a) { return xcd_grid(a.g.B, a.n.nchunk); }, 0, st)) return e;
  if (int e = launch_group("k_eca_fold", k_eca_fold, G, [](const EcaBwdArgs& a) { return nhwc_fold_blocks(a.g); }, 0, st)) return e;
  auto bwd = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
    return with_bool(sig.gmask, [&](auto gm) { return k_eca_bwd_nhwc<elem_t<decltype(t)>, v.value, gm.value>; }); });
  return launch_group("k_eca_bwd_nhwc", bwd, G, [](const EcaBwdArgs& a) { return kEcaRoles + xcd_grid(a.g.B, a.n.ntile); },
                      [](const EcaBwdArgs& a) { return lds_bytes(EcaBwdNhwcLds(a.g)); }, st);
}

extern "C" int mgacbam_eca_backward(const mgacbam_eca_bwd_level_t* levels, int n_levels, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<EcaBwdArgs, EcaSig>(levels, n_levels, true,
      [](const mgacbam_eca_bwd_level_t& L, EcaBwdArgs& A, EcaSig& s) { return eca_level("eca backward", L, A, s); },
      [&](EcaBwdArgs* g, int m, const EcaSig& s) { return eca_backward_group(g, m, s, st); });
}

// ------------------------------------------------------------------------------------------------
// nearest-neighbour resize (integer index path)
// ------------------------------------------------------------------------------------------------
extern "C" int mgacbam_resize_nearest(const float* src, float* dst, int n_planes, int in_h, int in_w, int out_h, int out_w,
                                      void* stream) {
  if (!src || !dst) return fail(MGACBAM_E_NULL, "resize: NULL pointer");
  if (n_planes < 1 || in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1) return fail(MGACBAM_E_SHAPE, "resize: bad shape");
  const size_t total = static_cast<size_t>(n_planes) * out_h * out_w;
  size_t grid = (total + kBlock - 1) / kBlock;
  if (grid > 4096) grid = 4096;
  if (int e = launch("k_resize_nearest", k_resize_nearest, grid, kBlock, 0, static_cast<hipStream_t>(stream), src, dst, n_planes, in_h, in_w,
                     out_h, out_w)) return e;
  g_err[0] = 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// ProbMaskGater
// ------------------------------------------------------------------------------------------------
static int pmg_args(size_t n, const mgapmg_cfg_t* cfg, GaterArgs& A) {
  if (!cfg) return fail(MGACBAM_E_NULL, "gater: cfg is NULL");
  if (n < 1 || !(cfg->tau > 0.f)) return fail(MGACBAM_E_SHAPE, "gater: n=%zu tau=%g", n, cfg->tau);
  A.n = n; A.inv_tau = 1.f / cfg->tau; A.p_min = cfg->p_min; A.threshold = cfg->threshold; A.hard = cfg->hard ? 1 : 0;
  A.p = A.u1 = A.u2 = A.gout = nullptr; A.out = A.msoft = A.gp = nullptr;
  return 0;
}
static unsigned pmg_grid(size_t n) { const size_t g = (n + kBlock - 1) / kBlock; return static_cast<unsigned>(g > 2048 ? 2048 : g); }
extern "C" int mgapmg_forward(const float* p, const float* u1, const float* u2, float* out, float* msoft, size_t n,
                              const mgapmg_cfg_t* cfg, void* stream) {
  if (!p || !u1 || !u2 || !out || !msoft) return fail(MGACBAM_E_NULL, "gater: NULL pointer");
  GaterArgs A;
  if (int e = pmg_args(n, cfg, A)) return e;
  A.p = p; A.u1 = u1; A.u2 = u2; A.out = out; A.msoft = msoft;
  if (int e = launch("k_pmg_fwd", k_pmg_fwd, pmg_grid(n), kBlock, 0, static_cast<hipStream_t>(stream), A)) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgapmg_backward(const float* p, const float* msoft, const float* gout, float* gp, size_t n, const mgapmg_cfg_t* cfg,
                               void* stream) {
  if (!p || !msoft || !gout || !gp) return fail(MGACBAM_E_NULL, "gater: NULL pointer");
  GaterArgs A;
  if (int e = pmg_args(n, cfg, A)) return e;
  A.p = p; A.msoft = const_cast<float*>(msoft); A.gout = gout; A.gp = gp;
  if (int e = launch("k_pmg_bwd", k_pmg_bwd, pmg_grid(n), kBlock, 0, static_cast<hipStream_t>(stream), A)) return e;
  g_err[0] = 0;
  return 0;
}
