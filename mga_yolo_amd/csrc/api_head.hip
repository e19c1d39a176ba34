// libmgacbam.so, C ABI (include/mgacbam.h): MGAMaskHead
#include "host.cuh"
#include "head_nhwc.cuh"

// ------------------------------------------------------------------------------------------------
// MGAMaskHead
// ------------------------------------------------------------------------------------------------
static int head_check_shape(int B, int C, int H, int W, int hidden) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || hidden < 1 || hidden > 1024 || C > 8192)
    return fail(MGACBAM_E_SHAPE, "mask head: bad shape B=%d C=%d H=%d W=%d hidden=%d", B, C, H, W, hidden);
  if (static_cast<long long>(H) * W > (1ll << 28) || static_cast<long long>(B) * std::max(C, hidden) * H * W > (1ll << 40))
    return fail(MGACBAM_E_SHAPE, "mask head: tensor too large B=%d C=%d H=%d W=%d", B, C, H, W);
  // the 3x3 kernels work on runs of pixels with a halo of W+1 either side (k_head_out: inside a run of at most 1024 pixels; k_head_bwd_act:
  // an LDS plane of run + halo): rows wider than that are refused here, not at launch; one sample's z block must fit a buffer descriptor
  { int ppt, opx, per;
    if (!head_out_shape(hidden, H * W, W, ppt, opx, per) || W > 500)
      return fail(MGACBAM_E_SHAPE, "mask head: image rows of W=%d do not fit the 3x3 kernels' pixel runs (W <= 500)", W);
    if (static_cast<long long>(hidden) * H * W >= (1ll << 30))
      return fail(MGACBAM_E_SHAPE, "mask head: hidden * H * W = %lld does not fit a buffer descriptor (< 2^30)", static_cast<long long>(hidden) * H * W); }
  return 0;
}
struct HeadTiling { int vec, hidp, cp, tile_px, tps, nwg, gx_tile_px, gx_tps, fw_kw, gx_kw, fw_mtw, gx_mtw, nwg_out, out_ppt, out_px, out_per, nwg1, act_ppt, act_hl, ncb, nshare, gw2; };
// wave arrangement of k_head_gemm (head.cuh): MW waves along M for `mtiles` 16-output tiles, KW waves along K when K is long (a chain of
// K/4 dependent steps otherwise), the rest along pixels
static void head_waves(int mtiles, int mtw, int K, int& pw, int& kw) {
  int mw = std::min(4, (mtiles + mtw - 1) / mtw);
  if (mw == 3) mw = 4;
  const int rest = 4 / mw;
  kw = K >= 128 ? rest : 1;
  pw = rest / kw;
}
// pixel shares of the LDS-staged dW1 forms (k_head_bwd_gw2, k_head_gw_nhwc): a share = every nshare-th 64-pixel chunk.
// kHeadGwDiv: 64-pixel chunks per workgroup (pixel shares = chunks / this).  5: the YOLOv8n pyramid's 1,008 workgroups are one resident round
// at the kernel's 108 VGPRs (4 per CU): slice 0.3886 -> 0.3852 ms; 3, 6, 8 and config 3: no difference
// (measured: 2-4 chunks per workgroup and 512-2048 shares all within 1 %; 6+ chunks, one resident round: +12 %)
constexpr int kHeadGwDiv = 5;
static int head_staged_nshare(int B, int HW, long long per_share) {
  const long long chunks64 = static_cast<long long>(B) * ((HW + kHeadGwPx - 1) / kHeadGwPx);
  const long long cap = std::max(1ll, std::min(512ll, (4ll << 20) / per_share));
  return static_cast<int>(std::max(1ll, std::min(cap, chunks64 / kHeadGwDiv)));
}
static HeadTiling head_tiling(int B, int C, int H, int W, int hidden, bool nhwc = false) {
  HeadTiling t;
  const int HW = H * W;
  t.vec = (HW % 4 == 0) ? 4 : 1;
  t.hidp = (hidden + 15) & ~15; t.cp = (C + 15) & ~15;
  int pw;
  t.fw_mtw = t.hidp / 16 > 8 ? 4 : 2;                               // forward: two accumulator tiles per wave (120 VGPRs, 4 workgroups per CU, every level of a YOLOv8n/s call in ONE launch); hidden > 128: four
  t.gx_mtw = 2;                                                     // gx: its B operand (g_a, z: E/4 each) is cheap to re-read; light workgroups
  head_waves(t.hidp / 16, t.fw_mtw, C, pw, t.fw_kw);
  t.tile_px = pw * 16 * t.vec;
  t.tps = (HW + t.tile_px - 1) / t.tile_px;
  t.nwg = B * t.tps;
  head_waves(t.cp / 16, t.gx_mtw, hidden, pw, t.gx_kw);
  t.gx_tile_px = pw * 16 * t.vec;
  t.gx_tps = (HW + t.gx_tile_px - 1) / t.gx_tile_px;
  head_out_shape(hidden, HW, W, t.out_ppt, t.out_px, t.out_per);
  t.nwg_out = B * t.out_per;
  t.act_ppt = HW >= 2048 ? 4 : (HW >= 512 ? 2 : 1);             // pixels per thread of k_head_bwd_act (amortises its per-channel reductions)
  t.nwg1 = B * ((HW + kBlock * t.act_ppt - 1) / (kBlock * t.act_ppt));
  t.act_hl = kBlock * t.act_ppt + 2 * (W + 1);
  t.ncb = (C + kHeadCB - 1) / kHeadCB;
  // pixel shares of k_head_bwd_gw: as many workgroups as ~4 MB of dW1 partials allow (32..256), and no more than there are pairs of pixel chunks
  const long long per_share = static_cast<long long>(t.ncb) * t.hidp * kHeadCB * 4;
  long long ns = (4ll << 20) / per_share;
  const long long chunks = static_cast<long long>(B) * ((HW + 4 * t.vec - 1) / (4 * t.vec));
  ns = std::min(ns, (chunks + 7) / 8);
  t.nshare = static_cast<int>(std::max(32ll, std::min(256ll, ns)));
  t.gw2 = (t.vec == 4 && t.hidp <= 64) ? 1 : 0;                     // k_head_bwd_gw2 (operands through LDS): a share = every nshare-th 64-pixel chunk
  if (t.gw2) t.nshare = head_staged_nshare(B, HW, per_share);
  if (nhwc) {
    // MGAHEAD_LAYOUT_NHWC (head_nhwc.cuh): 64 pixels per wave along N, no K split; dW1 always takes the LDS-staged form, shares as k_head_bwd_gw2's
    auto waves_px = [](int mtiles, int mtw) { int mw = std::min(4, (mtiles + mtw - 1) / mtw); if (mw == 3) mw = 4; return 4 / mw; };
    t.fw_kw = t.gx_kw = 1;
    t.tile_px = waves_px(t.hidp / 16, t.fw_mtw) * kHeadNhwcPx;
    t.tps = (HW + t.tile_px - 1) / t.tile_px;
    t.nwg = B * t.tps;
    t.gx_tile_px = waves_px(t.cp / 16, t.gx_mtw) * kHeadNhwcPx;
    t.gx_tps = (HW + t.gx_tile_px - 1) / t.gx_tile_px;
    t.nshare = head_staged_nshare(B, HW, per_share);
    t.gw2 = 0;
  }
  return t;
}
struct HeadCtxLayout { size_t z, mean, rstd, par, part, total; };
static HeadCtxLayout head_ctx_layout(int B, int C, int H, int W, int hidden, bool nhwc = false) {
  const HeadTiling t = head_tiling(B, C, H, W, hidden, nhwc);
  HeadCtxLayout L;
  Carver cv;
  L.z = cv.take(static_cast<size_t>(B) * hidden * H * W);
  L.mean = cv.take(t.hidp); L.rstd = cv.take(t.hidp);
  L.par = cv.take(static_cast<size_t>(t.hidp) * kHeadPar);
  L.part = cv.take(static_cast<size_t>(t.nwg) * 2 * t.hidp);
  L.total = cv.total;
  return L;
}
struct HeadScratchLayout { size_t ga, part1, kst, gwpart, total; };
static HeadScratchLayout head_scratch_layout(int B, int C, int H, int W, int hidden, bool nhwc = false) {
  const HeadTiling t = head_tiling(B, C, H, W, hidden, nhwc);
  HeadScratchLayout L;
  Carver cv;
  L.ga = cv.take(static_cast<size_t>(B) * hidden * H * W);
  L.part1 = cv.take(static_cast<size_t>(t.nwg1) * t.hidp * kHeadNStat);
  L.kst = cv.take(5 * static_cast<size_t>(t.hidp));
  L.gwpart = cv.take(static_cast<size_t>(t.ncb) * t.nshare * t.hidp * kHeadCB);
  L.total = cv.total;
  return L;
}
extern "C" size_t mgahead_ctx_bytes(int B, int C, int H, int W, int hidden) {
  if (head_check_shape(B, C, H, W, hidden)) return 0;
  return head_ctx_layout(B, C, H, W, hidden).total;
}
extern "C" size_t mgahead_bwd_scratch_bytes(int B, int C, int H, int W, int hidden) {
  if (head_check_shape(B, C, H, W, hidden)) return 0;
  return head_scratch_layout(B, C, H, W, hidden).total;
}
extern "C" size_t mgahead_ctx_bytes_flags(int B, int C, int H, int W, int hidden, int flags) {
  if (head_check_shape(B, C, H, W, hidden)) return 0;
  return head_ctx_layout(B, C, H, W, hidden, (flags & MGAHEAD_LAYOUT_NHWC) != 0).total;
}
extern "C" size_t mgahead_bwd_scratch_bytes_flags(int B, int C, int H, int W, int hidden, int flags) {
  if (head_check_shape(B, C, H, W, hidden)) return 0;
  return head_scratch_layout(B, C, H, W, hidden, (flags & MGAHEAD_LAYOUT_NHWC) != 0).total;
}
// What the mask head groups by (host.cuh: the signature of a family).  vec: along H*W in either layout; lf32: logits / g_logits are fp32
// whatever dtype is (MGAHEAD_LOGITS_F32); nhwc: MGAHEAD_LAYOUT_NHWC level, kernels of head_nhwc.cuh; cvec: their channels per lane access
// (4 when C % 4 == 0, else 1; 0 for an NCHW level)
struct HeadSig {
  int dtype, vec, lf32, nhwc, cvec, weight;
  bool operator==(const HeadSig& o) const { return dtype == o.dtype && vec == o.vec && lf32 == o.lf32 && nhwc == o.nhwc && cvec == o.cvec; }
};
static int head_common(const mgahead_params_t& P, int B, int C, int H, int W, int dtype, bool nhwc, void* ctx, HeadArgs& A, HeadSig& sig) {
  if (!P.w1 || !P.bn_weight || !P.bn_bias || !P.running_mean || !P.running_var || !P.wh || !P.bh)
    return fail(MGACBAM_E_NULL, "mask head: NULL parameter pointer");
  if (int e = head_check_shape(B, C, H, W, P.hidden)) return e;
  if (int e = check_dtype("mask head", dtype)) return e;
  if (!(P.eps > 0.f) || !(P.momentum >= 0.f && P.momentum <= 1.f)) return fail(MGACBAM_E_SHAPE, "mask head: eps=%g momentum=%g", P.eps, P.momentum);
  const HeadTiling t = head_tiling(B, C, H, W, P.hidden, nhwc);
  memset(&A, 0, sizeof(A));
  A.p = HeadPtrs{P.w1, P.bn_weight, P.bn_bias, P.running_mean, P.running_var, reinterpret_cast<long long*>(P.num_batches_tracked), P.wh, P.bh};
  A.g.B = B; A.g.C = C; A.g.hid = P.hidden; A.g.H = H; A.g.W = W; A.g.HW = H * W; A.g.hidp = t.hidp; A.g.cp = t.cp;
  A.g.eps = P.eps; A.g.momentum = P.momentum; A.g.training = P.training ? 1 : 0;
  const HeadCtxLayout L = head_ctx_layout(B, C, H, W, P.hidden, nhwc);
  A.c = HeadCtx{at(ctx, L.z), at(ctx, L.mean), at(ctx, L.rstd), at(ctx, L.par), at(ctx, L.part)};
  A.tile_px = t.tile_px; A.tiles_per_sample = t.tps; A.nwg = t.nwg;
  A.gx_tile_px = t.gx_tile_px; A.gx_tiles_per_sample = t.gx_tps; A.fw_kw = t.fw_kw; A.gx_kw = t.gx_kw; A.fw_mtw = t.fw_mtw; A.gx_mtw = t.gx_mtw;
  A.trace = knobs().trace; A.trace_base = 0;
  A.nwg_out = t.nwg_out; A.out_ppt = t.out_ppt; A.out_px = t.out_px; A.out_per = t.out_per; A.nwg1 = t.nwg1; A.act_ppt = t.act_ppt; A.act_hl_max = t.act_hl; A.ncb = t.ncb; A.nshare = t.nshare; A.gw2 = t.gw2;
  sig = HeadSig{};
  sig.dtype = dtype; sig.vec = t.vec; sig.nhwc = nhwc; sig.cvec = !nhwc ? 0 : C % 4 == 0 ? 4 : 1;
  sig.weight = C;
  return 0;
}
static size_t head_gemm_smem(const HeadArgs& a) { return (static_cast<size_t>(kHeadLdsX) + 8 * a.g.hidp) * sizeof(float); }
static int max_hidp(const HeadArgs* lv, int n) {
  int m = 0;
  for (int l = 0; l < n; ++l) m = std::max(m, lv[l].g.hidp);
  return m;
}
static int head_forward_group(HeadArgs* lv, int n, const HeadSig& sig, hipStream_t st) {
  Group<HeadArgs> G = make_group(lv, n);
  {
    // one launch per accumulator template (two tiles per wave: hidden <= 128, i.e. every level of the n/s models; four beyond): each level
    // alone is latency-bound, so levels that share a launch overlap each other
    const size_t smem = group_smem(G, head_gemm_smem);
    for (int pass = 0; pass < 2; ++pass) {
      Group<HeadArgs> Gm;
      Gm.n = 0;
      int grid = 0, mtw = 1;
      for (int l = 0; l < n; ++l)
        if ((lv[l].fw_mtw <= 2) == (pass == 0)) {
          Gm.lv[Gm.n] = lv[l]; Gm.start[Gm.n] = grid; grid += lv[l].nwg; ++Gm.n;
          mtw = std::max(mtw, lv[l].fw_mtw);
        }
      if (!Gm.n) continue;
      Gm.start[Gm.n] = grid;
      for (int l = 0; l < Gm.n; ++l) Gm.lv[l].trace_base = pass * 8192;
      if (sig.nhwc) {                                             // channels-last features: head_nhwc.cuh (the level's MTW is its own fw_mtw)
        const size_t nsmem = static_cast<size_t>(8) * max_hidp(lv, n) * sizeof(float);
        auto kernel = with_elem_vec(sig.dtype, sig.cvec, [&](auto t, auto cv) {
          return with_bool(mtw <= 2, [&](auto two) { return k_head_gemm_nhwc<elem_t<decltype(t)>, cv.value, two.value ? 2 : 4>; }); });
        if (int e = launch("k_head_gemm_nhwc", kernel, grid, kBlock, nsmem, st, Gm)) return e;
        continue;
      }
      for (int l = 0; l < Gm.n; ++l) {                            // the wave arrangement follows the template the level runs under
        int pw;
        head_waves(Gm.lv[l].g.hidp / 16, mtw, Gm.lv[l].g.C, pw, Gm.lv[l].fw_kw);
        if (pw * 16 * sig.vec != Gm.lv[l].tile_px) return fail(MGACBAM_E_SHAPE, "mask head: inconsistent tiling");   // (cannot happen: see head_tiling)
      }
      auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
        return with_bool(mtw <= 2, [&](auto two) { return k_head_gemm<elem_t<decltype(t)>, v.value, false, two.value ? 2 : 4>; }); });
      if (int e = launch("k_head_gemm<fwd>", kernel, grid, kBlock, smem, st, Gm)) return e;
    }
  }
  if (int e = launch_group("k_head_stats", k_head_stats, G, [](const HeadArgs& a) { return a.g.hid; }, 0, st)) return e;
  // (the kernel's element type is the LOGITS' type: z is fp32)
  auto out = with_elem(sig.lf32 ? MGACBAM_F32 : sig.dtype, [&](auto t) {
    return with_int<4, 1>(sig.vec, [&](auto v) { return k_head_out<elem_t<decltype(t)>, v.value>; }); });
  return launch_group("k_head_out", out, G, [](const HeadArgs& a) { return a.nwg_out; }, 0, st);
}
static int head_forward_level(const mgahead_fwd_level_t& L, HeadArgs& A, HeadSig& sig) {
  if (!L.x || !L.logits || !L.ctx) return fail(MGACBAM_E_NULL, "mask head forward: x / logits / ctx is NULL");
  const bool nhwc = (L.flags & MGAHEAD_LAYOUT_NHWC) != 0;
  if (int e = head_common(L.p, L.B, L.C, L.H, L.W, L.dtype, nhwc, L.ctx, A, sig)) return e;
  if (int e = check_capacity("mask head forward", "ctx", head_ctx_layout(L.B, L.C, L.H, L.W, L.p.hidden, nhwc).total, L.ctx_bytes)) return e;
  const size_t need = (nhwc ? nhwc_vec(L.C, L.dtype) : sig.vec) * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.ctx, 16)) return fail(MGACBAM_E_ALIGN, "mask head forward: x must be %zu-byte aligned, ctx 16-byte", need);
  A.x = L.x; A.logits = L.logits;
  sig.lf32 = (L.flags & MGAHEAD_LOGITS_F32) ? 1 : 0;
  return 0;
}
extern "C" int mgahead_forward(const mgahead_fwd_level_t* levels, int n_levels, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<HeadArgs, HeadSig>(levels, n_levels, false, head_forward_level,
                              [&](HeadArgs* g, int m, const HeadSig& s) { return head_forward_group(g, m, s, st); });
}
static int head_backward_group(HeadArgs* lv, int n, const HeadSig& sig, hipStream_t st) {
  int hl = 0;
  for (int l = 0; l < n; ++l) hl = std::max(hl, lv[l].act_hl_max);
  for (int l = 0; l < n; ++l) lv[l].act_hl_max = hl;            // the reduction scratch sits behind the launch's longest run
  Group<HeadArgs> G = make_group(lv, n);
  // (the kernel's element type is g_logits' type)
  auto act = with_elem(sig.lf32 ? MGACBAM_F32 : sig.dtype, [](auto t) { return k_head_bwd_act<elem_t<decltype(t)>>; });
  if (int e = launch_group("k_head_bwd_act", act, G, [](const HeadArgs& a) { return a.nwg1 * ((a.g.hid + kHeadJC - 1) / kHeadJC); },
                           (static_cast<size_t>(hl) + 16 * kHeadJC * kHeadNStat) * sizeof(float), st)) return e;
  if (int e = launch_group("k_head_bwd_fin", k_head_bwd_fin, G, [](const HeadArgs& a) { return a.g.hid; }, 0, st)) return e;
  auto gx_tiles = [](const HeadArgs& a) { return a.g.B * a.gx_tiles_per_sample; };
  if (sig.nhwc) {                                                 // channels-last features: head_nhwc.cuh
    const size_t hp = static_cast<size_t>(max_hidp(lv, n));
    auto gx = with_elem_vec(sig.dtype, sig.cvec, [](auto t, auto cv) { return k_head_gx_nhwc<elem_t<decltype(t)>, cv.value>; });
    if (int e = launch_group("k_head_gx_nhwc", gx, G, gx_tiles, 5 * hp * sizeof(float), st)) return e;
    auto gw = with_elem_vec(sig.dtype, sig.cvec, [](auto t, auto cv) { return k_head_gw_nhwc<elem_t<decltype(t)>, cv.value>; });
    if (int e = launch_group("k_head_gw_nhwc", gw, G, [](const HeadArgs& a) { return a.ncb * a.nshare; },
                             (5 * hp + 2 * static_cast<size_t>(kHeadGwPx) * kHeadGwPitch) * sizeof(float), st)) return e;
  } else {
    for (int l = 0; l < n; ++l) G.lv[l].trace_base = 16384;
    auto gx = with_elem_vec(sig.dtype, sig.vec, [](auto t, auto v) { return k_head_gemm<elem_t<decltype(t)>, v.value, true, 2>; });
    if (int e = launch_group("k_head_gemm<gx>", gx, G, gx_tiles, head_gemm_smem, st)) return e;
    // dW1 partials
    for (int pass = 0; pass < 2; ++pass) {                         // pass 0: the levels that take the LDS-staged form, pass 1: the rest
      Group<HeadArgs> Gw;
      Gw.n = 0;
      int grid = 0;
      size_t smem = 0;
      for (int l = 0; l < n; ++l)
        if ((lv[l].gw2 != 0) == (pass == 0)) {
          Gw.lv[Gw.n] = G.lv[l]; Gw.start[Gw.n] = grid; grid += lv[l].ncb * lv[l].nshare; ++Gw.n;
          const size_t hp = static_cast<size_t>(lv[l].g.hidp);
          smem = std::max(smem, (pass == 0 ? 5 * hp + (kHeadCB + hp) * kHeadGwPitch : 5 * hp + 1024) * sizeof(float));
        }
      if (!Gw.n) continue;
      Gw.start[Gw.n] = grid;
      if (pass == 0) {
        auto gw2 = with_elem(sig.dtype, [](auto t) { return k_head_bwd_gw2<elem_t<decltype(t)>>; });
        if (int e = launch("k_head_bwd_gw2", gw2, grid, kBlock, smem, st, Gw)) return e;
        continue;
      }
      auto gw = with_elem_vec(sig.dtype, sig.vec, [](auto t, auto v) { return k_head_bwd_gw<elem_t<decltype(t)>, v.value>; });
      if (int e = launch("k_head_bwd_gw", gw, grid, kBlock, smem, st, Gw)) return e;
    }
  }
  return launch_group("k_head_bwd_gwf", k_head_bwd_gwf, G,
                      [](const HeadArgs& a) { return (a.g.hid * a.g.C + kHeadGwfOut - 1) / kHeadGwfOut; }, 0, st);
}
static int head_backward_level(const mgahead_bwd_level_t& L, HeadArgs& A, HeadSig& sig) {
  if (!L.x || !L.g_logits || !L.ctx || !L.scratch || !L.gx) return fail(MGACBAM_E_NULL, "mask head backward: x / g_logits / ctx / scratch / gx is NULL");
  if (!L.gw1 || !L.gbn_weight || !L.gbn_bias || !L.gwh || !L.gbh) return fail(MGACBAM_E_NULL, "mask head backward: NULL parameter-gradient pointer");
  const bool nhwc = (L.flags & MGAHEAD_LAYOUT_NHWC) != 0;
  if (int e = head_common(L.p, L.B, L.C, L.H, L.W, L.dtype, nhwc, const_cast<void*>(L.ctx), A, sig)) return e;
  const size_t need = (nhwc ? nhwc_vec(L.C, L.dtype) : sig.vec) * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.gx, need) || !aligned_to(L.ctx, 16) || !aligned_to(L.scratch, 16))
    return fail(MGACBAM_E_ALIGN, "mask head backward: x/gx must be %zu-byte aligned, ctx/scratch 16-byte", need);
  A.x = L.x; A.gl = L.g_logits; A.gx = L.gx;
  A.gw1 = L.gw1; A.ggamma = L.gbn_weight; A.gbeta = L.gbn_bias; A.gwh = L.gwh; A.gbh = L.gbh;
  A.accum_gx = (L.flags & MGAHEAD_BWD_ACCUM_GX) ? 1 : 0;
  sig.lf32 = (L.flags & MGAHEAD_LOGITS_F32) ? 1 : 0;
  A.gl2 = L.g_logits2;
  const HeadScratchLayout SL = head_scratch_layout(L.B, L.C, L.H, L.W, L.p.hidden, nhwc);
  if (int e = check_capacity("mask head backward", "ctx", head_ctx_layout(L.B, L.C, L.H, L.W, L.p.hidden, nhwc).total, L.ctx_bytes)) return e;
  if (int e = check_capacity("mask head backward", "scratch", SL.total, L.scratch_bytes)) return e;
  A.s = HeadScratch{at(L.scratch, SL.ga), at(L.scratch, SL.part1), at(L.scratch, SL.kst), at(L.scratch, SL.gwpart)};
  return 0;
}
extern "C" int mgahead_backward(const mgahead_bwd_level_t* levels, int n_levels, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<HeadArgs, HeadSig>(levels, n_levels, false, head_backward_level,
                              [&](HeadArgs* g, int m, const HeadSig& s) { return head_backward_group(g, m, s, st); });
}
