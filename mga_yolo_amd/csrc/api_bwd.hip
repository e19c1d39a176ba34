// libmgacbam.so, C ABI (include/mgacbam.h): MaskCBAM backward (mgacbam_backward[_stages])
#include "host.cuh"
#include "bwd.cuh"
#include "nhwc_bwd.cuh"

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// What the backward groups by (host.cuh: the signature of a family).  gmask: dL/dmask is wanted; vec: along H*W, or along C for a
// channels-last level.  Whether a level has W1-projection planes is NOT here: the levels of a pyramid stay one launch group whichever qualify.
struct BwdSig {
  int dtype, vec, has_mask, k, gmask, nhwc, weight;
  bool operator==(const BwdSig& o) const {
    return dtype == o.dtype && vec == o.vec && has_mask == o.has_mask && k == o.k && gmask == o.gmask && nhwc == o.nhwc;
  }
};
// One level of either layout: validated (NULL, parameters, shape, dtype, alignment, capacity), then its kernel arguments; a channels-last
// level (sig.nhwc) also gets its chunk geometry and has no in-launch hand-off.
static int backward_args(const mgacbam_bwd_level_t& L, BwdArgs& A, BwdSig& sig) {
  const bool nhwc = (L.flags & MGACBAM_LAYOUT_NHWC) != 0;
  if (!L.x || !L.gy || !L.ctx || !L.scratch || !L.gx) return fail(MGACBAM_E_NULL, "backward: x / gy / ctx / scratch / gx is NULL");
  if (!L.gw1 || !L.gb1 || !L.gw2 || !L.gb2 || !L.gwsa || !L.gbeta) return fail(MGACBAM_E_NULL, "backward: NULL parameter-gradient pointer");
  if (L.gmask && !L.mask) return fail(MGACBAM_E_NULL, "backward: gmask requested but mask is NULL");
  if (int e = check_level("backward", L)) return e;
  const int VEC = level_vec(nhwc, L.C, L.H, L.W, L.dtype);
  const size_t need = VEC * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.gy, need) || !aligned_to(L.gx, need) || !aligned_to(L.ctx, 16) ||
      !aligned_to(L.scratch, 16) || (L.gmask && !aligned_to(L.gmask, nhwc ? 4 : 16)) || (nhwc && L.mask && !aligned_to(L.mask, 4)))
    return fail(MGACBAM_E_ALIGN, "backward%s: x/gy/gx must be %zu-byte aligned, ctx/scratch 16-byte", nhwc ? " (NHWC)" : "", need);
  const ScratchLayout SL = scratch_layout(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k, nhwc, VEC);
  if (int e = check_ctx_capacity("backward", L)) return e;
  if (int e = check_capacity("backward", "scratch", SL.total, L.scratch_bytes)) return e;
  A.x = L.x; A.mask = L.mask; A.gy = L.gy; A.gx = L.gx; A.gmask = L.gmask;
  A.gw1 = L.gw1; A.gb1 = L.gb1; A.gw2 = L.gw2; A.gb2 = L.gb2; A.gwsa = L.gwsa; A.gbeta = L.gbeta;
  level_setup(L, A);
  A.s = scratch_ptrs(L.scratch, SL);
  A.nconv = A.g.B * conv_tiles(A.t, A.g.H, A.g.W);
  A.nwsa = A.g.B * wsa_tiles(A.t, A.g.H, A.g.W);
  A.npg = params_blocks(A.g);
  A.merged = 0;
  A.make_proj = 0;
  A.vec = VEC;
  A.n = NhwcGeo{}; A.ncb = 0;
  sig = BwdSig{};
  sig.dtype = L.dtype; sig.vec = VEC; sig.has_mask = L.mask != nullptr; sig.k = L.p.k; sig.gmask = L.gmask != nullptr; sig.nhwc = nhwc;
  if (nhwc) {                                                     // (no projection planes, HAVE_PROJ is ignored: the NHWC apply reads x for dL/dmask)
    A.n = nhwc_geo(L.C, L.H, L.W, VEC);
    A.ncb = (L.C + kNhwcFoldC - 1) / kNhwcFoldC;
    A.nt = A.n.nchunk;
    A.ncg = A.ncb;
    A.bflag0 = A.cflag0 = A.mbflag0 = A.mcflag0 = A.wflag0 = A.sflag0 = 0;   // (no in-launch hand-off on this path)
    sig.weight = L.C;
    return 0;
  }
  A.nt = chan_tiles(A.t, A.g.H, A.g.W, VEC);
  A.ncg = 0;                                                      // (set per group: backward_group)
  const SyncLayout S = sync_layout(L.B, L.C, static_cast<size_t>(L.H) * L.W);
  A.bflag0 = static_cast<int>(S.bflag); A.cflag0 = static_cast<int>(S.cflag);
  A.mbflag0 = static_cast<int>(S.mbflag); A.mcflag0 = static_cast<int>(S.mcflag);
  A.wflag0 = static_cast<int>(S.wflag); A.sflag0 = static_cast<int>(S.sflag);
  sig.weight = L.C * A.t.chan_tx;
  // dL/dmask from the W1-projection planes (bwd.cuh): a property of the LEVEL alone -- gmask wanted (which implies a mask), a hidden
  // width the ctx has planes for, and either planes the caller's forward saved (MGACBAM_BWD_HAVE_PROJ) or an fp32 level, whose
  // k_bwd_reduce1 tiles then write them -- so a call that runs REDUCE1 and a later call that runs APPLY on the same ctx agree, whatever
  // other levels share either call.  fp32 only: at config 2 with bf16 / fp16 features the tiles lose more than k_bwd_apply gains
  // (step 0.1382 -> 0.1396 ms and 0.1519 -> 0.1547 ms, three interleaved pairs each), so those levels keep reading x.
  // (W1^T of the level must fit beside the tiles' combine buffer in the LDS every launch may ask for: C up to ~1,700.)
  // The signature follows "gmask wanted" only: the levels of a pyramid stay ONE launch group whichever of them qualify.
  const bool have = (L.flags & MGACBAM_BWD_HAVE_PROJ) != 0;
  const bool make = !have && L.dtype == MGACBAM_F32 && reduce1_smem(A.g, VEC, true) <= 64 * 1024;
  A.g.proj_h = (L.gmask && L.p.hidden <= MGACBAM_PROJ_MAX_HIDDEN && (have || make)) ? L.p.hidden : 0;
  A.make_proj = A.g.proj_h > 0 && make;
  // kProjMax < hidden <= kProjWide: the tiles form the planes on the matrix cores (bwd.cuh) into the SCRATCH buffer -- made and used inside
  // one backward, the ctx has no room for them -- whether or not HAVE_PROJ is set (the forward never saves planes this wide).  Again the
  // level alone decides (wide_proj_shape: the lane layout the MFMA needs and a level too large to stay in the cache).
  if (L.gmask && L.dtype == MGACBAM_F32 && wide_proj_shape(L.B, L.C, L.H, L.W, L.p.hidden, false, VEC, A.t)) {
    A.g.proj_h = L.p.hidden;
    A.make_proj = 2;
    A.c.proj = A.s.proj;                                          // k_bwd_apply reads a level's planes through c.proj wherever they live
  }
  return 0;
}

// The layout-free kernels: each launch computes its own grid and LDS size from the group
static size_t reduce2_smem(const Tune& t) { return (64 + static_cast<size_t>(std::max(kPghLds, kBlock / t.pool_tx))) * sizeof(float); }
static int launch_convT(Group<BwdArgs>& G, int k, hipStream_t st) {
  auto kernel = with_k(k, [](auto kk) { return k_bwd_convT<kk.value>; });
  return launch_group("k_bwd_convT", kernel, G, [](const BwdArgs& a) { return a.nconv; }, [&](const BwdArgs& a) { return convT_smem(a.t, k); }, st);
}
static int launch_wsa(Group<BwdArgs>& G, int k, hipStream_t st) {
  auto kernel = with_k(k, [](auto kk) { return k_bwd_wsa<kk.value>; });
  return launch_group("k_bwd_wsa", kernel, G, [](const BwdArgs& a) { return a.nwsa; }, [&](const BwdArgs& a) { return wsa_smem(a.t, k); }, st);
}
static int launch_params(Group<BwdArgs>& G, hipStream_t st) {
  return launch_group("k_bwd_params", k_bwd_params, G, [](const BwdArgs& a) { return a.npg; }, [](const BwdArgs& a) { return params_smem(a.g); }, st);
}

static int backward_group_nhwc(BwdArgs* lv, int n, const BwdSig& sig, int stages, hipStream_t st);
static int backward_group(BwdArgs* lv, int n, const BwdSig& sig, int stages, hipStream_t st) {
  if (sig.nhwc) return backward_group_nhwc(lv, n, sig, stages, st);
  // k_bwd_reduce2 re-reads three planes (g_planes x 2, cidx) per channel group: 4 channels per row halve that share of its loads
  // (config 4: 88 -> 80 us) whenever the grid still fills the chip; k_pool (one mask plane per group) measured slower with 4
  constexpr int kReduce2MaxCpt = 4;
  const int cpt = group_cpt(lv, n, kReduce2MaxCpt);
  for (int l = 0; l < n; ++l) {
    lv[l].t.pool_cpt = cpt;
    const int cpb = (kBlock / lv[l].t.pool_tx) * cpt;
    lv[l].ncg = (lv[l].g.C + cpb - 1) / cpb;
  }
  Group<BwdArgs> G = make_group(lv, n);

  // MGACBAM_BWD_FOLD: transposed conv as trailing role workgroups of the k_bwd_reduce1 launch (whole backward in this call, a tile at
  // least one image row and at least kSyncPx pixels -- one flag per tile in ctx.sync -- and few tiles per conv window)
  // (the conv tiles are the LAST workgroups of the launch and wait only for lower-numbered producers, which never wait themselves:
  //  progress does not depend on residency; the span bound is a speed heuristic)
  bool fold = (stages & MGACBAM_BWD_FOLD) && (stages & MGACBAM_BWD_REDUCE1) && (stages & MGACBAM_BWD_CONVT);
  for (int l = 0; l < n && fold; ++l) {
    const int TP = lv[l].t.chan_tx * sig.vec;
    fold = TP >= kSyncPx && TP >= lv[l].g.W && 8 * (((lv[l].t.conv_th + lv[l].g.k) * lv[l].g.W + TP - 1) / TP + 1) <= 512 &&
           lv[l].nconv <= lv[l].g.B * lv[l].nflag;                 // one flag per conv tile fits the region reserved in ctx.sync
  }
  // the plane-making instantiation of the tile kernels only where some level of the group makes planes: every other group runs the
  // kernels it ran before the planes moved into the backward
  bool mkproj = false;
  for (int l = 0; l < n; ++l) mkproj = mkproj || lv[l].make_proj;
  // k_bwd_r12: the folded launch AND k_bwd_reduce2 with its dWsa roles as one launch (bwd.cuh), when both stages are in this call
  const bool fuse = (stages & MGACBAM_BWD_FUSE) != 0;
  bool merge = fold && fuse && (stages & MGACBAM_BWD_REDUCE2) && (stages & MGACBAM_BWD_WSA) && sig.k == 7 && knobs().bwd_merge;
  for (int l = 0; l < n && merge; ++l) merge = lv[l].nwsa <= lv[l].g.B * lv[l].nflag && lv[l].ncg <= lv[l].g.C && lv[l].nconv % lv[l].g.B == 0;
  if (merge) {
    R12Group R;
    R.g.n = n;
    size_t smem = 0;
    for (int l = 0; l < n; ++l) {
      lv[l].merged = 1; lv[l].bflag0 = lv[l].mbflag0; lv[l].cflag0 = lv[l].mcflag0;
      R.g.lv[l] = lv[l];
      smem = std::max({smem, reduce1_smem(lv[l].g, sig.vec, lv[l].make_proj), convT_smem(lv[l].t, sig.k), wsa_smem(lv[l].t, sig.k),
                       reduce2_smem(lv[l].t)});
    }
    int tot = 0;
    for (int p = 0; p < 4; ++p) {
      for (int l = 0; l < n; ++l) {
        R.seg[p][l] = tot;
        tot += p == 0 ? xcd_grid(lv[l].g.B, lv[l].nt) : p == 1 ? pad8(lv[l].nconv) : p == 2 ? pad8(lv[l].nwsa) : sweep_blocks(lv[l], lv[l].t.pool_tx, cpt);
      }
      R.seg[p][n] = tot;
    }
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_cpt(cpt, [&](auto c) {
      return with_bool(mkproj, [&](auto pj) { return k_bwd_r12<elem_t<decltype(t)>, v.value, c.value, pj.value>; }); }); });
    if (int e = launch("k_bwd_r12", kernel, tot, kBlock, smem, st, R)) return e;
    for (int l = 0; l < n; ++l) G.lv[l] = lv[l];                  // (the later launches of this call see the same level state)
  }
  if (fold && !merge) {
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_k7(sig.k, [&](auto k) {
      return with_bool(mkproj, [&](auto pj) { return k_bwd_reduce1_fold<elem_t<decltype(t)>, v.value, k.value, pj.value>; }); }); });
    if (int e = launch_group("k_bwd_reduce1_fold", kernel, G, [](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt) + pad8(a.nconv); },
                             [&](const BwdArgs& a) { return std::max(reduce1_smem(a.g, sig.vec, a.make_proj), convT_smem(a.t, sig.k)); },
                             st)) return e;
  }
  if ((stages & MGACBAM_BWD_REDUCE1) && !fold) {  // 1. per-(b,c) and per-pixel reductions of gy*x
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_bool(mkproj, [&](auto pj) { return k_bwd_reduce1<elem_t<decltype(t)>, v.value, pj.value>; }); });
    if (int e = launch_group("k_bwd_reduce1", kernel, G, [](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt); },
                             [&](const BwdArgs& a) { return reduce1_smem(a.g, sig.vec, a.make_proj); }, st)) return e;
  }
  if ((stages & MGACBAM_BWD_CONVT) && !fold)  // 2. transposed conv
    if (int e = launch_convT(G, sig.k, st)) return e;
  const bool fuse_pg = fuse && (stages & MGACBAM_BWD_APPLY) && (stages & MGACBAM_BWD_PARAMGRAD);
  const bool fuse_wsa = fuse && (stages & MGACBAM_BWD_REDUCE2) && (stages & MGACBAM_BWD_WSA) && sig.k == 7;   // dWsa tile partials: leading roles of k_bwd_reduce2
  if ((stages & MGACBAM_BWD_REDUCE2) && !merge) {  // 3. rest of g_ca (needs g_planes), g_z [+ dWsa partials as role workgroups]
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_cpt(cpt, [&](auto c) {
      return with_bool(fuse_wsa, [&](auto fw) { return k_bwd_reduce2<elem_t<decltype(t)>, v.value, c.value, fw.value>; }); }); });
    if (int e = launch_group("k_bwd_reduce2", kernel, G,
                             [&](const BwdArgs& a) { return (fuse_wsa ? pad8(a.nwsa) : 0) + sweep_blocks(a, a.t.pool_tx, cpt); },
                             [&](const BwdArgs& a) { return std::max(reduce2_smem(a.t), fuse_wsa ? wsa_smem(a.t, sig.k) : 0); }, st)) return e;
  }
  if ((stages & MGACBAM_BWD_WSA) && !fuse_wsa && !merge)  // 4. dWsa tile partials (depends on stage 1 only)
    if (int e = launch_wsa(G, sig.k, st)) return e;
  if ((stages & MGACBAM_BWD_PARAMGRAD) && !fuse_pg)  // 5. every parameter gradient
    if (int e = launch_params(G, st)) return e;
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask) [+ parameter gradients as role workgroups]
    // A group whose fp32 levels ALL have planes runs the instantiation that cannot read x (fewer registers, one more workgroup per CU);
    // a level's results are the same bits under either, so this is a property of the launch, not of the level (it is not in BwdSig: a
    // mixed pyramid stays one launch).  Half-precision groups keep the one instantiation they had.
    bool nox = sig.gmask && sig.dtype == MGACBAM_F32 && sig.vec == 4;
    for (int l = 0; l < n; ++l) nox = nox && lv[l].g.proj_h > 0;
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_bool(sig.gmask, [&](auto gm) {
      return with_bool(fuse_pg, [&](auto pg) {
        using T = elem_t<decltype(t)>;
        if constexpr (std::is_same_v<T, float> && v.value == 4 && gm.value) {
          return nox ? k_bwd_apply<T, v.value, gm.value, pg.value, false> : k_bwd_apply<T, v.value, gm.value, pg.value, true>;
        } else {
          return k_bwd_apply<T, v.value, gm.value, pg.value, true>;
        } }); }); });
    if (int e = launch_group("k_bwd_apply", kernel, G, [&](const BwdArgs& a) { return (fuse_pg ? pad8(a.npg) : 0) + xcd_grid(a.g.B, a.nt); },
                             [&](const BwdArgs& a) { return std::max(bwd_apply_smem(a.g, sig.vec), fuse_pg ? params_smem(a.g) : 0); }, st)) return e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// backward of channels-last levels (nhwc.cuh): k_bwd_reduce1_nhwc, k_bwd_convT, k_bwd_reduce2_nhwc + k_bwd_fold_nhwc, k_bwd_wsa,
// k_bwd_params, k_bwd_apply_nhwc -- the layout-free kernels are the NCHW path's own
// ------------------------------------------------------------------------------------------------
static int backward_group_nhwc(BwdArgs* lv, int n, const BwdSig& sig, int stages, hipStream_t st) {
  Group<BwdArgs> G = make_group(lv, n);
  auto chunks = [](const BwdArgs& a) { return xcd_grid(a.g.B, a.n.nchunk); };
  if (stages & MGACBAM_BWD_REDUCE1) {  // 1. chunk partials of A and D, g_pre
    auto kernel = with_elem_vec8(sig.dtype, sig.vec, [](auto t, auto v) { return k_bwd_reduce1_nhwc<elem_t<decltype(t)>, v.value>; });
    if (int e = launch_group("k_bwd_reduce1_nhwc", kernel, G, chunks,
                             [&](const BwdArgs& a) { return lds_bytes(Reduce1NhwcLds(a.g, sig.vec)); }, st)) return e;
  }
  if (stages & MGACBAM_BWD_CONVT)  // 2. transposed conv
    if (int e = launch_convT(G, sig.k, st)) return e;
  if (stages & MGACBAM_BWD_REDUCE2) {  // 3. chunk partials of the g_planes term, then their fold: g_z, D, hidden-gradient partials
    auto kernel = with_elem_vec8(sig.dtype, sig.vec, [](auto t, auto v) { return k_bwd_reduce2_nhwc<elem_t<decltype(t)>, v.value>; });
    if (int e = launch_group("k_bwd_reduce2_nhwc", kernel, G, chunks, [](const BwdArgs& a) { return lds_bytes(Reduce2NhwcLds(a.g)); }, st)) return e;
    if (int e = launch_group("k_bwd_fold_nhwc", k_bwd_fold_nhwc, G, [](const BwdArgs& a) { return a.g.B * a.ncb; }, 0, st)) return e;
  }
  if (stages & MGACBAM_BWD_WSA)  // 4. dWsa tile partials
    if (int e = launch_wsa(G, sig.k, st)) return e;
  if (stages & MGACBAM_BWD_PARAMGRAD)  // 5. every parameter gradient
    if (int e = launch_params(G, st)) return e;
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask)
    auto kernel = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_bool(sig.gmask, [&](auto gm) { return k_bwd_apply_nhwc<elem_t<decltype(t)>, v.value, gm.value>; }); });
    if (int e = launch_group("k_bwd_apply_nhwc", kernel, G, [](const BwdArgs& a) { return xcd_grid(a.g.B, a.n.ntile); },
                             [](const BwdArgs& a) { return lds_bytes(BwdApplyNhwcLds(a.g)); }, st)) return e;
  }
  return 0;
}

extern "C" int mgacbam_backward_stages(const mgacbam_bwd_level_t* levels, int n_levels, int stages, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<BwdArgs, BwdSig>(levels, n_levels, true, backward_args,
      [&](BwdArgs* g, int m, const BwdSig& s) { return backward_group(g, m, s, stages, st); });
}
extern "C" int mgacbam_backward(const mgacbam_bwd_level_t* levels, int n_levels, void* stream) {
  return mgacbam_backward_stages(levels, n_levels, MGACBAM_BWD_ALL, stream);
}
