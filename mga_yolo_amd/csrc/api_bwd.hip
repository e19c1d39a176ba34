// libmgacbam.so, C ABI (include/mgacbam.h): MaskCBAM backward (mgacbam_backward[_stages])
#include "host.cuh"
#include "bwd.cuh"
#include "nhwc_bwd.cuh"

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// One level of either layout: validated (NULL, parameters, shape, dtype, alignment, capacity), then its kernel arguments.  N.a is the
// whole result for an NCHW level; a channels-last level (sig.nhwc) also gets its chunk geometry and has no in-launch hand-off.
static int backward_args(const mgacbam_bwd_level_t& L, NhwcBwdArgs& N, Sig& sig) {
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
  BwdArgs& A = N.a;
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
  sig = Sig{L.dtype, VEC, L.mask != nullptr, L.p.k, L.gmask != nullptr, 0};
  if (nhwc) {
    N.n = nhwc_geo(L.C, L.H, L.W, VEC);
    N.ncb = (L.C + kNhwcFoldC - 1) / kNhwcFoldC;
    A.nt = N.n.nchunk;
    A.ncg = N.ncb;
    A.bflag0 = A.cflag0 = A.mbflag0 = A.mcflag0 = A.wflag0 = A.sflag0 = 0;   // (no in-launch hand-off on this path)
    sig.nhwc = 1;                                                 // (no projection planes, HAVE_PROJ is ignored: the NHWC apply reads x for dL/dmask)
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
  // sig.proj follows "gmask wanted" only: the levels of a pyramid stay ONE launch group whichever of them qualify.
  const bool have = (L.flags & MGACBAM_BWD_HAVE_PROJ) != 0;
  const bool make = !have && L.dtype == MGACBAM_F32 && reduce1_smem(A.g, VEC, true) <= 64 * 1024;
  sig.proj = L.gmask != nullptr;
  A.g.proj_h = (L.gmask && L.p.hidden <= MGACBAM_PROJ_MAX_HIDDEN && (have || make)) ? L.p.hidden : 0;
  A.make_proj = A.g.proj_h > 0 && make;
  return 0;
}

// The layout-free kernels take the plain level arguments: each launch computes its own grid and LDS size from the group
template <typename SmemOf>
static size_t group_smem(const Group<BwdArgs>& G, SmemOf smem_of) {
  size_t smem = 0;
  for (int l = 0; l < G.n; ++l) smem = std::max(smem, smem_of(G.lv[l]));
  return smem;
}
static size_t reduce2_smem(const Tune& t) { return (64 + static_cast<size_t>(std::max(kPghLds, kBlock / t.pool_tx))) * sizeof(float); }
static int launch_convT(Group<BwdArgs>& G, int k, hipStream_t st) {
  const size_t smem = group_smem(G, [&](const BwdArgs& a) { return convT_smem(a.t, k); });
  const int grid = fill_starts(G, G.lv, G.n, [](const BwdArgs& a) { return a.nconv; });
  switch (k) {
    case 3: LAUNCH(k_bwd_convT<3>, grid, smem, st, G); break;
    case 5: LAUNCH(k_bwd_convT<5>, grid, smem, st, G); break;
    case 7: LAUNCH(k_bwd_convT<7>, grid, smem, st, G); break;
    default: LAUNCH(k_bwd_convT<0>, grid, smem, st, G); break;
  }
  return launch_status("k_bwd_convT");
}
static int launch_wsa(Group<BwdArgs>& G, int k, hipStream_t st) {
  const size_t smem = group_smem(G, [&](const BwdArgs& a) { return wsa_smem(a.t, k); });
  const int grid = fill_starts(G, G.lv, G.n, [](const BwdArgs& a) { return a.nwsa; });
  switch (k) {
    case 3: LAUNCH(k_bwd_wsa<3>, grid, smem, st, G); break;
    case 5: LAUNCH(k_bwd_wsa<5>, grid, smem, st, G); break;
    case 7: LAUNCH(k_bwd_wsa<7>, grid, smem, st, G); break;
    default: LAUNCH(k_bwd_wsa<0>, grid, smem, st, G); break;
  }
  return launch_status("k_bwd_wsa");
}
static int launch_params(Group<BwdArgs>& G, hipStream_t st) {
  const size_t smem = group_smem(G, [](const BwdArgs& a) { return params_smem(a.g); });
  const int grid = fill_starts(G, G.lv, G.n, [](const BwdArgs& a) { return a.npg; });
  LAUNCH(k_bwd_params, grid, smem, st, G);
  return launch_status("k_bwd_params");
}

static int backward_group(BwdArgs* lv, int n, const Sig& sig, int stages, hipStream_t st) {
  Group<BwdArgs> G;
  G.n = n;
  // k_bwd_reduce2 re-reads three planes (g_planes x 2, cidx) per channel group: 4 channels per row halve that share of its loads
  // (config 4: 88 -> 80 us) whenever the grid still fills the chip; k_pool (one mask plane per group) measured slower with 4
  constexpr int kReduce2MaxCpt = 4;
  const int cpt = group_cpt(lv, n, kReduce2MaxCpt);
  for (int l = 0; l < n; ++l) {
    lv[l].t.pool_cpt = cpt;
    const int cpb = (kBlock / lv[l].t.pool_tx) * cpt;
    lv[l].ncg = (lv[l].g.C + cpb - 1) / cpb;
    G.lv[l] = lv[l];
  }

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
    const int grid = tot;
#define CALL_R12B(CPTV) if (mkproj) LAUNCH((k_bwd_r12<TT, VV, CPTV, true>), grid, smem, st, R); else LAUNCH((k_bwd_r12<TT, VV, CPTV, false>), grid, smem, st, R)
#define CALL_R12(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; DISPATCH_CPT(cpt, CALL_R12B); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R12);
#undef CALL_R12
#undef CALL_R12B
    if (int e = launch_status("k_bwd_r12")) return e;
    for (int l = 0; l < n; ++l) G.lv[l] = lv[l];                  // (the later launches of this call see the same level state)
  }
  if (fold && !merge) {
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max({smem, reduce1_smem(lv[l].g, sig.vec, lv[l].make_proj), convT_smem(lv[l].t, sig.k)});
    const int grid = fill_starts(G, lv, n, [&](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt) + pad8(a.nconv); });
#define CALL_R1F2(Tt, Vv, PJ) if (sig.k == 7) LAUNCH((k_bwd_reduce1_fold<Tt, Vv, 7, PJ>), grid, smem, st, G); else LAUNCH((k_bwd_reduce1_fold<Tt, Vv, 0, PJ>), grid, smem, st, G)
#define CALL_R1F(Tt, Vv) if (mkproj) { CALL_R1F2(Tt, Vv, true); } else { CALL_R1F2(Tt, Vv, false); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R1F);
#undef CALL_R1F
#undef CALL_R1F2
    if (int e = launch_status("k_bwd_reduce1_fold")) return e;
  }
  if ((stages & MGACBAM_BWD_REDUCE1) && !fold) {  // 1. per-(b,c) and per-pixel reductions of gy*x
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, reduce1_smem(lv[l].g, sig.vec, lv[l].make_proj));
    const int grid = fill_starts(G, lv, n, [&](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt); });
#define CALL_R1(Tt, Vv) if (mkproj) LAUNCH((k_bwd_reduce1<Tt, Vv, true>), grid, smem, st, G); else LAUNCH((k_bwd_reduce1<Tt, Vv, false>), grid, smem, st, G)
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R1);
#undef CALL_R1
    if (int e = launch_status("k_bwd_reduce1")) return e;
  }
  if ((stages & MGACBAM_BWD_CONVT) && !fold)  // 2. transposed conv
    if (int e = launch_convT(G, sig.k, st)) return e;
  const bool fuse_pg = fuse && (stages & MGACBAM_BWD_APPLY) && (stages & MGACBAM_BWD_PARAMGRAD);
  const bool fuse_wsa = fuse && (stages & MGACBAM_BWD_REDUCE2) && (stages & MGACBAM_BWD_WSA) && sig.k == 7;   // dWsa tile partials: leading roles of k_bwd_reduce2
  if ((stages & MGACBAM_BWD_REDUCE2) && !merge) {  // 3. rest of g_ca (needs g_planes), g_z [+ dWsa partials as role workgroups]
    size_t smem = 0;
    for (int l = 0; l < n; ++l) {
      smem = std::max(smem, reduce2_smem(lv[l].t));
      if (fuse_wsa) smem = std::max(smem, wsa_smem(lv[l].t, sig.k));
    }
    const int grid = fill_starts(G, lv, n, [&](const BwdArgs& a) { return (fuse_wsa ? pad8(a.nwsa) : 0) + sweep_blocks(a, a.t.pool_tx, cpt); });
#define CALL_R22(CPTV) if (fuse_wsa) LAUNCH((k_bwd_reduce2<TT, VV, CPTV, true>), grid, smem, st, G); else LAUNCH((k_bwd_reduce2<TT, VV, CPTV, false>), grid, smem, st, G)
#define CALL_R2(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; DISPATCH_CPT(cpt, CALL_R22); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R2);
#undef CALL_R2
#undef CALL_R22
    if (int e = launch_status("k_bwd_reduce2")) return e;
  }
  if ((stages & MGACBAM_BWD_WSA) && !fuse_wsa && !merge)  // 4. dWsa tile partials (depends on stage 1 only)
    if (int e = launch_wsa(G, sig.k, st)) return e;
  if ((stages & MGACBAM_BWD_PARAMGRAD) && !fuse_pg)  // 5. every parameter gradient
    if (int e = launch_params(G, st)) return e;
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask) [+ parameter gradients as role workgroups]
    size_t smem = 0;
    for (int l = 0; l < n; ++l) {
      smem = std::max(smem, bwd_apply_smem(lv[l].g, sig.vec));
      if (fuse_pg) smem = std::max(smem, params_smem(lv[l].g));
    }
    const int grid = fill_starts(G, lv, n, [&](const BwdArgs& a) { return (fuse_pg ? pad8(a.npg) : 0) + xcd_grid(a.g.B, a.nt); });
#define CALL_AP2(GM) if (fuse_pg) LAUNCH((k_bwd_apply<TT, VV, GM, true>), grid, smem, st, G); else LAUNCH((k_bwd_apply<TT, VV, GM, false>), grid, smem, st, G)
#define CALL_AP(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; if (sig.gmask) { CALL_AP2(true); } else { CALL_AP2(false); } }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_AP);
#undef CALL_AP
#undef CALL_AP2
    if (int e = launch_status("k_bwd_apply")) return e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// backward of channels-last levels (nhwc.cuh): k_bwd_reduce1_nhwc, k_bwd_convT, k_bwd_reduce2_nhwc + k_bwd_fold_nhwc, k_bwd_wsa,
// k_bwd_params, k_bwd_apply_nhwc -- the layout-free kernels are the NCHW path's own
// ------------------------------------------------------------------------------------------------
static int backward_group_nhwc(NhwcBwdArgs* lv, int n, const Sig& sig, int stages, hipStream_t st) {
  Group<NhwcBwdArgs> G;
  Group<BwdArgs> GB;                                            // the layout-free kernels take the plain level arguments
  G.n = GB.n = n;
  for (int l = 0; l < n; ++l) { G.lv[l] = lv[l]; GB.lv[l] = lv[l].a; }
  auto chunks = [&]() { return fill_starts(G, lv, n, [&](const NhwcBwdArgs& a) { return xcd_grid(a.a.g.B, a.n.nchunk); }); };
  if (stages & MGACBAM_BWD_REDUCE1) {  // 1. chunk partials of A and D, g_pre
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, nhwc_reduce1_smem(lv[l].a.g, sig.vec));
    const int grid = chunks();
#define CALL_NR1(Tt, Vv) LAUNCH((k_bwd_reduce1_nhwc<Tt, Vv>), grid, smem, st, G)
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NR1);
#undef CALL_NR1
    if (int e = launch_status("k_bwd_reduce1_nhwc")) return e;
  }
  if (stages & MGACBAM_BWD_CONVT)  // 2. transposed conv
    if (int e = launch_convT(GB, sig.k, st)) return e;
  if (stages & MGACBAM_BWD_REDUCE2) {  // 3. chunk partials of the g_planes term, then their fold: g_z, D, hidden-gradient partials
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, nhwc_reduce2_smem(lv[l].a.g));
    const int grid = chunks();
#define CALL_NR2(Tt, Vv) LAUNCH((k_bwd_reduce2_nhwc<Tt, Vv>), grid, smem, st, G)
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NR2);
#undef CALL_NR2
    if (int e = launch_status("k_bwd_reduce2_nhwc")) return e;
    const int fgrid = fill_starts(G, lv, n, [&](const NhwcBwdArgs& a) { return a.a.g.B * a.ncb; });
    LAUNCH(k_bwd_fold_nhwc, fgrid, 0, st, G);
    if (int e = launch_status("k_bwd_fold_nhwc")) return e;
  }
  if (stages & MGACBAM_BWD_WSA)  // 4. dWsa tile partials
    if (int e = launch_wsa(GB, sig.k, st)) return e;
  if (stages & MGACBAM_BWD_PARAMGRAD)  // 5. every parameter gradient
    if (int e = launch_params(GB, st)) return e;
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask)
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, nhwc_bwd_apply_smem(lv[l].a.g));
    const int grid = fill_starts(G, lv, n, [&](const NhwcBwdArgs& a) { return xcd_grid(a.a.g.B, a.n.ntile); });
#define CALL_NAP(Tt, Vv) if (sig.gmask) LAUNCH((k_bwd_apply_nhwc<Tt, Vv, true>), grid, smem, st, G); else LAUNCH((k_bwd_apply_nhwc<Tt, Vv, false>), grid, smem, st, G)
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NAP);
#undef CALL_NAP
    if (int e = launch_status("k_bwd_apply_nhwc")) return e;
  }
  return 0;
}

extern "C" int mgacbam_backward_stages(const mgacbam_bwd_level_t* levels, int n_levels, int stages, void* stream) {
  if (!levels) return fail(MGACBAM_E_NULL, "levels is NULL");
  if (n_levels < 1 || n_levels > MGACBAM_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "n_levels=%d", n_levels);
  hipStream_t st = static_cast<hipStream_t>(stream);
  BwdArgs args[MGACBAM_MAX_LEVELS];
  Sig sigs[MGACBAM_MAX_LEVELS];
  NhwcBwdArgs nargs[MGACBAM_MAX_LEVELS];
  Sig nsigs[MGACBAM_MAX_LEVELS];
  int nc = 0, nn = 0;                                           // NCHW levels, NHWC levels (every level is checked before any launch)
  for (int l = 0; l < n_levels; ++l) {
    NhwcBwdArgs N;
    Sig s;
    if (int e = backward_args(levels[l], N, s)) return e;
    if (s.nhwc) { nargs[nn] = N; nsigs[nn++] = s; } else { args[nc] = N.a; sigs[nc++] = s; }
  }
  if (nc) if (int e = for_each_group(args, sigs, nc, [&](BwdArgs* g, int m, const Sig& s) { return backward_group(g, m, s, stages, st); })) return e;
  if (nn) if (int e = for_each_group(nargs, nsigs, nn, [&](NhwcBwdArgs* g, int m, const Sig& s) { return backward_group_nhwc(g, m, s, stages, st); })) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgacbam_backward(const mgacbam_bwd_level_t* levels, int n_levels, void* stream) {
  return mgacbam_backward_stages(levels, n_levels, MGACBAM_BWD_ALL, stream);
}

