// libmgacbam.so, C ABI (include/mgacbam.h): MaskCBAM backward (mgacbam_backward[_stages])
#include "host.cuh"
#include "bwd.cuh"
#include "nhwc_bwd.cuh"

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
static int backward_args(const mgacbam_bwd_level_t& L, BwdArgs& A, Sig& sig) {
  if (!L.x || !L.gy || !L.ctx || !L.scratch || !L.gx) return fail(MGACBAM_E_NULL, "backward: x / gy / ctx / scratch / gx is NULL");
  if (!L.gw1 || !L.gb1 || !L.gw2 || !L.gb2 || !L.gwsa || !L.gbeta) return fail(MGACBAM_E_NULL, "backward: NULL parameter-gradient pointer");
  if (L.gmask && !L.mask) return fail(MGACBAM_E_NULL, "backward: gmask requested but mask is NULL");
  if (int e = check_params(L.p)) return e;
  if (int e = check_shape(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k)) return e;
  if (L.dtype < MGACBAM_F32 || L.dtype > MGACBAM_BF16) return fail(MGACBAM_E_DTYPE, "backward: dtype %d", L.dtype);
  const int VEC = vec_of(L.H, L.W);
  const size_t need = VEC * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.gy, need) || !aligned_to(L.gx, need) || !aligned_to(L.ctx, 16) ||
      !aligned_to(L.scratch, 16) || (L.gmask && !aligned_to(L.gmask, 16)))
    return fail(MGACBAM_E_ALIGN, "backward: x/gy/gx must be %zu-byte aligned, ctx/scratch 16-byte", need);
  A.x = L.x; A.mask = L.mask; A.gy = L.gy; A.gx = L.gx; A.gmask = L.gmask;
  A.gw1 = L.gw1; A.gb1 = L.gb1; A.gw2 = L.gw2; A.gb2 = L.gb2; A.gwsa = L.gwsa; A.gbeta = L.gbeta;
  A.c = ctx_ptrs(const_cast<void*>(L.ctx), L.B, L.C, L.H, L.W, L.p.hidden);
  A.p = make_params(L.p);
  A.g = make_geo(L.B, L.C, L.H, L.W, L.p);
  A.t = choose_tune(L.B, L.C, L.H, L.W, L.p.k);
  const ScratchLayout SL = scratch_layout(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k);
  {
    mgacbam_ctx_layout_t CL;
    ctx_layout(L.B, L.C, L.H, L.W, L.p.hidden, &CL);
    if (int e = check_capacity("backward", "ctx", static_cast<size_t>(CL.total), L.ctx_bytes)) return e;
    if (int e = check_capacity("backward", "scratch", SL.total, L.scratch_bytes)) return e;
  }
  char* sp = static_cast<char*>(L.scratch);
  A.s.A_part = reinterpret_cast<float*>(sp + SL.A_part);
  A.s.gpre = reinterpret_cast<float*>(sp + SL.gpre); A.s.gplanes = reinterpret_cast<float*>(sp + SL.gplanes);
  A.s.gwsa_part = reinterpret_cast<float*>(sp + SL.gwsa_part);
  A.s.gz = reinterpret_cast<float*>(sp + SL.gz); A.s.gbq = reinterpret_cast<float*>(sp + SL.gbq);
  A.s.gh_avg = reinterpret_cast<float*>(sp + SL.gh_avg); A.s.gh_mx = reinterpret_cast<float*>(sp + SL.gh_mx);
  A.s.pgh = reinterpret_cast<float*>(sp + SL.pgh);
  A.nt = chan_tiles(A.t, A.g.H, A.g.W, VEC);
  A.nconv = A.g.B * conv_tiles(A.t, A.g.H, A.g.W);
  A.nwsa = A.g.B * wsa_tiles(A.t, A.g.H, A.g.W);
  A.npg = params_blocks(A.g);
  A.ncg = 0;
  A.nflag = static_cast<int>(sync_flags(static_cast<size_t>(L.H) * L.W));
  A.bflag0 = L.B * A.nflag + 4 + L.B;
  A.cflag0 = A.bflag0 + L.B * A.nflag;
  A.mbflag0 = A.cflag0 + L.B * A.nflag; A.mcflag0 = A.mbflag0 + L.B * A.nflag;
  A.wflag0 = A.mcflag0 + L.B * A.nflag; A.sflag0 = A.wflag0 + L.B * A.nflag;
  A.merged = 0;
  A.vec = VEC;
  { const Knobs kn = knobs(); A.trace = kn.trace; A.spin_limit = kn.spin_limit; }
  const int proj = (L.flags & MGACBAM_BWD_HAVE_PROJ) && L.gmask != nullptr;
  A.g.proj_h = (proj && L.p.hidden <= MGACBAM_PROJ_MAX_HIDDEN) ? L.p.hidden : 0;
  sig = Sig{L.dtype, VEC, L.mask != nullptr, L.p.k, L.gmask != nullptr, proj};
  return 0;
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
  auto fill = [&](auto blocks_of) { int tot = 0; for (int l = 0; l < n; ++l) { G.start[l] = tot; tot += blocks_of(lv[l]); } G.start[n] = tot; return tot; };

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
      smem = std::max({smem, reduce1_smem(lv[l].g, sig.vec), convT_smem(lv[l].t, sig.k), wsa_smem(lv[l].t, sig.k),
                       (64 + static_cast<size_t>(std::max(kPghLds, kBlock / lv[l].t.pool_tx))) * sizeof(float)});
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
#define CALL_R12B(CPTV) LAUNCH((k_bwd_r12<TT, VV, CPTV>), grid, smem, st, R)
#define CALL_R12(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; DISPATCH_CPT(cpt, CALL_R12B); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R12);
#undef CALL_R12
#undef CALL_R12B
    if (int e = launch_status("k_bwd_r12")) return e;
    for (int l = 0; l < n; ++l) G.lv[l] = lv[l];                  // (the later launches of this call see the same level state)
  }
  if (fold && !merge) {
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max({smem, reduce1_smem(lv[l].g, sig.vec), convT_smem(lv[l].t, sig.k)});
    const int grid = fill([&](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt) + pad8(a.nconv); });
#define CALL_R1F(Tt, Vv) if (sig.k == 7) LAUNCH((k_bwd_reduce1_fold<Tt, Vv, 7>), grid, smem, st, G); else LAUNCH((k_bwd_reduce1_fold<Tt, Vv, 0>), grid, smem, st, G)
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R1F);
#undef CALL_R1F
    if (int e = launch_status("k_bwd_reduce1_fold")) return e;
  }
  if ((stages & MGACBAM_BWD_REDUCE1) && !fold) {  // 1. per-(b,c) and per-pixel reductions of gy*x
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, reduce1_smem(lv[l].g, sig.vec));
    const int grid = fill([&](const BwdArgs& a) { return xcd_grid(a.g.B, a.nt); });
#define CALL_R1(Tt, Vv) LAUNCH((k_bwd_reduce1<Tt, Vv>), grid, smem, st, G)
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R1);
#undef CALL_R1
    if (int e = launch_status("k_bwd_reduce1")) return e;
  }
  if ((stages & MGACBAM_BWD_CONVT) && !fold) {  // 2. transposed conv
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, convT_smem(lv[l].t, sig.k));
    const int grid = fill([&](const BwdArgs& a) { return a.nconv; });
    switch (sig.k) {
      case 3: LAUNCH(k_bwd_convT<3>, grid, smem, st, G); break;
      case 5: LAUNCH(k_bwd_convT<5>, grid, smem, st, G); break;
      case 7: LAUNCH(k_bwd_convT<7>, grid, smem, st, G); break;
      default: LAUNCH(k_bwd_convT<0>, grid, smem, st, G); break;
    }
    if (int e = launch_status("k_bwd_convT")) return e;
  }
  const bool fuse_pg = fuse && (stages & MGACBAM_BWD_APPLY) && (stages & MGACBAM_BWD_PARAMGRAD);
  const bool fuse_wsa = fuse && (stages & MGACBAM_BWD_REDUCE2) && (stages & MGACBAM_BWD_WSA) && sig.k == 7;   // dWsa tile partials: leading roles of k_bwd_reduce2
  if ((stages & MGACBAM_BWD_REDUCE2) && !merge) {  // 3. rest of g_ca (needs g_planes), g_z [+ dWsa partials as role workgroups]
    size_t smem = 0;
    for (int l = 0; l < n; ++l) {
      smem = std::max(smem, (64 + static_cast<size_t>(std::max(kPghLds, kBlock / lv[l].t.pool_tx))) * sizeof(float));
      if (fuse_wsa) smem = std::max(smem, wsa_smem(lv[l].t, sig.k));
    }
    const int grid = fill([&](const BwdArgs& a) { return (fuse_wsa ? pad8(a.nwsa) : 0) + sweep_blocks(a, a.t.pool_tx, cpt); });
#define CALL_R22(CPTV) if (fuse_wsa) LAUNCH((k_bwd_reduce2<TT, VV, CPTV, true>), grid, smem, st, G); else LAUNCH((k_bwd_reduce2<TT, VV, CPTV, false>), grid, smem, st, G)
#define CALL_R2(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; DISPATCH_CPT(cpt, CALL_R22); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_R2);
#undef CALL_R2
#undef CALL_R22
    if (int e = launch_status("k_bwd_reduce2")) return e;
  }
  if ((stages & MGACBAM_BWD_WSA) && !fuse_wsa && !merge) {  // 4. dWsa tile partials (depends on stage 1 only)
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, wsa_smem(lv[l].t, sig.k));
    const int grid = fill([&](const BwdArgs& a) { return a.nwsa; });
    switch (sig.k) {
      case 3: LAUNCH(k_bwd_wsa<3>, grid, smem, st, G); break;
      case 5: LAUNCH(k_bwd_wsa<5>, grid, smem, st, G); break;
      case 7: LAUNCH(k_bwd_wsa<7>, grid, smem, st, G); break;
      default: LAUNCH(k_bwd_wsa<0>, grid, smem, st, G); break;
    }
    if (int e = launch_status("k_bwd_wsa")) return e;
  }
  if ((stages & MGACBAM_BWD_PARAMGRAD) && !fuse_pg) {  // 5. every parameter gradient
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, params_smem(lv[l].g));
    const int grid = fill([&](const BwdArgs& a) { return a.npg; });
    LAUNCH(k_bwd_params, grid, smem, st, G);
    if (int e = launch_status("k_bwd_params")) return e;
  }
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask) [+ parameter gradients as role workgroups]
    size_t smem = 0;
    for (int l = 0; l < n; ++l) {
      smem = std::max(smem, bwd_apply_smem(lv[l].g, sig.vec));
      if (fuse_pg) smem = std::max(smem, params_smem(lv[l].g));
    }
    const int grid = fill([&](const BwdArgs& a) { return (fuse_pg ? pad8(a.npg) : 0) + xcd_grid(a.g.B, a.nt); });
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
namespace mgacbam {
inline int level_weight(const NhwcBwdArgs& a, int) { return a.a.g.C; }   // (found by for_each_group through ADL)
}

static int nhwc_backward_args(const mgacbam_bwd_level_t& L, NhwcBwdArgs& N, Sig& sig) {
  if (!L.x || !L.gy || !L.ctx || !L.scratch || !L.gx) return fail(MGACBAM_E_NULL, "backward: x / gy / ctx / scratch / gx is NULL");
  if (!L.gw1 || !L.gb1 || !L.gw2 || !L.gb2 || !L.gwsa || !L.gbeta) return fail(MGACBAM_E_NULL, "backward: NULL parameter-gradient pointer");
  if (L.gmask && !L.mask) return fail(MGACBAM_E_NULL, "backward: gmask requested but mask is NULL");
  if (int e = check_params(L.p)) return e;
  if (int e = check_shape(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k)) return e;
  if (L.dtype < MGACBAM_F32 || L.dtype > MGACBAM_BF16) return fail(MGACBAM_E_DTYPE, "backward: dtype %d", L.dtype);
  const int VEC = nhwc_vec(L.C, L.dtype);
  const size_t need = VEC * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.gy, need) || !aligned_to(L.gx, need) || !aligned_to(L.ctx, 16) ||
      !aligned_to(L.scratch, 16) || (L.gmask && !aligned_to(L.gmask, 4)) || (L.mask && !aligned_to(L.mask, 4)))
    return fail(MGACBAM_E_ALIGN, "backward (NHWC): x/gy/gx must be %zu-byte aligned, ctx/scratch 16-byte", need);
  const ScratchLayout SL = nhwc_scratch_layout(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k, VEC);
  {
    mgacbam_ctx_layout_t CL;
    ctx_layout(L.B, L.C, L.H, L.W, L.p.hidden, &CL);
    if (int e = check_capacity("backward", "ctx", static_cast<size_t>(CL.total), L.ctx_bytes)) return e;
    if (int e = check_capacity("backward", "scratch", SL.total, L.scratch_bytes)) return e;
  }
  BwdArgs& A = N.a;
  A.x = L.x; A.mask = L.mask; A.gy = L.gy; A.gx = L.gx; A.gmask = L.gmask;
  A.gw1 = L.gw1; A.gb1 = L.gb1; A.gw2 = L.gw2; A.gb2 = L.gb2; A.gwsa = L.gwsa; A.gbeta = L.gbeta;
  A.c = ctx_ptrs(const_cast<void*>(L.ctx), L.B, L.C, L.H, L.W, L.p.hidden);
  A.p = make_params(L.p);
  A.g = make_geo(L.B, L.C, L.H, L.W, L.p);
  A.t = choose_tune(L.B, L.C, L.H, L.W, L.p.k);
  char* sp = static_cast<char*>(L.scratch);
  A.s.A_part = reinterpret_cast<float*>(sp + SL.A_part);
  A.s.gpre = reinterpret_cast<float*>(sp + SL.gpre); A.s.gplanes = reinterpret_cast<float*>(sp + SL.gplanes);
  A.s.gwsa_part = reinterpret_cast<float*>(sp + SL.gwsa_part);
  A.s.gz = reinterpret_cast<float*>(sp + SL.gz); A.s.gbq = reinterpret_cast<float*>(sp + SL.gbq);
  A.s.gh_avg = reinterpret_cast<float*>(sp + SL.gh_avg); A.s.gh_mx = reinterpret_cast<float*>(sp + SL.gh_mx);
  A.s.pgh = reinterpret_cast<float*>(sp + SL.pgh);
  N.n = nhwc_geo(L.C, L.H, L.W, VEC);
  N.ncb = (L.C + kNhwcFoldC - 1) / kNhwcFoldC;
  A.nt = N.n.nchunk;
  A.nconv = A.g.B * conv_tiles(A.t, A.g.H, A.g.W);
  A.nwsa = A.g.B * wsa_tiles(A.t, A.g.H, A.g.W);
  A.npg = params_blocks(A.g);
  A.ncg = N.ncb;
  A.nflag = static_cast<int>(sync_flags(static_cast<size_t>(L.H) * L.W));
  A.bflag0 = A.cflag0 = A.mbflag0 = A.mcflag0 = A.wflag0 = A.sflag0 = 0;   // (no in-launch hand-off on this path)
  A.merged = 0;
  A.vec = VEC;
  { const Knobs kn = knobs(); A.trace = kn.trace; A.spin_limit = kn.spin_limit; }
  A.g.proj_h = 0;                                               // (HAVE_PROJ is ignored: the NHWC apply reads x for dL/dmask)
  sig = Sig{L.dtype, VEC, L.mask != nullptr, L.p.k, L.gmask != nullptr, 0};
  sig.nhwc = 1;
  return 0;
}

static int backward_group_nhwc(NhwcBwdArgs* lv, int n, const Sig& sig, int stages, hipStream_t st) {
  Group<NhwcBwdArgs> G;
  Group<BwdArgs> GB;                                            // the layout-free kernels take the plain level arguments
  G.n = GB.n = n;
  for (int l = 0; l < n; ++l) { G.lv[l] = lv[l]; GB.lv[l] = lv[l].a; }
  auto fill = [&](auto blocks_of) { int tot = 0; for (int l = 0; l < n; ++l) { G.start[l] = tot; tot += blocks_of(lv[l]); } G.start[n] = tot; return tot; };
  auto fillb = [&](auto blocks_of) { int tot = 0; for (int l = 0; l < n; ++l) { GB.start[l] = tot; tot += blocks_of(lv[l].a); } GB.start[n] = tot; return tot; };
  auto chunks = [&]() { return fill([&](const NhwcBwdArgs& a) { return xcd_grid(a.a.g.B, a.n.nchunk); }); };
  if (stages & MGACBAM_BWD_REDUCE1) {  // 1. chunk partials of A and D, g_pre
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, (3 * ((static_cast<size_t>(lv[l].a.g.C) + 3) & ~static_cast<size_t>(3)) + 2 * kBlock * sig.vec) * sizeof(float));
    const int grid = chunks();
#define CALL_NR1(Tt, Vv) LAUNCH((k_bwd_reduce1_nhwc<Tt, Vv>), grid, smem, st, G)
    DISPATCH_T_NVEC(sig.dtype, sig.vec, CALL_NR1);
#undef CALL_NR1
    if (int e = launch_status("k_bwd_reduce1_nhwc")) return e;
  }
  if (stages & MGACBAM_BWD_CONVT) {  // 2. transposed conv
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, convT_smem(lv[l].a.t, sig.k));
    const int grid = fillb([&](const BwdArgs& a) { return a.nconv; });
    switch (sig.k) {
      case 3: LAUNCH(k_bwd_convT<3>, grid, smem, st, GB); break;
      case 5: LAUNCH(k_bwd_convT<5>, grid, smem, st, GB); break;
      case 7: LAUNCH(k_bwd_convT<7>, grid, smem, st, GB); break;
      default: LAUNCH(k_bwd_convT<0>, grid, smem, st, GB); break;
    }
    if (int e = launch_status("k_bwd_convT")) return e;
  }
  if (stages & MGACBAM_BWD_REDUCE2) {  // 3. chunk partials of the g_planes term, then their fold: g_z, D, hidden-gradient partials
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, static_cast<size_t>(lv[l].a.g.C) * sizeof(float));
    const int grid = chunks();
#define CALL_NR2(Tt, Vv) LAUNCH((k_bwd_reduce2_nhwc<Tt, Vv>), grid, smem, st, G)
    DISPATCH_T_NVEC(sig.dtype, sig.vec, CALL_NR2);
#undef CALL_NR2
    if (int e = launch_status("k_bwd_reduce2_nhwc")) return e;
    const int fgrid = fill([&](const NhwcBwdArgs& a) { return a.a.g.B * a.ncb; });
    LAUNCH(k_bwd_fold_nhwc, fgrid, 0, st, G);
    if (int e = launch_status("k_bwd_fold_nhwc")) return e;
  }
  if (stages & MGACBAM_BWD_WSA) {  // 4. dWsa tile partials
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, wsa_smem(lv[l].a.t, sig.k));
    const int grid = fillb([&](const BwdArgs& a) { return a.nwsa; });
    switch (sig.k) {
      case 3: LAUNCH(k_bwd_wsa<3>, grid, smem, st, GB); break;
      case 5: LAUNCH(k_bwd_wsa<5>, grid, smem, st, GB); break;
      case 7: LAUNCH(k_bwd_wsa<7>, grid, smem, st, GB); break;
      default: LAUNCH(k_bwd_wsa<0>, grid, smem, st, GB); break;
    }
    if (int e = launch_status("k_bwd_wsa")) return e;
  }
  if (stages & MGACBAM_BWD_PARAMGRAD) {  // 5. every parameter gradient
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, params_smem(lv[l].a.g));
    const int grid = fillb([&](const BwdArgs& a) { return a.npg; });
    LAUNCH(k_bwd_params, grid, smem, st, GB);
    if (int e = launch_status("k_bwd_params")) return e;
  }
  if (stages & MGACBAM_BWD_APPLY) {  // 6. gx (+ gmask)
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, (5 * static_cast<size_t>(lv[l].a.g.C) + 2 * lv[l].a.g.hidden) * sizeof(float));
    const int grid = fill([&](const NhwcBwdArgs& a) { return xcd_grid(a.a.g.B, a.n.ntile); });
#define CALL_NAP(Tt, Vv) if (sig.gmask) LAUNCH((k_bwd_apply_nhwc<Tt, Vv, true>), grid, smem, st, G); else LAUNCH((k_bwd_apply_nhwc<Tt, Vv, false>), grid, smem, st, G)
    DISPATCH_T_NVEC(sig.dtype, sig.vec, CALL_NAP);
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
    if (levels[l].flags & MGACBAM_LAYOUT_NHWC) { if (int e = nhwc_backward_args(levels[l], nargs[nn], nsigs[nn])) return e; ++nn; }
    else { if (int e = backward_args(levels[l], args[nc], sigs[nc])) return e; ++nc; }
  }
  if (nc) if (int e = for_each_group(args, sigs, nc, [&](BwdArgs* g, int m, const Sig& s) { return backward_group(g, m, s, stages, st); })) return e;
  if (nn) if (int e = for_each_group(nargs, nsigs, nn, [&](NhwcBwdArgs* g, int m, const Sig& s) { return backward_group_nhwc(g, m, s, stages, st); })) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgacbam_backward(const mgacbam_bwd_level_t* levels, int n_levels, void* stream) {
  return mgacbam_backward_stages(levels, n_levels, MGACBAM_BWD_ALL, stream);
}

