// libmgacbam.so, C ABI (include/mgacbam.h): MaskCBAM forward (mgacbam_forward[_stages])
#include "host.cuh"
#include "fwd.cuh"
#include "nhwc_fwd.cuh"

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// One level of either layout: validated (NULL, parameters, shape, dtype, alignment, capacity), then its kernel arguments.  N.a is the
// whole result for an NCHW level; a channels-last level (sig.nhwc) also gets its chunk geometry and the ws buffer.
static int forward_args(const mgacbam_fwd_level_t& L, NhwcFwdArgs& N, Sig& sig) {
  const bool nhwc = (L.flags & MGACBAM_LAYOUT_NHWC) != 0;
  if (!L.x || !L.y || !L.ctx || (nhwc && !L.ws))
    return fail(MGACBAM_E_NULL, nhwc ? "forward (NHWC): x / y / ctx / ws is NULL" : "forward: x / y / ctx is NULL");
  if (int e = check_level("forward", L)) return e;
  const int VEC = level_vec(nhwc, L.C, L.H, L.W, L.dtype);
  const size_t need = VEC * elem_size(L.dtype);
  if (!aligned_to(L.x, need) || !aligned_to(L.y, need) || !aligned_to(L.ctx, 16) || (nhwc && !aligned_to(L.ws, 16)) ||
      (L.mask && !aligned_to(L.mask, nhwc ? 4 : 16)))
    return fail(MGACBAM_E_ALIGN, "forward%s: x/y must be %zu-byte aligned, ctx%s 16-byte, mask %d-byte", nhwc ? " (NHWC)" : "", need,
                nhwc ? " / ws" : "", nhwc ? 4 : VEC * 4);
  if (int e = check_ctx_capacity("forward", L)) return e;
  if (nhwc) if (int e = check_capacity("forward", "ws", nhwc_ws_bytes(L.B, L.C, L.H, L.W, VEC), L.ws_bytes)) return e;
  FwdArgs& A = N.a;
  A.x = L.x; A.mask = L.mask; A.y = L.y; A.fused = 0;
  level_setup(L, A);
  A.fault = knobs().fault;
  sig = Sig{L.dtype, VEC, L.mask != nullptr, L.p.k, 0, 0};
  if (nhwc) {
    N.n = nhwc_geo(L.C, L.H, L.W, VEC);
    N.ws = static_cast<float*>(L.ws);
    const int rows = std::min((N.n.ch - 1) / L.W + 2, L.H);     // image rows a chunk of ch pixels touches
    A.t.apply_rows = rows + L.p.k - 1;
    sig.nhwc = 1;
    sig.weight = L.C;
    return 0;
  }
  sig.weight = L.C * A.t.chan_tx;
  sig.proj = (L.flags & MGACBAM_FWD_SAVE_PROJ) && L.mask != nullptr;
  A.g.proj_h = (sig.proj && L.p.hidden <= MGACBAM_PROJ_MAX_HIDDEN) ? L.p.hidden : 0;
  // fp16 / bf16: k_gate reads 16 bytes per lane (8 elements, kept packed in the registers) whatever vector width the other kernels
  // use -- twice the pixels per tile, half the workgroups: at YOLOv8n sizes the grid then runs as ONE resident round
  sig.gvec = VEC;
  if (L.dtype != MGACBAM_F32 && VEC == 4 && (static_cast<long long>(L.H) * L.W) % 8 == 0) {
    Tune t8 = A.t;
    gate_geometry(L.C, L.H, L.W, L.p.k, 8, t8);
    if (t8.gate_tx > 0) { sig.gvec = 8; A.t = t8; }
  }
  return 0;
}

// k_mlp is layout-free: one workgroup per sample, the plain level arguments
static int launch_mlp(Group<FwdArgs>& G, hipStream_t st) {
  size_t smem = 0;
  for (int l = 0; l < G.n; ++l) smem = std::max(smem, mlp_smem(G.lv[l].g));
  const int grid = fill_starts(G, G.lv, G.n, [](const FwdArgs& a) { return a.g.B; });
  LAUNCH(k_mlp, grid, smem, st, G);
  return launch_status("k_mlp");
}

static int forward_group(FwdArgs* lv, int n, const Sig& sig, int stages, hipStream_t st) {
  Group<FwdArgs> G;
  G.n = n;
  const int pool_cpt = group_cpt(lv, n);
  for (int l = 0; l < n; ++l) { lv[l].t.pool_cpt = pool_cpt; G.lv[l] = lv[l]; }

  // MGACBAM_FWD_FUSE: stages 2 + 3 become ONE x-resident launch (k_gate) when every level of the group is eligible
  const int gvec = sig.gvec;                   // per level (forward_args), uniform over the group by construction
  bool gate = (stages & MGACBAM_FWD_FUSE) && (stages & MGACBAM_FWD_CHAN) && (stages & MGACBAM_FWD_APPLY) && !sig.proj && gvec > 0;
  for (int l = 0; l < n && gate; ++l) gate = lv[l].t.gate_tx > 0;
  size_t gsmem = 0;
  if (gate) {
    // residency precondition of the in-launch hand-off, from the DEVICE (CU count x occupancy of the chosen instantiation): the
    // 8*span + 1 workgroups a tile's wait spans must be co-resident; half of the budget is left to whatever else runs on the chip
    int span = 0;
    for (int l = 0; l < n; ++l) { gsmem = std::max(gsmem, gate_smem(lv[l].g, lv[l].t, gvec)); span = std::max(span, lv[l].t.gate_span); }
    int resident = 0;
#define RES_GATE(Tt, Vv) resident = (sig.k == 7) ? resident_workgroups(k_gate<Tt, Vv, 7>, gsmem) : resident_workgroups(k_gate<Tt, Vv, 0>, gsmem)
    DISPATCH_T_VEC8(sig.dtype, gvec, RES_GATE);
#undef RES_GATE
    gate = 2 * (8 * span + 1) <= resident;
  }
  if (gate) for (int l = 0; l < n; ++l) { lv[l].fused = 1; G.lv[l].fused = 1; }

  if (stages & MGACBAM_FWD_POOL) {  // 1. pooling
    const int grid = fill_starts(G, lv, n, [&](const FwdArgs& a) { return sweep_blocks(a, a.t.pool_tx, pool_cpt); });
#define CALL_POOL2(CPTV) if (sig.has_mask) LAUNCH((k_pool<TT, VV, CPTV, true>), grid, 0, st, G); else LAUNCH((k_pool<TT, VV, CPTV, false>), grid, 0, st, G)
#define CALL_POOL(Tt, Vv) { using TT = Tt; constexpr int VV = Vv; DISPATCH_CPT(pool_cpt, CALL_POOL2); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_POOL);
#undef CALL_POOL
#undef CALL_POOL2
    if (int e = launch_status("k_pool")) return e;
  }
  if (gate) {
    const size_t smem = gsmem;
    GateGroup GG;
    const int tiles = fill_starts(G, lv, n, [&](const FwdArgs& a) { return xcd_grid(a.g.B, gate_tiles(a.t, a.g.H, a.g.W, gvec)); });
    GG.g = G;
    GG.nrole = 0;
    for (int l = 0; l < n; ++l) { GG.rstart[l] = GG.nrole; GG.nrole += lv[l].g.B; }
    GG.rstart[n] = GG.nrole;
    const int grid = GG.nrole + tiles;
#define CALL_GATE(Tt, Vv) if (sig.k == 7) LAUNCH((k_gate<Tt, Vv, 7>), grid, smem, st, GG); else LAUNCH((k_gate<Tt, Vv, 0>), grid, smem, st, GG)
    DISPATCH_T_VEC8(sig.dtype, gvec, CALL_GATE);
#undef CALL_GATE
    return launch_status("k_gate");
  }
  if (stages & MGACBAM_FWD_CHAN) {  // 2. shared MLP + channel gate (prologue, or a launch of its own), channel max / mean planes
    // With C*hidden large the MLP prologue keeps every k_chan workgroup from streaming for 15-20 us; one tiny launch per step is cheaper
    bool split_mlp = false;
    for (int l = 0; l < n; ++l) split_mlp |= static_cast<long long>(lv[l].g.C) * lv[l].g.hidden >= 8192;
    if (split_mlp) if (int e = launch_mlp(G, st)) return e;
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, chan_smem(lv[l].g, sig.vec, sig.proj));
    const int grid = fill_starts(G, lv, n, [&](const FwdArgs& a) { return xcd_grid(a.g.B, chan_tiles(a.t, a.g.H, a.g.W, sig.vec)); });
#define CALL_CHAN(Tt, Vv)                                                                                         \
    if (split_mlp) { if (sig.proj) LAUNCH((k_chan<Tt, Vv, true, true>), grid, smem, st, G); else LAUNCH((k_chan<Tt, Vv, false, true>), grid, smem, st, G); } \
    else { if (sig.proj) LAUNCH((k_chan<Tt, Vv, true>), grid, smem, st, G); else LAUNCH((k_chan<Tt, Vv, false>), grid, smem, st, G); }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_CHAN);
#undef CALL_CHAN
    if (int e = launch_status("k_chan")) return e;
  }
  if (stages & MGACBAM_FWD_APPLY) {  // 3. k x k conv + spatial gate (prologue), both gates + alpha residual
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, apply_smem(lv[l].g, lv[l].t, sig.vec));
    const int grid = fill_starts(G, lv, n, [&](const FwdArgs& a) { return xcd_grid(a.g.B, chan_tiles(a.t, a.g.H, a.g.W, sig.vec)); });
#define CALL_APPLY(Tt, Vv)                                                    \
    switch (sig.k) {                                                          \
      case 3: LAUNCH((k_apply<Tt, Vv, 3>), grid, smem, st, G); break;         \
      case 5: LAUNCH((k_apply<Tt, Vv, 5>), grid, smem, st, G); break;         \
      case 7: LAUNCH((k_apply<Tt, Vv, 7>), grid, smem, st, G); break;         \
      default: LAUNCH((k_apply<Tt, Vv, 0>), grid, smem, st, G); break;        \
    }
    DISPATCH_T_VEC(sig.dtype, sig.vec, CALL_APPLY);
#undef CALL_APPLY
    if (int e = launch_status("k_apply")) return e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// forward of channels-last levels (nhwc.cuh): k_pool_nhwc, k_pool_fin (+ shared MLP), k_chan_nhwc, k_apply_nhwc
// ------------------------------------------------------------------------------------------------
static int forward_group_nhwc(NhwcFwdArgs* lv, int n, const Sig& sig, int stages, hipStream_t st) {
  Group<NhwcFwdArgs> G;
  G.n = n;
  for (int l = 0; l < n; ++l) G.lv[l] = lv[l];
  if (stages & MGACBAM_FWD_POOL) {  // 1. chunk partials of the pooling, 2. their fold, 3. the shared MLP -> ca
    size_t psmem = 0;
    for (int l = 0; l < n; ++l) psmem = std::max(psmem, nhwc_pool_smem(lv[l].a.g));
    const int chunk_grid = fill_starts(G, lv, n, [&](const NhwcFwdArgs& a) { return xcd_grid(a.a.g.B, a.n.nchunk); });
#define CALL_NPOOL(Tt, Vv) if (sig.has_mask) LAUNCH((k_pool_nhwc<Tt, Vv, true>), chunk_grid, psmem, st, G); else LAUNCH((k_pool_nhwc<Tt, Vv, false>), chunk_grid, psmem, st, G)
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NPOOL);
#undef CALL_NPOOL
    if (int e = launch_status("k_pool_nhwc")) return e;
    const int fgrid = fill_starts(G, lv, n, [&](const NhwcFwdArgs& a) { return a.a.g.B * ((a.a.g.C + kNhwcFoldC - 1) / kNhwcFoldC); });
    if (sig.has_mask) LAUNCH(k_pool_fin<true>, fgrid, 0, st, G); else LAUNCH(k_pool_fin<false>, fgrid, 0, st, G);
    if (int e = launch_status("k_pool_fin")) return e;
    Group<FwdArgs> GM;
    GM.n = n;
    for (int l = 0; l < n; ++l) GM.lv[l] = lv[l].a;
    if (int e = launch_mlp(GM, st)) return e;
  }
  const int cgrid = fill_starts(G, lv, n, [&](const NhwcFwdArgs& a) { return xcd_grid(a.a.g.B, a.n.ntile); });
  if (stages & MGACBAM_FWD_CHAN) {  // 3. channel max / mean planes
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, nhwc_chan_smem(lv[l].a.g));
#define CALL_NCHAN(Tt, Vv) if (sig.has_mask) LAUNCH((k_chan_nhwc<Tt, Vv, true>), cgrid, smem, st, G); else LAUNCH((k_chan_nhwc<Tt, Vv, false>), cgrid, smem, st, G)
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NCHAN);
#undef CALL_NCHAN
    if (int e = launch_status("k_chan_nhwc")) return e;
  }
  if (stages & MGACBAM_FWD_APPLY) {  // 4. k x k conv + spatial gate (prologue), y
    size_t smem = 0;
    for (int l = 0; l < n; ++l) smem = std::max(smem, nhwc_apply_smem(lv[l].a.g, lv[l].a.t, lv[l].n));
#define CALL_NAPPLY(Tt, Vv)                                                        \
    switch (sig.k) {                                                               \
      case 3: LAUNCH((k_apply_nhwc<Tt, Vv, 3>), cgrid, smem, st, G); break;        \
      case 5: LAUNCH((k_apply_nhwc<Tt, Vv, 5>), cgrid, smem, st, G); break;        \
      case 7: LAUNCH((k_apply_nhwc<Tt, Vv, 7>), cgrid, smem, st, G); break;        \
      default: LAUNCH((k_apply_nhwc<Tt, Vv, 0>), cgrid, smem, st, G); break;       \
    }
    DISPATCH_T_VEC8(sig.dtype, sig.vec, CALL_NAPPLY);
#undef CALL_NAPPLY
    if (int e = launch_status("k_apply_nhwc")) return e;
  }
  return 0;
}

extern "C" int mgacbam_forward_stages(const mgacbam_fwd_level_t* levels, int n_levels, int stages, void* stream) {
  if (!levels) return fail(MGACBAM_E_NULL, "levels is NULL");
  if (n_levels < 1 || n_levels > MGACBAM_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "n_levels=%d", n_levels);
  hipStream_t st = static_cast<hipStream_t>(stream);
  FwdArgs args[MGACBAM_MAX_LEVELS];
  Sig sigs[MGACBAM_MAX_LEVELS];
  NhwcFwdArgs nargs[MGACBAM_MAX_LEVELS];
  Sig nsigs[MGACBAM_MAX_LEVELS];
  int nc = 0, nn = 0;                                           // NCHW levels, NHWC levels (every level is checked before any launch)
  for (int l = 0; l < n_levels; ++l) {
    NhwcFwdArgs N;
    Sig s;
    if (int e = forward_args(levels[l], N, s)) return e;
    if (s.nhwc) { nargs[nn] = N; nsigs[nn++] = s; } else { args[nc] = N.a; sigs[nc++] = s; }
  }
  if (nc) if (int e = for_each_group(args, sigs, nc, [&](FwdArgs* g, int m, const Sig& s) { return forward_group(g, m, s, stages, st); })) return e;
  if (nn) if (int e = for_each_group(nargs, nsigs, nn, [&](NhwcFwdArgs* g, int m, const Sig& s) { return forward_group_nhwc(g, m, s, stages, st); })) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgacbam_forward(const mgacbam_fwd_level_t* levels, int n_levels, void* stream) {
  return mgacbam_forward_stages(levels, n_levels, MGACBAM_FWD_ALL, stream);
}

