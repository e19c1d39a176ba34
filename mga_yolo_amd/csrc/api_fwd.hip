// libmgacbam.so, C ABI (include/mgacbam.h): MaskCBAM forward (mgacbam_forward[_stages])
#include "host.cuh"
#include "fwd.cuh"
#include "nhwc_fwd.cuh"

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// What the forward groups by (host.cuh: the signature of a family).  gvec: elements per lane of k_gate for this level -- a function of
// the LEVEL alone (dtype, shape, k, knobs), never of the levels it happens to be called with: the hand-off flags in ctx.sync count calls per
// TILE, so a ctx must see the same tiling in every call whatever the group composition (levels of different gvec go to different launches).
// proj: W1-projection planes are saved (NCHW levels); vec: along H*W, or along C for a channels-last level
struct FwdSig {
  int dtype, vec, has_mask, k, proj, gvec, nhwc, weight;
  bool operator==(const FwdSig& o) const {
    return dtype == o.dtype && vec == o.vec && has_mask == o.has_mask && k == o.k && proj == o.proj && gvec == o.gvec && nhwc == o.nhwc;
  }
};
// One level of either layout: validated (NULL, parameters, shape, dtype, alignment, capacity), then its kernel arguments; a channels-last
// level (sig.nhwc) also gets its chunk geometry and the ws buffer.
static int forward_args(const mgacbam_fwd_level_t& L, FwdArgs& A, FwdSig& sig) {
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
  A.x = L.x; A.mask = L.mask; A.y = L.y; A.fused = 0;
  level_setup(L, A);
  A.fault = knobs().fault;
  A.pool_mlp = 0;
  A.arrive0 = static_cast<int>(sync_layout(L.B, L.C, static_cast<size_t>(L.H) * L.W).arrive);
  A.n = NhwcGeo{}; A.ws = nullptr;
  sig = FwdSig{};
  sig.dtype = L.dtype; sig.vec = VEC; sig.has_mask = L.mask != nullptr; sig.k = L.p.k; sig.nhwc = nhwc;
  if (nhwc) {
    A.n = nhwc_geo(L.C, L.H, L.W, VEC);
    A.ws = static_cast<float*>(L.ws);
    const int rows = std::min((A.n.ch - 1) / L.W + 2, L.H);     // image rows a chunk of ch pixels touches
    A.t.apply_rows = rows + L.p.k - 1;
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
  A.pool_mlp = pool_forms_ca(A.g, A.t, false, L.dtype);
  return 0;
}

// k_mlp is layout-free: one workgroup per sample
static int launch_mlp(Group<FwdArgs>& G, hipStream_t st) {
  return launch_group("k_mlp", k_mlp, G, [](const FwdArgs& a) { return a.g.B; }, [](const FwdArgs& a) { return mlp_smem(a.g); }, st);
}

static int forward_group_nhwc(FwdArgs* lv, int n, const FwdSig& sig, int stages, hipStream_t st);
static int forward_group(FwdArgs* lv, int n, const FwdSig& sig, int stages, hipStream_t st) {
  if (sig.nhwc) return forward_group_nhwc(lv, n, sig, stages, st);
  const int pool_cpt = group_cpt(lv, n);
  for (int l = 0; l < n; ++l) lv[l].t.pool_cpt = pool_cpt;
  Group<FwdArgs> G = make_group(lv, n);

  // MGACBAM_FWD_FUSE: stages 2 + 3 become ONE x-resident launch (k_gate) when every level of the group is eligible
  const int gvec = sig.gvec;                   // per level (forward_args), uniform over the group by construction
  bool gate = (stages & MGACBAM_FWD_FUSE) && (stages & MGACBAM_FWD_CHAN) && (stages & MGACBAM_FWD_APPLY) && !sig.proj && gvec > 0;
  for (int l = 0; l < n && gate; ++l) gate = lv[l].t.gate_tx > 0;
  void (*gate_kernel)(GateGroup) = nullptr;
  size_t gsmem = 0;
  if (gate) {
    // residency precondition of the in-launch hand-off, from the DEVICE (CU count x occupancy of the chosen instantiation): the
    // 8*span + 1 workgroups a tile's wait spans must be co-resident; half of the budget is left to whatever else runs on the chip
    int span = 0;
    for (int l = 0; l < n; ++l) span = std::max(span, lv[l].t.gate_span);
    gsmem = group_smem(G, [&](const FwdArgs& a) { return gate_smem(a.g, a.t, gvec); });
    gate_kernel = with_elem_vec8(sig.dtype, gvec, [&](auto t, auto v) {
      return with_k7(sig.k, [&](auto k) { return k_gate<elem_t<decltype(t)>, v.value, k.value>; }); });
    gate = 2 * (8 * span + 1) <= resident_workgroups(gate_kernel, gsmem);
  }
  if (gate) for (int l = 0; l < n; ++l) { lv[l].fused = 1; G.lv[l].fused = 1; }

  // levels whose ca k_pool forms (pool_forms_ca, a rule of the level alone): a group with one takes k_pool's instantiation with the tail
  bool any_pool_mlp = false, all_pool_mlp = true;
  for (int l = 0; l < n; ++l) { any_pool_mlp |= lv[l].pool_mlp != 0; all_pool_mlp &= lv[l].pool_mlp != 0; }

  if (stages & MGACBAM_FWD_POOL) {  // 1. pooling
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_cpt(pool_cpt, [&](auto c) {
      return with_bool(sig.has_mask, [&](auto m) { return with_bool(any_pool_mlp, [&](auto ml) {
        return k_pool<elem_t<decltype(t)>, v.value, c.value, m.value, ml.value>; }); }); }); });
    if (int e = launch_group("k_pool", kernel, G, [&](const FwdArgs& a) { return sweep_blocks(a, a.t.pool_tx, pool_cpt); },
                             [](const FwdArgs& a) { return a.pool_mlp ? pool_mlp_smem(a.g) : size_t(0); }, st)) return e;
  }
  if (gate) {
    GateGroup GG;
    const int tiles = fill_starts(G, lv, n, [&](const FwdArgs& a) { return xcd_grid(a.g.B, gate_tiles(a.t, a.g.H, a.g.W, gvec)); });
    GG.g = G;
    GG.nrole = 0;
    for (int l = 0; l < n; ++l) { GG.rstart[l] = GG.nrole; GG.nrole += lv[l].pool_mlp ? 0 : lv[l].g.B; }
    GG.rstart[n] = GG.nrole;
    return launch("k_gate", gate_kernel, GG.nrole + tiles, kBlock, gsmem, st, GG);
  }
  if (stages & MGACBAM_FWD_CHAN) {  // 2. shared MLP + channel gate (prologue, or a launch of its own), channel max / mean planes
    // With C*hidden large the MLP prologue keeps every k_chan workgroup from streaming for 15-20 us; one tiny launch per step is cheaper
    bool split_mlp = false;
    for (int l = 0; l < n; ++l) split_mlp |= static_cast<long long>(lv[l].g.C) * lv[l].g.hidden >= 8192;
    if (split_mlp) if (int e = launch_mlp(G, st)) return e;
    const bool have_ca = split_mlp || all_pool_mlp;            // from k_mlp, or every level's from k_pool: no prologue (mixed groups keep it)
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) { return with_bool(sig.proj, [&](auto pj) {
      return with_bool(have_ca, [&](auto sp) { return k_chan<elem_t<decltype(t)>, v.value, pj.value, sp.value>; }); }); });
    if (int e = launch_group("k_chan", kernel, G, [&](const FwdArgs& a) { return xcd_grid(a.g.B, chan_tiles(a.t, a.g.H, a.g.W, sig.vec)); },
                             [&](const FwdArgs& a) { return chan_smem(a.g, sig.vec, sig.proj); }, st)) return e;
  }
  if (stages & MGACBAM_FWD_APPLY) {  // 3. k x k conv + spatial gate (prologue), both gates + alpha residual
    auto kernel = with_elem_vec(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_k(sig.k, [&](auto k) { return k_apply<elem_t<decltype(t)>, v.value, k.value>; }); });
    if (int e = launch_group("k_apply", kernel, G, [&](const FwdArgs& a) { return xcd_grid(a.g.B, chan_tiles(a.t, a.g.H, a.g.W, sig.vec)); },
                             [&](const FwdArgs& a) { return apply_smem(a.g, a.t, sig.vec); }, st)) return e;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// forward of channels-last levels (nhwc.cuh): k_pool_nhwc, k_pool_fin (+ shared MLP), k_chan_nhwc, k_apply_nhwc
// ------------------------------------------------------------------------------------------------
static int forward_group_nhwc(FwdArgs* lv, int n, const FwdSig& sig, int stages, hipStream_t st) {
  Group<FwdArgs> G = make_group(lv, n);
  if (stages & MGACBAM_FWD_POOL) {  // 1. chunk partials of the pooling, 2. their fold, 3. the shared MLP -> ca
    auto pool = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_bool(sig.has_mask, [&](auto m) { return k_pool_nhwc<elem_t<decltype(t)>, v.value, m.value>; }); });
    if (int e = launch_group("k_pool_nhwc", pool, G, [](const FwdArgs& a) { return xcd_grid(a.g.B, a.n.nchunk); },
                             [](const FwdArgs& a) { return lds_bytes(PoolNhwcLds(a.g)); }, st)) return e;
    auto fin = with_bool(sig.has_mask, [](auto m) { return k_pool_fin<m.value>; });
    if (int e = launch_group("k_pool_fin", fin, G, [](const FwdArgs& a) { return nhwc_fold_blocks(a.g); }, 0, st)) return e;
    if (int e = launch_mlp(G, st)) return e;
  }
  auto tiles = [](const FwdArgs& a) { return xcd_grid(a.g.B, a.n.ntile); };
  if (stages & MGACBAM_FWD_CHAN) {  // 3. channel max / mean planes
    auto kernel = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_bool(sig.has_mask, [&](auto m) { return k_chan_nhwc<elem_t<decltype(t)>, v.value, m.value>; }); });
    if (int e = launch_group("k_chan_nhwc", kernel, G, tiles, [](const FwdArgs& a) { return lds_bytes(ChanNhwcLds(a.g)); }, st)) return e;
  }
  if (stages & MGACBAM_FWD_APPLY) {  // 4. k x k conv + spatial gate (prologue), y
    auto kernel = with_elem_vec8(sig.dtype, sig.vec, [&](auto t, auto v) {
      return with_k(sig.k, [&](auto k) { return k_apply_nhwc<elem_t<decltype(t)>, v.value, k.value>; }); });
    if (int e = launch_group("k_apply_nhwc", kernel, G, tiles, [](const FwdArgs& a) { return lds_bytes(ApplyNhwcLds(a.g, a.t, a.n, a.g.k)); }, st)) return e;
  }
  return 0;
}

extern "C" int mgacbam_forward_stages(const mgacbam_fwd_level_t* levels, int n_levels, int stages, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  return run_levels<FwdArgs, FwdSig>(levels, n_levels, true, forward_args,
      [&](FwdArgs* g, int m, const FwdSig& s) { return forward_group(g, m, s, stages, st); });
}
extern "C" int mgacbam_forward(const mgacbam_fwd_level_t* levels, int n_levels, void* stream) {
  return mgacbam_forward_stages(levels, n_levels, MGACBAM_FWD_ALL, stream);
}
