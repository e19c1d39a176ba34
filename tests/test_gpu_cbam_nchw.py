"""GPU tests (-m gpu) of MaskCBAM on NCHW features (csrc/fwd.cuh, csrc/bwd.cuh), the block the benchmark times: every row of
tests/cbam_nchw_rows.py -- one per launch form of api_fwd.hip / api_bwd.hip -- against the fp64 oracle element by element, outputs and saved
statistics; the launch form that really ran, read from the hand-off counters in ctx.sync; the forced forms on a few small rows; a
half-precision mask.  tests/test_abi_cbam_nchw.py checks on the CPU that the rows reach the forms their comments state.

Bars.  fp32 outputs (every output of an fp32 row; dL/dmask, the parameter gradients and the saved statistics of a half row, whose inputs are
exactly representable and whose sums are accumulated in fp32): 1e-4 of the tensor's scale, 1e-3 element-wise on y / gx / gmask and the
feature-sized statistics, parameter gradients within 1e-4 max|want| + 1e-7 |gy| |x|.  Outputs stored in half (y, gx of a half row):
per element |got - want| <= u |want| + the fp32 element bar, u one rounding to nearest (2^-11 fp16, 2^-8 bf16), plus 2^-25 for fp16
subnormals.  Indices (valid, amax on valid channels, cidx) are exact outside the near-ties row_case lists."""
import pytest
import torch

from cbam_nchw_rows import ENV_ROWS, GRADS, KNOB_ROWS, NCHW_ROWS, ROW_IDS, cbam_nchw_geo, oracle64, row_case
from conftest import elem_err, rel_err

pytestmark = pytest.mark.gpu
U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUBNORMAL = {"f16": 2.0 ** -25, "bf16": 0.0}
PGRADS = ("gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta")


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


def _cfg(F, c):
    return F.BlockConfig(hidden=c.hidden, k=c.k, use_sigmoid_mask=c.use_sig, tiny_thr=c.tiny_thr, eps=c.eps)


def _params_dev(c, grad=False):
    return [t.cuda().requires_grad_(grad) for t in (c.p.w1, c.p.b1, c.p.w2, c.p.b2, c.p.wsa, c.p.beta)]


def _run(F, c, mask=None):
    """The autograd path: F.mask_cbam + backward -> (y, grads).  mask: another mask than the row's (the half-precision mask test)."""
    mask = c.mask if mask is None else mask
    x = c.x.cuda().to(c.dtype).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(c.mask_grad)
    ps = _params_dev(c, True)
    y = F.mask_cbam(x, md, *ps, _cfg(F, c))
    y.backward(c.gy.cuda().to(c.dtype))
    torch.cuda.synchronize()
    g = dict(gx=x.grad, gmask=md.grad if (md is not None and c.mask_grad) else None, **{k: p.grad for k, p in zip(PGRADS, ps)})
    assert y.dtype == c.dtype and g["gx"].dtype == c.dtype and y.shape == c.x.shape == g["gx"].shape and y.is_contiguous()
    assert (g["gmask"] is None) == (mask is None or not c.mask_grad)
    if g["gmask"] is not None:
        assert g["gmask"].shape == mask.shape and g["gmask"].dtype == mask.dtype
    for k, want in zip(PGRADS, (c.p.w1, c.p.b1, c.p.w2, c.p.b2, c.p.wsa, c.p.beta)):
        assert g[k].dtype == torch.float32 and g[k].shape == want.shape, k
    return y.detach(), g


def _bar32(want):
    """The fp32 bar per element: 1e-4 of the scale and 1e-3 of the element itself (floored at 1e-3 of the scale), whichever is smaller."""
    w = want.abs()
    scale = w.max().clamp_min(1e-30)
    return torch.minimum(1e-3 * w.clamp_min(1e-3 * scale), 1e-4 * scale)


class _Report:
    """Collects worst error / bar per output of a row, prints them, and fails with every miss."""

    def __init__(self, name):
        self.name, self.lines, self.bad, self.worst = name, [], [], 0.0

    def add(self, key, ratio, detail):
        self.worst = max(self.worst, ratio)
        self.lines.append(f"{key} {ratio:.3f}")
        if not ratio < 1.0:
            self.bad.append(f"{key}: {detail}")

    def scale32(self, key, got, want):
        e = rel_err(got, want)
        self.add(key, e / 1e-4, f"rel_err {e:.3e} over 1e-4")

    def elem32(self, key, got, want):
        e, ee = rel_err(got, want), elem_err(got, want)
        self.add(key, max(e / 1e-4, ee / 1e-3), f"rel_err {e:.3e} over 1e-4, element-wise {ee:.3e} over 1e-3")

    def half(self, key, dt, got, want):
        got, want = got.detach().double().cpu(), want.double()
        bar = U[dt] * want.abs() + _bar32(want) + SUBNORMAL[dt]
        r = ((got - want).abs() / bar)
        i = int(r.argmax())
        self.add(key, float(r.max()), f"|diff| {float((got - want).abs().reshape(-1)[i]):.3e} over {float(bar.reshape(-1)[i]):.3e} "
                 f"at want {float(want.reshape(-1)[i]):.3e}")

    def param(self, key, got, want, floor):
        want = want.double()
        d = float((got.detach().double().cpu() - want).abs().max())
        bar = 1e-4 * float(want.abs().max()) + floor
        self.add(key, d / bar, f"|diff| {d:.3e} over {bar:.3e}")

    def exact(self, key, got, want, keep=None):
        ne = got.cpu().long() != want.long()
        if keep is not None:
            ne &= keep
        self.add(key, float(int(ne.sum())), f"{int(ne.sum())} mismatching indices")

    def done(self):
        print(f"{self.name}: worst error / bar {self.worst:.3f} | " + ", ".join(self.lines))
        assert not self.bad, f"{self.name}: " + "; ".join(self.bad)


def _check_outputs(rep, c, y, g, y_o=None, g_o=None, mask_dt=None, skip_px=None):
    y_o, g_o = (c.y_o, c.g_o) if y_o is None else (y_o, g_o)
    B, H, W = c.B, c.H, c.W
    keep = (~(c.skip_px if skip_px is None else skip_px)).reshape(B, 1, H, W).double()
    gx_got, gx_want = g["gx"].detach().double().cpu() * keep, g_o["gx"].double() * keep
    if c.dt == "f32":
        rep.elem32("y", y, y_o)
        rep.elem32("gx", gx_got, gx_want)
    else:
        rep.half("y", c.dt, y, y_o)
        rep.half("gx", c.dt, gx_got, gx_want)
    if g["gmask"] is not None:
        gmask = g["gmask"].reshape(g_o["gmask"].shape)                # (a plan holds (B,1,H,W) whatever shape the row's mask has)
        if mask_dt is None:
            rep.elem32("gmask", gmask, g_o["gmask"])
        else:
            rep.half("gmask", mask_dt, gmask, g_o["gmask"])
    floor = 1e-7 * float(c.gy.double().norm() * c.x.double().norm())
    for k in PGRADS:
        rep.param(k, g[k], g_o[k], floor)


def _check_stats(rep, c, v, tag, proj):
    """The saved statistics of a forward (views into its ctx) against the oracle's intermediates, all at the fp32 bars."""
    o, B, C, HW = c.c, c.B, c.C, c.H * c.W
    if c.mask is not None:
        for k in ("S", "use", "den", "mavg"):
            rep.scale32(f"{tag}{k}", v[k], getattr(o, k))
    for k in ("avg", "mx", "h_avg", "h_mx", "ca"):
        rep.scale32(f"{tag}{k}", v[k], getattr(o, k))
    rep.exact(f"{tag}valid", v["valid"], o.valid.long())
    rep.exact(f"{tag}amax", v["amax"], o.amax, keep=o.valid & ~c.skip_ch)
    rep.exact(f"{tag}cidx", v["cidx"], o.cidx, keep=~c.skip_px)
    rep.elem32(f"{tag}planes", v["planes"], o.planes.reshape(B, 3, HW))
    rep.elem32(f"{tag}sa", v["sa"], o.sa)
    if proj:
        rep.elem32(f"{tag}proj", v["proj"], torch.einsum("jc,bcn->bjn", c.p.w1.double(), c.x.double().reshape(B, C, HW)))


# ---------------------------------------------------------------------------------------------------------------------------
# a. every row against its oracle, element-wise: outputs and saved statistics
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_IDS)
def test_cbam_nchw_row_vs_oracle(F, name):
    """Outputs: the autograd path, in the form the row is named for.  Saved statistics: F.forward_with_ctx, which asks a masked row for its
    W1-projection planes (SAVE_PROJ) and so runs the THREE-LAUNCH forward whatever the row's form -- k_pool without its tail, k_mlp or
    k_chan's prologue, k_chan (the only producer of `proj` in the forward), k_apply; a row without a mask runs its own form here.  The
    statistics k_gate and k_pool's tail save are held in test (b), from the plan's ctx."""
    c = row_case(name)
    rep = _Report(name)
    y, g = _run(F, c)
    _check_outputs(rep, c, y, g)
    y2, v = F.forward_with_ctx(c.x.cuda().to(c.dtype), None if c.mask is None else c.mask.cuda(), _params_dev(c), _cfg(F, c))
    torch.cuda.synchronize()
    _check_stats(rep, c, v, "ctx.", proj=c.mask is not None and "proj" in v)
    if c.dt == "f32":
        rep.elem32("y (stages)", y2, c.y_o)
    else:
        rep.half("y (stages)", c.dt, y2, c.y_o)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------
# b. the form that ran
# ---------------------------------------------------------------------------------------------------------------------------
def _plan(F, c, **kw):
    from mga_yolo_amd.plan import PyramidPlan
    plan = PyramidPlan([(c.B, c.C, c.H, c.W)], [[t for t in (c.p.w1, c.p.b1, c.p.w2, c.p.b2, c.p.wsa, c.p.beta)]], [_cfg(F, c)], dtype=c.dtype,
                       with_mask=c.mask is not None, want_gmask=c.mask is not None and c.mask_grad, **kw)
    plan.x[0].copy_(c.x.cuda().to(c.dtype))
    plan.gy[0].copy_(c.gy.cuda().to(c.dtype))
    if c.mask is not None:
        plan.mask[0].copy_(c.mask.cuda().reshape(c.B, 1, c.H, c.W))
    return plan


def _plan_out(plan):
    torch.cuda.synchronize()
    g = dict(gx=plan.gx[0].clone(), gmask=None if plan.gmask[0] is None else plan.gmask[0].clone(),
             **{k: t.clone() for k, t in zip(PGRADS, plan.param_grads[0])})
    return plan.y[0].clone(), g


def _assert_same_bits(what, a, b):
    (ya, ga), (yb, gb) = a, b
    assert torch.equal(ya, yb), f"{what}: y"
    for k in GRADS:
        if ga[k] is None or gb[k] is None:
            assert ga[k] is None and gb[k] is None, (what, k)
            continue
        assert torch.equal(ga[k].reshape(-1), gb[k].reshape(-1)), f"{what}: {k} differs in {int((ga[k].reshape(-1) != gb[k].reshape(-1)).sum())} elements"


def _assert_counters(name, plan, c, g, steps):
    """The hand-off counters of the plan's ctx after `steps` forward + backward calls against the restated geometry g: every class of
    counters is bumped once per launch of its kind, by the workgroups that launch has, so they say which form ran and with which tiling."""
    from mga_yolo_amd import _lib
    B, C, nflag = c.B, c.C, g["nflag"]
    sync = plan.ctx_view(0)["sync"].cpu()
    r = {k: sync[s] for k, s in _lib.sync_slices(c.B, c.C, c.H, c.W).items()}
    assert int(r["status"].abs().sum()) == 0, f"{name}: a hand-off timed out"
    assert int(r["arrive"].abs().sum()) == 0, f"{name}: k_pool left an arrival word behind"

    def per_sample(region, n):                   # (B, nflag): the first n flags of every sample read `steps`, the others 0
        want = torch.zeros(B, nflag, dtype=torch.int32)
        want[:, :n] = steps
        return torch.equal(r[region].reshape(B, nflag), want)

    def leading(region, n):                      # a flat region: its first n words read `steps`, the others 0
        want = torch.zeros_like(r[region])
        want[:n] = steps
        return torch.equal(r[region], want)

    gt = g["gtiles"] if g["gate"] else 0
    assert per_sample("gate", gt), f"{name}: k_gate flags: want {gt} tiles per sample at {steps}, got {r['gate'].reshape(B, nflag)[0, :gt + 2].tolist()}"
    mt, ft = (g["tiles"] if g["merge"] else 0), (g["tiles"] if g["fold"] and not g["merge"] else 0)
    mc, fc = (B * g["conv_tiles"] if g["merge"] else 0), (B * g["conv_tiles"] if g["fold"] and not g["merge"] else 0)
    assert per_sample("merged_tiles", mt), f"{name}: merged tile flags, want {mt} per sample"
    assert leading("merged_conv_tiles", mc), f"{name}: merged conv-tile flags, want {mc}"
    assert leading("wsa_tiles", B * g["wsa_tiles"] if g["merge"] else 0), f"{name}: dWsa-tile flags"
    assert bool((r["sweeps"] == (steps if g["merge"] else 0)).all()), f"{name}: sweep flags"
    assert per_sample("tiles", ft), f"{name}: folded tile flags, want {ft} per sample"
    assert leading("conv_tiles", fc), f"{name}: folded conv-tile flags, want {fc}"


def _form_test(F, c, g, name):
    plan = _plan(F, c)
    for _ in range(2):
        plan.forward()
        plan.backward()
    out = _plan_out(plan)
    # whether k_gate runs also depends on the device: 2 * (8 * span + 1) workgroups must be co-resident.  A device that says no breaks the
    # row's premise, and that is a failure of the row, not a reason to skip it
    assert plan.gate_active() == g["gate"], f"{name}: k_gate {'did not run' if g['gate'] else 'ran'} on this device (span {g['span']})"
    _assert_counters(name, plan, c, g, 2)
    rep = _Report(f"{name} (plan)")
    _check_outputs(rep, c, *out)
    _check_stats(rep, c, plan.ctx_view(0), "ctx.", proj=False)
    _check_backward_planes(rep, c, g, plan)
    rep.done()
    return out


def _check_backward_planes(rep, c, g, plan):
    """The W1-projection planes the backward makes, where the restated rule says it makes them, and only there.  VALU form (make_proj 1):
    into ctx.proj, which a plan zero-fills and whose forward (no SAVE_PROJ) never writes.  MFMA form (make_proj 2): into the last region of
    the scratch buffer.  Element-wise against W1 x in fp64 at the fp32 bars."""
    if c.mask is None:
        return
    B, C, HW = c.B, c.C, c.H * c.W
    want = torch.einsum("jc,bcn->bjn", c.p.w1.double(), c.x.double().reshape(B, C, HW))
    v = plan.ctx_view(0)
    if "proj" in v:
        if g["make_proj"] == 1:
            rep.elem32("bwd planes (VALU)", v["proj"], want)
        else:
            rep.add("bwd planes (none)", float(int((v["proj"] != 0).sum())), "ctx.proj was written although the rule makes no planes")
    if g["make_proj"] == 2:
        n = B * c.hidden * HW * 4                                     # (a multiple of 16 bytes: vec 4)
        got = plan.scratch[0][-n:].view(torch.float32).reshape(B, c.hidden, HW)
        rep.elem32("bwd planes (MFMA)", got, want)


@pytest.mark.parametrize("name", ROW_IDS)
def test_cbam_nchw_row_runs_the_form_it_is_there_for(F, name):
    """The row as a one-level PyramidPlan, two steps: the counters in ctx.sync agree with the row's geometry column (which
    tests/test_abi_cbam_nchw.py holds against the restatement), the statistics k_gate / k_pool's tail saved hold the bars, and the plan's
    outputs are the autograd path's bits."""
    c = row_case(name)
    row = NCHW_ROWS[ROW_IDS.index(name)]
    g = cbam_nchw_geo(c.B, c.C, c.H, c.W, c.k, c.hidden, c.dt, c.mask is not None and c.mask_grad)
    assert {k: g[k] for k in row[-1]} == row[-1]
    out = _form_test(F, c, g, name)
    _assert_same_bits(f"{name}: plan against autograd", out, _run(F, c))


@pytest.mark.parametrize("name", sorted(ENV_ROWS))
def test_cbam_nchw_row_again_under_its_knob(F, name, monkeypatch):
    """w150_narrow under MGACBAM_GATE_NARROW=1 runs k_gate with tiles inside one image row; one_tile_merged under MGACBAM_BWD_MERGE=0 runs the
    folded launch at k = 7: same oracle, same bars, and the counters of the form the knob asks for."""
    from mga_yolo_amd import _lib
    c, env = row_case(name), ENV_ROWS[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_env()
    try:
        g = cbam_nchw_geo(c.B, c.C, c.H, c.W, c.k, c.hidden, c.dt, c.mask is not None and c.mask_grad,
                          gate_narrow=env.get("MGACBAM_GATE_NARROW") == "1", bwd_merge=env.get("MGACBAM_BWD_MERGE", "1") != "0")
        _form_test(F, c, g, f"{name} {env}")
    finally:
        monkeypatch.undo()
        _lib.reload_env()


@pytest.mark.parametrize("name", ROW_IDS)
def test_k_pool_forms_ca_exactly_where_the_rule_says(F, name):
    """pool_forms_ca leaves no counter behind (the arrival words return to 0), so it is observed as test_gpu_pool_mlp does: run the pool
    stage, overwrite ca, run chan | apply.  Where k_pool's last arriver formed ca nothing forms it again and the overwritten values stay;
    anywhere else k_gate's role workgroups, k_mlp or k_chan's prologue write it anew.  Pins the rule from both sides of 1 MiB
    (pool_ca_b1 / pool_ca_b9 against below_1mib_nograd), with 2-byte elements (the two gvec 8 rows), and its other conditions (streamed MLP,
    C * hidden < 8192, k_gate eligible) at every row that misses one."""
    from mga_yolo_amd import _lib
    c = row_case(name)
    g = cbam_nchw_geo(c.B, c.C, c.H, c.W, c.k, c.hidden, c.dt, c.mask is not None and c.mask_grad)
    plan = _plan(F, c)
    S = _lib.FWD_STAGES
    plan.forward(S["pool"])
    torch.cuda.synchronize()
    plan.ctx_view(0)["ca"].fill_(0.25)
    plan.forward(S["chan"] | S["apply"])
    torch.cuda.synchronize()
    kept = bool((plan.ctx_view(0)["ca"] == 0.25).all())
    assert kept == g["pool_ca"], f"{name}: k_pool {'formed' if not kept else 'did not form'} ca, the rule says {g['pool_ca']}"
    plan.check_handoff()
    if not kept:                                                      # formed after the pool stage: the values the whole forward gives
        rep = _Report(f"{name} (staged forward)")
        rep.scale32("ca", plan.ctx_view(0)["ca"], c.c.ca)
        rep.done()


# ---------------------------------------------------------------------------------------------------------------------------
# c. forced forms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [dict(MGACBAM_POOL_TX="1", MGACBAM_POOL_CPT="1", MGACBAM_CHAN_TX="1"),
                                 dict(MGACBAM_POOL_TX="16", MGACBAM_POOL_CPT="1", MGACBAM_CHAN_TX="16"),
                                 dict(MGACBAM_POOL_TX="64", MGACBAM_POOL_CPT="4", MGACBAM_CHAN_TX="64"),
                                 dict(MGACBAM_POOL_TX="128", MGACBAM_POOL_CPT="2", MGACBAM_CHAN_TX="32"),
                                 dict(MGACBAM_POOL_TX="256", MGACBAM_POOL_CPT="4", MGACBAM_CHAN_TX="8"),
                                 dict(MGACBAM_BWD_MERGE="0"), dict(MGACBAM_POOL_MLP="0"), dict(MGACBAM_POOL_MLP="2"),
                                 dict(MGACBAM_GATE_NARROW="1")],
                         ids=["tx1_cpt1_ctx1", "tx16_cpt1_ctx16", "tx64_cpt4_ctx64", "tx128_cpt2_ctx32", "tx256_cpt4_ctx8", "merge0", "pool_mlp0",
                              "pool_mlp2", "gate_narrow"])
def test_forced_forms_hold_the_same_bars(F, env, monkeypatch):
    """KNOB_ROWS (fp32 at vec 1 and vec 4, fp16, bf16 scalar and with 16-byte k_gate lanes) under every forced launch geometry and form:
    each run goes against the row's own oracle at the row's own bars."""
    from mga_yolo_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_env()
    try:
        for name in KNOB_ROWS:
            c = row_case(name)
            rep = _Report(f"{name} {'/'.join(env.values())}")
            _check_outputs(rep, c, *_run(F, c))
            rep.done()
    finally:
        monkeypatch.undo()
        _lib.reload_env()


@pytest.mark.parametrize("name", KNOB_ROWS)
def test_backward_forms_give_the_same_bits(F, name, monkeypatch):
    """The merged launch (k_bwd_r12), the folded launch (MGACBAM_BWD_MERGE=0) and the unfused backward (fold_backward off) are documented as
    the same bits.  The default form and the three-launch forward (fuse_forward off; no bit equality is claimed for it) hold the row's
    bars."""
    from mga_yolo_amd import _lib
    c = row_case(name)

    def step(**kw):
        fold = kw.pop("fold_backward", True)
        plan = _plan(F, c, **kw)
        plan.fold_backward = fold
        plan.forward()
        plan.backward()
        out = _plan_out(plan)
        plan.check_handoff()
        return out

    base = step()
    unfused = step(fold_backward=False)
    three = step(fuse_forward=False)
    monkeypatch.setenv("MGACBAM_BWD_MERGE", "0")
    _lib.reload_env()
    try:
        folded = step()
    finally:
        monkeypatch.undo()
        _lib.reload_env()
    for what, out in (("unfused backward", unfused), ("folded backward", folded)):
        _assert_same_bits(f"{name}: {what} against the default form", out, base)
    for what, out in (("default", base), ("three-launch forward", three)):
        rep = _Report(f"{name} {what}")
        _check_outputs(rep, c, *out)
        rep.done()


def test_needx_and_nox_apply_give_the_same_bits(F):
    """k_bwd_apply's no-x instantiation runs only when every level of its launch has planes.  one_tile_merged has them; called together
    with h8_needx_ctx32 (same signature, no planes) it runs in the instantiation that can read x, and its results are the same bits."""
    a, b = row_case("one_tile_merged"), row_case("h8_needx_ctx32")
    ga = cbam_nchw_geo(a.B, a.C, a.H, a.W, a.k, a.hidden, a.dt, True)
    gb = cbam_nchw_geo(b.B, b.C, b.H, b.W, b.k, b.hidden, b.dt, True)
    assert ga["nox"] and not gb["nox"] and gb["make_proj"] == 0 and (a.k, a.dt, ga["vec"]) == (b.k, b.dt, gb["vec"])
    alone = _run(F, a)
    leaves = []
    for c in (a, b):
        leaves.append((c.x.cuda().requires_grad_(True), c.mask.cuda().requires_grad_(True), _params_dev(c, True), _cfg(F, c)))
    ys = F.mask_cbam_pyramid(leaves)
    torch.autograd.backward(ys, [a.gy.cuda(), b.gy.cuda()])
    torch.cuda.synchronize()
    x, m, ps, _ = leaves[0]
    together = (ys[0].detach(), dict(gx=x.grad, gmask=m.grad, **{k: p.grad for k, p in zip(PGRADS, ps)}))
    _assert_same_bits("one_tile_merged: NEEDX against no-x", together, alone)
    x, m, ps, _ = leaves[1]
    rep = _Report("h8_needx_ctx32 (grouped)")
    _check_outputs(rep, b, ys[1].detach(), dict(gx=x.grad, gmask=m.grad, **{k: p.grad for k, p in zip(PGRADS, ps)}))
    rep.done()


# ---------------------------------------------------------------------------------------------------------------------------
# d. half-precision mask
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mdt", ["f16", "bf16"])
def test_half_precision_mask_gets_its_gradient_in_its_own_type(F, mdt):
    """one_tile_merged with its mask rounded to fp16 / bf16 and passed in that type: the kernels read it as fp32 (exact), dL/dmask is
    computed in fp32 and comes back rounded once to the mask's type, so it is barred like a half output; everything else keeps fp32 bars."""
    from cbam_nchw_rows import DT, MAX_TIE_PIXELS, near_tie_pixels
    c = row_case("one_tile_merged")
    mask = c.mask.to(DT[mdt])
    y_o, g_o, o = oracle64(c.x, mask.float(), c.gy, c.p, c.use_sig, c.tiny_thr)
    skip = near_tie_pixels(c.x, o)
    assert int(skip.sum()) <= MAX_TIE_PIXELS
    y, g = _run(F, c, mask=mask)
    assert g["gmask"].dtype == DT[mdt]
    rep = _Report(f"one_tile_merged, {mdt} mask")
    _check_outputs(rep, c, y, g, y_o, g_o, mask_dt=mdt, skip_px=skip)
    rep.done()
