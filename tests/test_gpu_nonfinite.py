"""GPU tests (-m gpu): a NaN or an infinity that enters MaskCBAM, MaskECA, MaskSPADE or the mask head comes out non-finite wherever the
reference's torch operators carry it, and nowhere else ("Non-finite values").  The rows, the poisons and the expected values
(fp64 autograd of the families' eager forms on the CPU) are those of tests/nonfinite_cases.py; tests/test_nonfinite_host.py holds the
eager forms to the reference modules themselves and the rows to their launch forms.

  R1  wherever the expected value is non-finite, the device's is: y, gx, gmask, every parameter gradient, the running statistics.
  R2  wherever the expected value of y / gx / gmask is finite, the device's is finite and within the family's standing bar (below); a
      sample whose expected values the poison leaves as they were is the bits of the same call without the poison.
  R3  a parameter gradient (or running statistic) whose expected value is finite is within the bar or non-finite, never a wrong finite
      number; non-finite only in a call where some parameter gradient is expected non-finite too (the step is skipped either way).
  Absorbed cases (an infinite mask logit under use_sigmoid: the sigmoid saturates) are finite everywhere and within the bars.
  Indices (amax, valid, cidx) are not compared under poison.

Bars, the families' standing ones: MaskCBAM and MaskECA 1e-4 (fp32) / 4e-3 (fp16) / 3e-2 (bf16) of the tensor's scale, fp32 also 1e-3
element-wise on y / gx / gmask, parameter gradients tol * max|want| + 1e-7 |gy| |x| (test_gpu_channels_last_edges._check,
test_gpu_eca_channels_last._check); MaskSPADE fp32 1e-4 / 1e-3 element-wise, half precision at most twice the error of the torch
composition under autocast (test_gpu_spade_paths; _half_allowance says how that reads on part of a tensor); the mask head 1e-4 / 4e-3 / 3e-2 of the scale
(head_nchw_rows.TOL).  Under a poison the scale of a tensor is that of its finite part, and so are the norms of the floor (the clean
inputs')."""
import pytest
import torch

import nonfinite_cases as N
import plan_replays as PR
import spade_oracle as SO
from conftest import rel_err

pytestmark = pytest.mark.gpu
CL = torch.channels_last
TOL = {"f32": 1e-4, "f16": 4e-3, "bf16": 3e-2}
ELEM = 1e-3
MAX_TIE_PIXELS = 4                        # cbam_nchw_rows.MAX_TIE_PIXELS

# R2's named deviations: places where the device is non-finite although the expected value is finite, kept because removing them would
# cost an instruction in a streaming loop.  (family, poison id, tensor) -> (which elements, as a function of the case and the expected
# tensor -> bool mask; the source line that causes it).  The test asserts exactly that set.  None is kept.
KEPT = {}


@pytest.fixture(scope="module")
def F(built_lib):
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


@pytest.fixture(autouse=True)
def _stop_at_a_device_error():
    """A device error is no test failure to run on from: the session ends with it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error: {e}", returncode=3)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
def run_device(F, c, inp, layout):
    """One forward + backward of the family's autograd entry point on inp -> {output name: tensor}, the names of nonfinite_cases.eager_step"""
    fmt = CL if layout == "nhwc" else torch.contiguous_format
    x = inp["x"].cuda().to(c.dtype).contiguous(memory_format=fmt).requires_grad_(True)
    mask = None if inp["mask"] is None else inp["mask"].cuda().requires_grad_(True)
    gy = inp["gy"].cuda().to(c.dtype)
    P = {k: v.cuda().requires_grad_(True) for k, v in inp["params"].items()}
    run = None
    if "running" in inp:
        run = (inp["running"][0].cuda().clone(), inp["running"][1].cuda().clone(), torch.zeros((), dtype=torch.long, device="cuda"))
    if c.family == "cbam":
        y = F.mask_cbam(x, mask, *(P[k] for k in N.CBAM_KEYS), F.BlockConfig(**c.cfg))
    elif c.family == "eca":
        y = F.mask_eca(x, mask, P["w"], P["beta"], F.EcaConfig(**c.cfg))
    elif c.family == "head":
        w1 = P["w1"].detach().reshape(*P["w1"].shape, 1, 1).requires_grad_(True)
        y = F.mask_head(x, w1, P["gamma"], P["beta"], run[0], run[1], run[2], P["wh"], P["bh"], eps=c.cfg["eps"], momentum=c.cfg["momentum"],
                        training=c.cfg["training"])
        P["w1"] = w1
    else:
        y = F.mask_spade(x, mask, [P[k] for k in SO.PARAM_KEYS], F.SpadeConfig(**c.cfg), running=run)
    y.backward(gy.contiguous(memory_format=fmt) if gy.shape[1] > 1 else gy)
    torch.cuda.synchronize()
    if layout == "nhwc" and c.family != "head":
        assert y.is_contiguous(memory_format=CL) and x.grad.is_contiguous(memory_format=CL), "y / gx came back in another layout"
    out = dict(y=y.detach(), gx=x.grad)
    if mask is not None:
        out["gmask"] = mask.grad
    for k, p in P.items():
        out["g." + k] = p.grad.reshape(inp["params"][k].shape)
    if run is not None:
        out["running_mean"], out["running_var"] = run[0], run[1]
    return {k: v.detach().double().cpu() for k, v in out.items()}


_clean = {}


def clean_device(F, c, layout):
    key = (N.row_id(c.row), c.dt, c.training, layout)
    if key not in _clean:
        _clean[key] = run_device(F, c, c.inp, layout)
    return _clean[key]


def spade_composition(F, c, inp):
    """The block's torch composition under autocast on the device, on inp: the yardstick of MaskSPADE's half-precision bar"""
    x = inp["x"].cuda().to(c.dtype).requires_grad_(True)
    mask = inp["mask"].cuda().requires_grad_(True)
    P = {k: v.cuda().requires_grad_(True) for k, v in inp["params"].items()}
    cfg = F.SpadeConfig(**c.cfg)
    run = None
    if "running" in inp:
        run = (inp["running"][0].cuda().clone(), inp["running"][1].cuda().clone(), torch.zeros((), dtype=torch.long, device="cuda"))
    with torch.autocast("cuda", dtype=c.dtype):
        y = F.spade_compose(x, mask, [P[k] for k in SO.PARAM_KEYS], cfg, run)
    y.backward(inp["gy"].cuda().to(c.dtype))
    out = dict(y=y.detach(), gx=x.grad, gmask=mask.grad, **{"g." + k: p.grad for k, p in P.items()})
    if run is not None:
        out["running_mean"], out["running_var"] = run[0], run[1]
    return {k: v.detach().double().cpu() for k, v in out.items()}


_clean_comp = {}


def clean_composition(F, c):
    key = (N.row_id(c.row), c.dt)
    if key not in _clean_comp:
        _clean_comp[key] = spade_composition(F, c, c.inp)
    return _clean_comp[key]


# ---------------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------------
def _err_on(got, want, fin, elementwise=False, absolute=False):
    """rel_err / elem_err of conftest over the elements `fin`, the scale taken over them too (absolute: max |got - want| over them)"""
    if not bool(fin.any()):
        return 0.0
    d, w = (got - want).abs()[fin], want.abs()[fin]
    if absolute:
        return float(d.max())
    scale = float(w.max().clamp_min(1e-30))
    return float((d / w.clamp_min(ELEM * scale)).max()) if elementwise else float(d.max()) / scale


def _half_allowance(h, hc, w, cw, on):
    """MaskSPADE's half-precision bar gives the device twice the error of the torch composition under autocast, tensor by tensor.  Under a
    poison: twice the composition's worst absolute error over the compared elements `on` of this call or over the same tensor of the row's
    clean call, whichever is larger -- a poison takes elements out of the comparison and leaves the arithmetic of the others as it was,
    so the allowance the standing bar gives the row's tensor stays; a subset alone can hold the device's worst element and not the
    composition's."""
    return 2 * max(_err_on(h, w, on & torch.isfinite(h), absolute=True), _err_on(hc, cw, torch.ones_like(cw, dtype=torch.bool), absolute=True))


def check(F, c, layout, p, got, want, report):
    """R1 - R3 of one call.  p: the poison (None: the clean call, where everything is finite and within the bars)."""
    tol = TOL[c.dt]
    tag = "clean" if p is None else p.id
    clean_want, clean_got = N.expected(c), (got if p is None else clean_device(F, c, layout))
    floor = 1e-7 * float(c.inp["gy"].double().norm() * c.inp["x"].double().norm())
    inp = c.inp if p is None else N.poisoned(c, p)
    keep = None
    if c.family == "cbam":                                              # near-ties of the channel arg-max may route gx to either channel
        skip = N.cbam_near_tie_pixels(c, inp)
        assert int(skip.sum()) <= MAX_TIE_PIXELS, f"{int(skip.sum())} channel arg-max near-ties"
        keep = ~skip.reshape(c.B, 1, *want["gx"].shape[2:])
    half_ref = half_clean = None
    if c.family == "spade" and c.dt != "f32":
        half_clean = clean_composition(F, c)
        half_ref = half_clean if p is None else spade_composition(F, c, inp)
    any_param_nonfinite = any(not bool(torch.isfinite(w).all()) for k, w in want.items() if N.is_param_output(k))
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, w in want.items():
        g = got[name].reshape(w.shape)
        fin = torch.isfinite(w)
        # R1
        miss = ~fin & torch.isfinite(g)
        if bool(miss.any()):
            report.append(f"R1 {tag} {name}: {int(miss.sum())} of {int((~fin).sum())} expected non-finite elements are finite on the device "
                          f"(first at {tuple(int(i) for i in miss.nonzero()[0])}: {float(g[tuple(miss.nonzero()[0])]):.6g})")
        gfin = torch.isfinite(g)
        if N.is_param_output(name):
            # R3
            bad_nf = fin & ~gfin
            if bool(bad_nf.any()) and not any_param_nonfinite:
                report.append(f"R3 {tag} {name}: non-finite on the device in a call whose expected parameter gradients are all finite")
            both = fin & gfin
            if bool(both.any()):
                if c.family in ("cbam", "eca"):
                    d, bar = float((g - w).abs()[both].max()), tol * float(w.abs()[fin].max()) + floor
                    if not d <= bar:
                        report.append(f"R3 {tag} {name}: |diff| {d:.3e} over {bar:.3e}")
                elif half_ref is not None and name.startswith("g."):
                    a = _err_on(g, w, both, absolute=True)
                    b = _half_allowance(half_ref[name].reshape(w.shape), half_clean[name].reshape(w.shape), w, clean_want[name].reshape(w.shape), both)
                    if not a <= b:
                        report.append(f"R3 {tag} {name}: device |diff| {a:.3e} > {b:.3e} (twice the torch composition's)")
                else:
                    e = _err_on(g, w, both)
                    if not e <= (1e-4 if c.family == "spade" else tol):
                        report.append(f"R3 {tag} {name}: rel_err {e:.3e}")
            continue
        # R2
        extra = fin & ~gfin
        allowed = KEPT.get((c.family, tag, name))
        if allowed is not None:
            where = allowed[0](c, w)
            if not torch.equal(extra, where & fin):
                report.append(f"R2 {tag} {name}: the kept deviation ({allowed[1]}) is not exactly the set the table names")
            extra = extra & ~where
            fin = fin & ~where
        if bool(extra.any()):
            report.append(f"R2 {tag} {name}: {int(extra.sum())} of {int(fin.sum())} expected finite elements are non-finite on the device "
                          f"(first at {tuple(int(i) for i in extra.nonzero()[0])})")
        cmp_ = fin & gfin & (keep if (keep is not None and name == "gx") else torch.ones_like(fin))
        if half_ref is not None:
            a = _err_on(g, w, cmp_, absolute=True)
            b = _half_allowance(half_ref[name].reshape(w.shape), half_clean[name].reshape(w.shape), w, clean_want[name].reshape(w.shape), cmp_)
            if not a <= b:
                report.append(f"R2 {tag} {name}: device |diff| {a:.3e} > {b:.3e} (twice the torch composition's)")
        else:
            e = _err_on(g, w, cmp_)
            if not e <= (1e-4 if c.family == "spade" else tol):
                report.append(f"R2 {tag} {name}: rel_err {e:.3e}")
            if c.dt == "f32" and c.family != "head":
                ee = _err_on(g, w, cmp_, elementwise=True)
                if not ee < ELEM:
                    report.append(f"R2 {tag} {name}: element-wise {ee:.3e}")
        if p is not None:
            cw, cg = clean_want[name].reshape(w.shape), clean_got[name].reshape(w.shape)
            for b in range(w.shape[0]):
                if bool(torch.isfinite(w[b]).all()) and torch.equal(w[b], cw[b]) and not torch.equal(g[b], cg[b]):
                    report.append(f"R2 {tag} {name}: sample {b}, which the poison leaves alone, differs from the call without the poison in "
                                  f"{int((g[b] != cg[b]).sum())} elements")
        if p is not None and N.absorbed(c, p) and not bool(torch.isfinite(w).all()):
            report.append(f"absorbed {tag} {name}: the expected value is not finite everywhere")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. R1 - R3 and the absorbed cases: every (family, layout, row, dtype[, mode]) under every poison
# ---------------------------------------------------------------------------------------------------------------------------
def _has_mask(r):
    if r.family == "head":
        return False
    if r.family == "spade":
        return True
    return (N._table_row(N.CBAM_NCHW if r.family == "cbam" else N.ECA_NCHW, r.name)[8 if r.family == "cbam" else 7]
            if r.layout == "nchw" else (N.CBAM_NHWC if r.family == "cbam" else N.ECA_NHWC)[r.name][5]) != "none"


CALLS = [(r, layout, dt, training) for r in N.ROWS for layout in N.layouts(r) for dt in r.dtypes
         for training in ((True, False) if r.family == "head" else (True,))]
CALL_IDS = [f"{N.row_id(r)}{'-' + layout if r.layout == 'both' else ''}-{dt}{'' if training else '-eval'}" for r, layout, dt, training in CALLS]
POISONED = [(call, p) for call in CALLS for p in N.POISONS if p.target != "mask" or _has_mask(call[0])]
POISONED_IDS = [f"{CALL_IDS[CALLS.index(call)]}-{p.id}" for call, p in POISONED]


@pytest.mark.parametrize("call", CALLS, ids=CALL_IDS)
def test_clean_call_holds_the_bars(F, call):
    """The row without a poison, through the same runner and the same rules: the bars hold at the widened B and the chosen seeds, so a miss
    under a poison is the poison's."""
    r, layout, dt, training = call
    c = N.case(r, dt, training)
    report = []
    check(F, c, layout, None, clean_device(F, c, layout), N.expected(c), report)
    assert not report, f"{CALL_IDS[CALLS.index(call)]}: " + "; ".join(report)


@pytest.mark.parametrize("call,p", POISONED, ids=POISONED_IDS)
def test_non_finite_values_go_where_the_reference_carries_them(F, call, p):
    r, layout, dt, training = call
    c = N.case(r, dt, training)
    want = N.expected(c, p)
    got = run_device(F, c, N.poisoned(c, p), layout)
    report = []
    check(F, c, layout, p, got, want, report)
    nf = {k: int((~torch.isfinite(v)).sum()) for k, v in want.items()}
    print(f"{POISONED_IDS[POISONED.index((call, p))]}: expected non-finite elements {nf}")
    assert not report, "; ".join(report)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. residue in the eager path: pooled ctxs (MaskCBAM) and the allocator's recycled work buffers (the other families)
# ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return [k for k in a if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("call", CALLS, ids=CALL_IDS)
def test_clean_call_after_a_poisoned_one_gives_the_bits_of_a_fresh_ctx(F, call):
    """Fold counters, accumulate flags, saved planes and generation words survive a call.  After every poison, the next clean call on the
    recycled ctx gives the bits of the clean call on a ctx the process had never used."""
    r, layout, dt, training = call
    c = N.case(r, dt, training)
    F._POOL.clear()
    torch.cuda.empty_cache()
    fresh = run_device(F, c, c.inp, layout)
    for p in N.poisons_of(c):
        run_device(F, c, N.poisoned(c, p), layout)
        again = run_device(F, c, c.inp, layout)
        assert not _same_bits(fresh, again), f"after {p.id}: {_same_bits(fresh, again)} differ from the fresh call"
    F.handoff_report()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. residue in a captured static plan with its BucketOptimizer (the shapes of test_gpu_opt.test_plan_and_optimizer_replay_as_one_graph)
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)]
PLAN_ROWS = [(b, cl) for b in ("cbam", "eca", "spade") for cl in (False, True)]


@pytest.mark.parametrize("block,cl", PLAN_ROWS, ids=[f"{b}-{'cl' if c else 'nchw'}" for b, c in PLAN_ROWS])
def test_poisoned_replay_is_skipped_and_leaves_no_residue(built_lib, block, cl):
    """plan.step(); opt.step() captured once (heads -> blocks -> loss, then the fused optimizer step).  A replay whose gy holds a NaN sets
    found_inf and leaves parameters, optimizer state and t byte-identical; the clean replay after it equals a fresh plan (new ctx, scratch
    and sync state) with a fresh optimizer on the same state, outputs and optimizer state bit for bit."""
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    index = 70 + PLAN_ROWS.index((block, cl))
    r = PR.row(f"nonfinite-{block}", "slice", SHAPES, block=block, hidden=[16, 32, 64], cl=cl)
    state, cfgs = PR.initial_state(r)
    plan = PR.make_plan(r, cfgs, state)
    cfg = OptConfig("adamw", lr=[0.0007, 0.001, 0.001], momentum=0.9, weight_decay=5e-4, ema_tau=5.0)
    opt = BucketOptimizer.for_plan(plan, cfg)
    trained = [s for s in opt.segments if s.grad is not None]
    model_state = lambda o: [s.param for s in o.segments if s.grad is not None] + list(o._state0.values()) + list(o._state1.values())
    PR.load_inputs(plan, PR.make_inputs(r, index, 0, False))
    graph = opt.capture(plan)
    graph.replay()                                                      # one applied step first: the state is not all zero
    PR.check_handoff(plan)
    assert opt.t == 1 and int(opt.found_inf) == 0
    ins = PR.make_inputs(r, index, 1, False)
    t = ins["gy"][1]                                                    # the middle level, its middle sample
    t[(t.shape[0] // 2,) + tuple(n // 2 for n in t.shape[1:])] = float("nan")
    PR.load_inputs(plan, ins)
    before, t_before = [v.clone() for v in model_state(opt)], opt.t
    graph.replay()
    torch.cuda.synchronize()
    assert int(opt.found_inf) == 1, "the NaN in gy did not reach the gradient bucket"
    assert opt.t == t_before and all(torch.equal(a, b) for a, b in zip(model_state(opt), before))
    assert all(bool(torch.isfinite(s.param).all()) for s in trained)
    ins = PR.make_inputs(r, index, 2, False)
    PR.load_inputs(plan, ins)
    fresh = PR.fresh_like(plan)
    assert not (PR._storages(plan) & PR._storages(fresh))
    fopt = BucketOptimizer.for_plan(fresh, cfg)
    for a, b in zip(fopt.state_tensors(), opt.state_tensors()):
        a.copy_(b)
    PR.load_inputs(fresh, ins)
    graph.replay()
    fresh.step(); fopt.step()
    PR.check_handoff(plan); PR.check_handoff(fresh)
    assert int(opt.found_inf) == 0 and opt.t == 2
    differ = [(l, name) for (l, name, a), (_, _, b) in zip(PR.outputs(plan), PR.outputs(fresh)) if not torch.equal(a, b)]
    assert not differ, f"the clean replay after the poisoned one differs from a fresh plan in {differ}"
    names = [s.name for s in opt.segments]
    differ = [names[i % len(names)] for i, (a, b) in enumerate(zip(opt.state_tensors(), fopt.state_tensors())) if not torch.equal(a, b)]
    assert not differ, differ


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the GradScaler's overflow step through the modules
# ---------------------------------------------------------------------------------------------------------------------------
def _scaled_model(family):
    from mga_yolo_amd import MGAMaskHead, MaskCBAM, MaskECA, MaskSPADE
    torch.manual_seed(1)
    blk = dict(cbam=lambda: MaskCBAM(64), eca=lambda: MaskECA(64), spade=lambda: MaskSPADE(64, hidden=32), head=lambda: MGAMaskHead(64, 16))[family]()
    if family in ("cbam", "eca"):
        with torch.no_grad():
            blk.beta.fill_(0.5)
    return blk.cuda()


def _scaled_step(m, family, h0, mask, sign, fmt, scaler, opt, seen):
    """One step of block -> loss = sum(+-y) under fp16 autocast: dL/dy is +-scale, formed in fp32 and rounded to fp16 where y was cast.
    seen: what arrived at the block's output as dL/dy, and mean(y^2)."""
    h = h0.detach().clone(memory_format=fmt).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        y = m(h) if family == "head" else m([h, mask])
        assert y.dtype == torch.float16
        y.register_hook(lambda g: seen.update(gy_finite=bool(torch.isfinite(g).all()), gy_max=float(g.float().abs().max())))
        loss = (y.float() * sign).sum()
    opt.zero_grad(set_to_none=True)
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    grads = {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}
    grads["block_input"] = h.grad.detach().float() / float(scaler.get_scale())
    scaler.step(opt)
    scaler.update()
    seen["loss"] = float(y.detach().float().square().mean())          # the AMP tests' loss, as the figure the layouts are compared on
                                                                      # (the signed sum cancels to a few units: no scale to be relative to)
    return grads


@pytest.mark.parametrize("family", N.FAMILIES)
def test_scaler_overflow_step_is_skipped_and_the_next_one_is_applied(F, family):
    """The reference trainer's first steps overflow by design: GradScaler starts at 65536, the first power of two fp16 cannot hold.  With
    loss = sum(+-y) the scaled dL/dy that arrives at the block's output is +-65536 in fp32 and +-inf once rounded to fp16, in every
    element.  Step 1: the block's parameter gradients are non-finite, the step is skipped, the scale halves, the parameters are unchanged.
    So it goes on while a product inside the block's backward (gy * xhat, the half MFMA operands) still overflows fp16, as it does in
    torch's composition; every skipped step is held to the same three things.  The first step whose parameter gradients are finite is
    applied, at the same scale in both layouts, and channels_last agrees with NCHW at the bars of the AMP tests (test_amp_channels_last_model_matches_nchw:
    4e-3 on the loss and the parameters, 4 x 4e-3 on the gradients; MaskSPADE: the same bits, test_fp16_autocast_gradscaler_step_through_the_module)."""
    from conftest import synth
    tol = 4e-3
    torch.manual_seed(0)
    c1 = torch.nn.Conv2d(16, 64, 3, padding=1).cuda()
    x, mask, _ = synth(4, 16, 32, 32, seed=12)
    mask = mask.cuda()
    with torch.autocast("cuda", dtype=torch.float16):
        h0 = c1(x.cuda()).detach()                                      # fp16 feature, NCHW
    sign = (torch.rand(4, 1 if family == "head" else 64, 32, 32, generator=torch.Generator().manual_seed(3)) < 0.5).float().cuda() * 2 - 1
    scale = 65536.0
    res = {}
    for fmt in (torch.contiguous_format, CL):
        m = _scaled_model(family).to(memory_format=fmt)
        opt = torch.optim.SGD(m.parameters(), lr=1e-4)
        scaler = torch.amp.GradScaler("cuda")
        assert float(scaler.get_scale()) == scale
        p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
        skipped = 0
        while True:                                                     # steps until one is applied
            seen, before = {}, float(scaler.get_scale())
            g = _scaled_step(m, family, h0, mask, sign, fmt, scaler, opt, seen)
            bad = [n for n, t in g.items() if n != "block_input" and not bool(torch.isfinite(t).all())]
            assert seen["gy_max"] == before or (before == scale and not seen["gy_finite"]), (fmt, before, seen)
            if skipped == 0:
                assert not seen["gy_finite"] and bad, (fmt, seen, "no parameter gradient took the overflow")
            if not bad:
                break
            skipped += 1
            assert float(scaler.get_scale()) == before / 2, "the scale did not halve: the step was not skipped"
            assert all(torch.equal(p.detach(), p0[n]) for n, p in m.named_parameters()), "a skipped step moved a parameter"
            assert skipped <= 8, "the scale never came down to a step that is applied"
        assert float(scaler.get_scale()) == scale / 2 ** skipped and seen["gy_finite"]
        assert any(not torch.equal(p.detach(), p0[n]) for n, p in m.named_parameters()), "the applied step moved nothing"
        res[fmt] = (seen["loss"], g, {n: p.detach().clone() for n, p in m.named_parameters()}, skipped)
    assert res[torch.contiguous_format][3] == res[CL][3], "the two layouts skipped a different number of steps"
    res = {k: v[:3] for k, v in res.items()}
    (l0, g0, q0), (l1, g1, q1) = res[torch.contiguous_format], res[CL]
    if family == "spade":
        assert l0 == l1 and all(torch.equal(g0[n], g1[n]) for n in g0 if n != "block_input") and all(torch.equal(q0[n], q1[n]) for n in q0)
        assert torch.equal(torch.nan_to_num(g0["block_input"]), torch.nan_to_num(g1["block_input"]))
        return
    assert abs(l0 - l1) <= tol * abs(l0)
    both = torch.isfinite(g0["block_input"]) & torch.isfinite(g1["block_input"])
    assert float(both.float().mean()) > 0.99
    zero = torch.zeros_like(g0["block_input"])
    g0["block_input"], g1["block_input"] = torch.where(both, g0["block_input"], zero), torch.where(both, g1["block_input"], zero)
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 4 * tol, n
    for n in q0:
        assert rel_err(q1[n], q0[n]) < tol, n
