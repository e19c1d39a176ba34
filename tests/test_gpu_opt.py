"""The fused optimizer step (include/mgaopt.h, mga_yolo_amd/optim.py) on the MI355X, at the smallest sizes at which the chunking can go wrong:
segments of 1, 2, 147, 1023, 1024, 1025 and 4099 elements laid out in one bucket in that order -- every gradient view after the first is
misaligned to 16 bytes and a chunk ends inside a segment --, all three parameter groups, and one EMA-only segment of 65 elements.

Every comparison with torch uses the rule of tests/opt_ref.bar_check: the oracle is an fp64 run of the same torch sequence on the host, and the
device result may differ from it by at most max(1e-6 max|p|, 4 x the error of torch's own fp32 device run against that oracle).

Sections 6 and 7 run the same segments where a run spends its time: 256 steps from `updates` = 0, 1000 and 20000 at the reference's tau = 2000
under the warm-up schedule, a GradScaler's run of scaled, accumulated and skipped steps, and check_finite=False against torch element for element.

The measured figures are in DESIGN 7h."""
import pytest
import torch

import opt_ref as R
import plan_replays as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ["sgd", "adamw"]


def _worst(figures):
    what, err, own, scale, bar = max(figures, key=lambda f: f[1] / max(f[4], 1e-300))
    return f"worst error / bar: {err:.3e} / {bar:.3e} ({what})"


# ---- 1. against torch and against the reference's trajectories ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_steps_agree_with_torch(built_lib, kind):
    """K = 4 steps, group lr and momentum changed before each, the clip active at steps 0 and 2 and inactive at 1 and 3 (asserted inside)"""
    figures = []
    misses = R.run_against_torch(kind, DEV, figures)
    print(kind, _worst(figures))
    assert not misses, misses


@pytest.mark.parametrize("kind", KINDS)
def test_steps_reproduce_the_reference_trajectories(built_lib, kind):
    misses = R.run_golden(kind, DEV)
    assert not misses, misses


# ---- helpers of the bit-exact cases ------------------------------------------------------------------------------------------------------
def _opt(kind, accumulate=False, check_finite=True, seed=0):
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    segs, grads, bucket, _, _, _ = R.make_case(DEV, seed)
    cfg = OptConfig(kind, lr=[0.05, 0.01, 0.01] if kind == "sgd" else [0.001, 0.002, 0.002], momentum=0.9, weight_decay=5e-4, ema_tau=5.0,
                    check_finite=check_finite)
    return BucketOptimizer(segs, cfg, DEV, accumulate=accumulate, bucket=bucket), grads, bucket


def _model_state(opt):
    """parameters, optimizer state and the applied-step count: what a skipped step must leave alone"""
    trained = [s for s in opt.segments if s.grad is not None]
    return [s.param for s in trained] + list(opt._state0.values()) + list(opt._state1.values())


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---- 2. a non-finite gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("how", ["inf", "nan", "external"])
def test_a_non_finite_gradient_skips_the_step(built_lib, kind, how):
    opt, grads, bucket = _opt(kind)
    bucket.copy_(R.step_grads(0, DEV))
    opt.step()                                                          # one applied step first: the state is not all zero
    before = [t.clone() for t in _model_state(opt)]
    ema0 = {n: v.clone() for n, v in opt.ema.items()}
    assert opt.t == 1 and opt.updates == 1
    bucket.copy_(R.step_grads(1, DEV))
    if how == "external":
        opt.set_external(found_inf=True)
    else:
        grads["seg1025"][-1] = float(how)                               # the last element of a segment whose last chunk holds one element
    opt.step()
    torch.cuda.synchronize()
    assert _same(_model_state(opt), before)
    assert opt.t == 1 and opt.updates == 2                              # the applied-step count stays, the EMA's count advances
    assert int(opt.found_inf) == (0 if how == "external" else 1)
    for s in opt.segments:                                              # d ema + (1 - d) p: the average of every parameter that had moved, moved
        assert s.grad is None or not torch.equal(opt.ema[s.name], ema0[s.name]), s.name
    # the next clean step is applied, with bias corrections of t = 2
    opt.set_external(found_inf=False)
    bucket.copy_(R.step_grads(2, DEV))
    opt.step()
    assert opt.t == 2 and opt.updates == 3 and int(opt.found_inf) == 0 and not _same(_model_state(opt), before)


@pytest.mark.parametrize("kind", KINDS)
def test_check_finite_off_applies_the_step(built_lib, kind):
    opt, grads, bucket = _opt(kind, check_finite=False)
    bucket.copy_(R.step_grads(0, DEV))
    grads["seg1025"][-1] = float("inf")
    before = [t.clone() for t in _model_state(opt)]
    opt.step()
    assert opt.t == 1 and int(opt.found_inf) == 1
    assert not _same(_model_state(opt), before)                          # what the reference does without a scaler


# ---- 3. the loss scale -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_power_of_two_scale_unscales_exactly(built_lib, kind):
    a, _, bucket_a = _opt(kind)
    b, _, bucket_b = _opt(kind)
    b.set_scale(1024.0)
    for t in range(2):
        g = R.step_grads(t, DEV)
        bucket_a.copy_(g); bucket_b.copy_(g * 1024.0)
        a.step(); b.step()
    assert _same(_model_state(a), _model_state(b)) and _same(list(a.ema.values()), list(b.ema.values()))
    assert float(a.grad_norm) == float(b.grad_norm) and a.t == b.t == 2


# ---- 4. accumulation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_accumulated_micro_steps_equal_one_step_on_their_sum(built_lib, kind):
    a, _, bucket_a = _opt(kind, accumulate=True)
    b, _, bucket_b = _opt(kind)
    total = torch.zeros_like(bucket_b)
    for t in range(4):
        g = R.step_grads(t, DEV)
        bucket_a.copy_(g)
        a.accumulate()
        total += g                                                      # the same additions in the same order
    assert torch.equal(a.acc, total)
    bucket_a.fill_(float("nan"))                                         # step() reads acc, not the bucket
    bucket_b.copy_(total)
    a.step(); b.step()
    assert _same(_model_state(a), _model_state(b)) and _same(list(a.ema.values()), list(b.ema.values()))
    assert float(a.grad_norm) == float(b.grad_norm) > 0 and int(a.found_inf) == 0
    assert int(torch.count_nonzero(a.acc)) == 0                         # left zero for the next 16 micro-steps
    assert torch.equal(bucket_b, total)                                 # without accumulation the bucket is read and left alone


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_give_the_same_bits(built_lib, kind):
    a, _, bucket_a = _opt(kind)
    b, _, bucket_b = _opt(kind)
    assert not {t.data_ptr() for t in a.state_tensors()} & {t.data_ptr() for t in b.state_tensors()}
    for t in range(3):
        g = R.step_grads(t, DEV)
        bucket_a.copy_(g); bucket_b.copy_(g)
        a.set_external(sumsq=200.0 * (t & 1)); b.set_external(sumsq=200.0 * (t & 1))
        a.step(); b.step()
        assert _same(a.state_tensors(), b.state_tensors()), t


# ---- 6. over a run's horizon (opt_ref: "a run's horizon"; tests/test_opt_host.py runs the same rows through the host path) -----------------
def _worst_by_kind(figures):
    return " | ".join(f"worst {k}: " + "{1:.1e} / {2:.1e} / {4:.1e} ({0})".format(*max((f for f in figures if f" {k}." in f[0]), key=lambda f: f[1] / f[4]))
                      for k in ("param", "ema"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("u0,t0", R.LATE_STARTS)
def test_steps_agree_with_torch_from_a_late_start(built_lib, kind, u0, t0):
    """256 steps from `updates` = u0 with t0 applied steps, tau = 2000, decay 0.9999, the warm-up schedule, every fourth step clipped:
    expm1f(t ln m), expm1f(t ln beta2) and expf(-u / tau) at the arguments of a run under way.  Compared at steps 1, 16, 64 and 256, and at
    256 every tensor has moved at least 100 bars (both inside check_late_row).  That the rows miss a tau, ema_decay, beta2 or t that is
    slightly wrong is shown on the host path (tests/test_opt_host.py)."""
    figures, least = R.check_late_row(kind, u0, t0, DEV)
    print(kind, u0, _worst_by_kind(figures), "| least displacement / bar", f"{least:.0f}")


# ---- 7. the GradScaler's run: scaled, accumulated, skipped ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_scaled_accumulation_with_skips(built_lib, kind):
    """40 steps of 4 accumulate() calls on scale x g, the scale halved and doubled as GradScaler.update does, an inf or a NaN in one micro-step
    of five steps: skips at an even and an odd `updates` and two in a row.  After every step acc is all zero -- a skipped step that left it
    alone would keep the inf and skip every step after --, found_inf, updates and t are as injected, and a skipped step leaves parameters
    and state bit for bit (all inside run_scaled_accumulation); at steps 1, 8 and 40 everything is within the bar of the fp64 tail."""
    figures = []
    misses = R.run_scaled_accumulation(kind, DEV, figures)
    print(kind, _worst_by_kind(figures))
    assert not misses, misses


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_check_finite_off_is_torch_without_a_scaler(built_lib, kind, value):
    """What torch does with a non-finite gradient and no GradScaler, element for element.  An infinity: the norm is inf, coef = 10 / inf = 0,
    inf * 0 = NaN in that element of the parameter, its state and its average, and every other element takes a step on a zero gradient
    (weight decay and the momentum it already had).  A NaN: a NaN norm, a NaN coefficient, and every trained tensor is NaN throughout; only
    the EMA-only buffer's average stays finite.  NaN positions equal the fp64 tail's in parameters, state and averages; the finite elements
    are within the bar."""
    figures = []
    misses = R.run_unchecked(kind, DEV, value, figures)
    print(kind, value, _worst(figures) if figures else "nothing finite")
    assert not misses, misses


def test_sgd_refuses_momentum_zero(built_lib):
    """k_opt_step stores buf = g at momentum 0 where torch leaves the buffer alone (tests/test_opt_host.py shows the trajectories part)"""
    opt, _, _ = _opt("sgd")
    with pytest.raises(ValueError, match="momentum"):
        opt.set_group(0, momentum=0.0)


# ---- 8. in the graph ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)]
GRAPH_ROWS = [("cbam", False), ("spade", True)]                         # (block, channels_last); MaskSPADE's middle level is a batch-norm level
GRAPH_LR = dict(sgd=[[0.1, 0.002, 0.002], [0.08, 0.004, 0.004], [0.05, 0.007, 0.007], [0.01, 0.01, 0.01]],
                adamw=[[0.0, 0.0005, 0.0005], [0.0007, 0.001, 0.001], [0.0014, 0.0015, 0.0015], [0.002, 0.002, 0.002]])
GRAPH_MOMENTUM = [0.8, 0.83, 0.88, 0.9]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block,cl", GRAPH_ROWS, ids=[f"{b}-{'cl' if c else 'nchw'}" for b, c in GRAPH_ROWS])
def test_plan_and_optimizer_replay_as_one_graph(built_lib, block, cl, kind):
    """plan.step(); opt.step() captured once and replayed four times on fresh inputs, group lr and momentum changed between replays without a
    re-capture.  After every replay: a torch optimizer holding clones of the initial parameters, fed the plan's own bucket, agrees within the
    bar (this isolates the optimizer from the kernels before it); the same row run eagerly on a second plan gives the same bits, y included,
    so the replays read the moved weights; y differs from the replay before; check_handoff() is clean."""
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    index = 40 + GRAPH_ROWS.index((block, cl))
    r = PR.row(f"opt-{block}", "slice", SHAPES, block=block, hidden=[16, 32, 64], cl=cl)
    state, cfgs = PR.initial_state(r)
    plan = PR.make_plan(r, cfgs, state)
    twin = PR.fresh_like(plan)                                          # on clones: the two share no parameter
    assert not (PR._storages(plan) & PR._storages(twin))
    cfg = OptConfig(kind, lr=GRAPH_LR[kind][0], momentum=GRAPH_MOMENTUM[0], weight_decay=5e-4, ema_tau=5.0)
    opt, topt = BucketOptimizer.for_plan(plan, cfg), BucketOptimizer.for_plan(twin, cfg)
    names = [s.name for s in opt.segments]
    trained = [s for s in opt.segments if s.grad is not None]
    ema_only = [s for s in opt.segments if s.grad is None]
    assert len(trained) == 3 * len(plan.block.params[0]) + 3 * 5 + 1 and sorted({s.group for s in trained}) == [0, 1, 2]
    assert len(ema_only) == 6 + (2 if block == "spade" else 0)          # the heads' running statistics, and the batch-norm level's
    assert sum(s.grad.numel() for s in trained) == plan.grad_bucket.numel()
    kw = dict(decay=5e-4, buffers={s.name: s.param for s in ema_only}, ema_tau=5.0)
    init, groups = {s.name: s.param.clone() for s in trained}, {s.name: s.group for s in trained}
    t32 = R.TorchTail(kind, init, groups, dtype=torch.float32, device=DEV, **kw)
    t64 = R.TorchTail(kind, init, groups, dtype=torch.float64, device="cpu", **kw)
    PR.load_inputs(plan, PR.make_inputs(r, index, 0, False))
    before = [t.clone() for t in opt.state_tensors()]
    graph = opt.capture(plan)                                           # its warm-up step is undone
    torch.cuda.synchronize()
    assert _same(opt.state_tensors(), before) and opt.updates == 0 and opt.t == 0
    figures, misses, y_prev = [], [], None
    for t in range(PR.K):
        ins = PR.make_inputs(r, index, t, False)
        PR.load_inputs(plan, ins); PR.load_inputs(twin, ins)
        for o in (opt, topt):
            for j in range(3):
                o.set_group(j, lr=GRAPH_LR[kind][t][j], momentum=GRAPH_MOMENTUM[t])
        graph.replay()
        twin.step(); topt.step()
        PR.check_handoff(plan); PR.check_handoff(twin)
        # the eager row: the same bits
        assert torch.equal(plan.grad_bucket, twin.grad_bucket), t
        for l in range(plan.n):
            assert torch.equal(plan.y[l], twin.y[l]), (t, l)
        for i, (a, b) in enumerate(zip(opt.state_tensors(), topt.state_tensors())):
            assert torch.equal(a, b), (t, i, names[i % len(names)])
        assert opt.updates == t + 1 and opt.t == t + 1 and int(opt.found_inf) == 0
        y = [v.clone() for v in plan.y]
        assert y_prev is None or all(not torch.equal(a, b) for a, b in zip(y, y_prev)), t
        y_prev = y
        # torch, fed the plan's own bucket
        gs = {s.name: s.grad.clone() for s in trained}
        bufs = {s.name: s.param for s in ema_only}
        lr, mom = GRAPH_LR[kind][t], [GRAPH_MOMENTUM[t]] * 3
        n32, _ = t32.step(gs, lr, mom, buffers=bufs)
        n64, c64 = t64.step(gs, lr, mom, buffers=bufs)
        assert abs(float(opt.grad_norm) - n64) <= max(1e-6 * n64, 4 * abs(n32 - n64)) and abs(float(opt.clip_coef) - c64) <= 1e-6
        ours = {f"param.{s.name}": s.param for s in trained}
        ours.update({f"ema.{n}": v for n, v in opt.ema.items()})
        a32, a64 = t32.tensors(), t64.tensors()
        assert sorted(ours) == sorted(a64)
        for name in ours:
            misses += R.bar_check(f"{block} {kind} replay {t} {name}", ours[name], a32[name], a64[name], figures)
    moved = max(float((s.param - init[s.name]).abs().max()) for s in trained)
    print(block, kind, _worst(figures), "| largest parameter move", moved)
    assert moved > 0
    assert not misses, misses
