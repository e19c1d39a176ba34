"""The fused optimizer without a GPU: the parameter groups against the table the reference's own build_optimizer produced
(tests/golden/opt_groups.json, tools/gen_golden_opt.py), and BucketOptimizer's host path -- the torch restatement of csrc/opt.cuh that runs on
CPU tensors -- against the reference's recorded trajectories and against torch.optim.SGD / AdamW + clip_grad_norm_ + a restated ModelEMA on
random segments; then the same over a run's horizon (late starts at tau = 2000, a scaled accumulating run with skips, check_finite=False), with
the wrong settings those rows are built to notice.  Every comparison uses the rule of tests/opt_ref.bar_check."""
import pytest
import torch

import opt_ref as R
from opt_ref import make_case, run_against_torch, step_grads

def test_groups_equal_the_reference_table():
    """for_plan's rule, name by name, against what build_optimizer did with the reference's own modules"""
    from mga_yolo_amd import optim as O
    _, table = R.load_opt_golden("sgd")
    assert len(table["groups"]) == 20 and table["group_weight_decay"] == [0.0, table["decay"], 0.0]
    for full, group in table["groups"].items():
        kind, _, name = full.partition(".")
        if not name:
            kind, name = "model", full
        assert O.reference_group(kind, name) == group, full
    assert sorted(set(table["groups"].values())) == [0, 1, 2]
    assert table["groups"]["cbam.beta"] == table["groups"]["eca.beta"] == table["groups"]["mtl_log_vars"] == 1      # decayed: no "bias" in the name
    assert table["groups"]["head.proj.1.weight"] == 2 and table["groups"]["head.proj.1.bias"] == 0


@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_plan_segments_name_and_group_every_tensor(block):
    """plan_segments on the plans' lists (the plans themselves need the device: tests/test_gpu_opt.py builds real ones)"""
    from mga_yolo_amd import optim as O
    from mga_yolo_amd import plan as P
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES, SlicePlan
    _, table = R.load_opt_golden("sgd")
    cls, names = dict(cbam=(P.PyramidPlan, P.PARAM_NAMES), eca=(P.EcaPyramidPlan, P.ECA_PARAM_NAMES), spade=(P.SpadePyramidPlan, P.SPADE_PARAM_NAMES))[block]
    blk = cls.__new__(cls)
    blk.n = 2
    blk.params = [[torch.zeros(3) for _ in names] for _ in range(2)]
    blk.param_grads = [[torch.zeros(3) for _ in names] for _ in range(2)]
    if block == "spade":
        blk.running = [(None, None, None), (torch.zeros(4), torch.ones(4), torch.zeros((), dtype=torch.int64))]
    sp = SlicePlan.__new__(SlicePlan)
    sp.block, sp.n = blk, 2
    sp.head_params = [[torch.zeros(3) for _ in HEAD_PARAM_NAMES] for _ in range(2)]
    sp.head_grads = [[torch.zeros(3) for _ in HEAD_PARAM_NAMES] for _ in range(2)]
    sp.head_buffers = [(torch.zeros(4), torch.ones(4), torch.zeros((), dtype=torch.int64)) for _ in range(2)]
    sp.log_vars, sp.g_log_vars = torch.zeros(2), torch.zeros(2)
    segs = O.plan_segments(sp, ema=True)
    trained = [s for s in segs if s.grad is not None]
    assert len(trained) == 2 * len(names) + 2 * 5 + 1
    want = {k: v for k, v in table["groups"].items()}
    for s in trained:
        where, _, name = s.name.partition(".")
        key = "mtl_log_vars" if s.name == "mtl_log_vars" else f"{'head' if where.startswith('head') else block}.{name}"
        assert s.group == want[key], s.name
    assert {n.partition(".")[2] for n in (s.name for s in trained) if n.startswith("block")} == {k.partition(".")[2] for k in want if k.startswith(block + ".")}
    ema_only = [s.name for s in segs if s.grad is None]
    heads = [f"head{l}.proj.1.{n}" for l in range(2) for n in ("running_mean", "running_var")]
    assert ema_only == (["block1.norm.running_mean", "block1.norm.running_var"] if block == "spade" else []) + heads
    assert all(s.param.dtype.is_floating_point for s in segs)                                  # integer buffers are no segments
    assert [s.name for s in O.plan_segments(sp, ema=False)] == [s.name for s in trained]
    assert [s.name for s in O.plan_segments(blk, ema=False)] == [s.name for s in trained if s.name.startswith("block")]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_host_path_reproduces_the_reference_trajectories(kind):
    misses = R.run_golden(kind, "cpu")
    assert not misses, misses


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_host_path_agrees_with_torch(kind):
    misses = run_against_torch(kind, "cpu")
    assert not misses, misses


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_host_path_skips_on_a_non_finite_gradient(kind):
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    segs, grads, bucket, init, groups, bufs = make_case("cpu")
    opt = BucketOptimizer(segs, OptConfig(kind, ema_tau=5.0), "cpu")
    bucket.copy_(step_grads(0, "cpu"))
    opt.step()
    before = [t.clone() for s in segs for t in (s.param, opt._state0.get(s.name), opt._state1.get(s.name)) if t is not None]
    ema0 = {n: v.clone() for n, v in opt.ema.items()}
    grads["seg1025"][-1] = float("inf")
    opt.step()
    after = [t for s in segs for t in (s.param, opt._state0.get(s.name), opt._state1.get(s.name)) if t is not None]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert int(opt.found_inf) == 1 and opt.updates == 2 and opt.t == 1
    assert not torch.equal(opt.ema["seg4099"], ema0["seg4099"])


# ---- over a run's horizon (opt_ref: "a run's horizon") --------------------------------------------------------------------------------------
LATE_ROWS = [(k, u0, t0) for k in ("sgd", "adamw") for u0, t0 in R.LATE_STARTS]
MUTATIONS = [(k, u0, u0 - 10, w) for (k, u0), ws in sorted(R.BUILT_AGAINST.items()) for w in ws]


@pytest.mark.parametrize("kind,u0,t0", LATE_ROWS)
def test_host_path_agrees_with_torch_from_a_late_start(kind, u0, t0):
    R.check_late_row(kind, u0, t0, "cpu")


@pytest.mark.parametrize("kind,u0,t0,wrong", MUTATIONS)
def test_late_rows_miss_the_wrong_setting_they_are_built_against(kind, u0, t0, wrong):
    """tau x 1.01, ema_decay 0.99989 for 0.9999, beta2 0.9989 for 0.999, or one applied step too many, on BucketOptimizer's side alone: the
    row misses its bar.  Given the same wrong settings, the four-step rows above (tau = 5, t <= 4) pass with the changed ema_decay (worst
    error / bar 0.15) and the changed beta2 (0.21) as they do unchanged; they see a wrong tau only at their own tau = 5, where exp(-u / tau)
    is all of 1 - d, and a wrong t only where the bias corrections are coarsest.  At the reference's tau = 2000 and at t in the thousands
    nothing looked: that is the gap the late rows close.  (The same rows unchanged pass: test_host_path_agrees_with_torch_from_a_late_start.)"""
    assert (u0, t0) in R.LATE_STARTS and wrong in R.WRONG
    misses, _ = R.run_late(kind, u0, t0, "cpu", wrong=wrong)
    assert misses, (kind, u0, wrong)


def test_every_wrong_setting_has_its_row():
    assert sorted({w for ws in R.BUILT_AGAINST.values() for w in ws}) == sorted(R.WRONG)
    assert {u0 for _, u0 in R.BUILT_AGAINST} <= {u0 for u0, _ in R.LATE_STARTS}


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_host_path_scaled_accumulation_with_skips(kind):
    misses = R.run_scaled_accumulation(kind, "cpu")
    assert not misses, misses


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_host_path_check_finite_off_is_torch_without_a_scaler(kind, value):
    """What torch does with a non-finite gradient and no GradScaler, element for element.  An infinity: the norm is inf, coef = 10 / inf = 0,
    inf * 0 = NaN in that element of the parameter, its state and its average, and every other element takes a step on a zero gradient
    (weight decay and the momentum it already had).  A NaN: a NaN norm, a NaN coefficient, and every trained tensor is NaN throughout; only
    the EMA-only buffer's average stays finite."""
    misses = R.run_unchecked(kind, "cpu", value)
    assert not misses, misses


# ---- SGD with momentum 0 ------------------------------------------------------------------------------------------------------------------
def test_sgd_refuses_momentum_zero_because_torch_keeps_the_buffer():
    """torch.optim.SGD leaves momentum_buffer alone while momentum is 0 (and would create it as clone(g) on the first non-zero step);
    k_opt_step and the host path store buf = 0 buf + g.  The parameters agree while momentum is 0 and part once it is back: shown here with
    the momentum words written past set_group, which refuses the value -- the reference's warm-up starts at 0.8, and torch itself refuses
    nesterov with momentum 0 at construction."""
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig, _word
    segs, grads, bucket, init, groups, bufs = make_case("cpu")
    opt = BucketOptimizer(segs, OptConfig("sgd", lr=0.01, momentum=0.9, weight_decay=5e-4), "cpu")
    for m in (0.0, -0.1, 1.0):
        with pytest.raises(ValueError, match="momentum"):
            opt.set_group(1, momentum=m)
        with pytest.raises(ValueError, match="momentum"):
            BucketOptimizer(segs, OptConfig("sgd", momentum=m), "cpu")
    opt.set_group(1, momentum=0.5)
    opt.set_group(1, momentum=0.9)
    kw = dict(decay=5e-4, buffers=bufs)
    t32 = R.TorchTail("sgd", init, groups, dtype=torch.float32, device="cpu", **kw)
    t64 = R.TorchTail("sgd", init, groups, dtype=torch.float64, device="cpu", **kw)
    missed = []
    for i, m in enumerate([0.9, 0.9, 0.0, 0.0, 0.9]):
        for j in range(3):
            opt._host_f[_word("momentum") + j], opt._host_f[_word("one_minus_momentum") + j] = m, 1.0 - m
        opt._upload()
        bucket.copy_(step_grads(i, "cpu"))
        gs = {n: g.clone() for n, g in grads.items()}
        opt.step()
        t32.step(gs, [0.01] * 3, [m] * 3, buffers=bufs)
        t64.step(gs, [0.01] * 3, [m] * 3, buffers=bufs)
        a32, a64 = t32.tensors(), t64.tensors()
        missed.append(bool(sum((R.bar_check(f"momentum {m} step {i} {s.name}", s.param, a32[f"param.{s.name}"], a64[f"param.{s.name}"])
                                for s in segs if s.grad is not None), [])))
    assert missed == [False, False, False, False, True], missed
