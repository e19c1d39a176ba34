"""The fused optimizer without a GPU: the parameter groups against the table the reference's own build_optimizer produced
(tests/golden/opt_groups.json, tools/gen_golden_opt.py), and BucketOptimizer's host path -- the torch restatement of csrc/opt.cuh that runs on
CPU tensors -- against the reference's recorded trajectories and against torch.optim.SGD / AdamW + clip_grad_norm_ + a restated ModelEMA on
random segments.  Every comparison uses the rule of tests/opt_ref.bar_check."""
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
