"""The pyramid gate with in-kernel Philox noise (include/mgagate.h, csrc/gate_rng.cuh) on the device, fp32 throughout.
The kernels draw their own uniforms, so every check that involves noise rebuilds those uniforms on the host from the pure-Python restatement
(tests/philox_ref.py), uploads them and asks the EXISTING per-level path (mgapmg_forward / mgapmg_backward, pinned to the reference's goldens
by tests/test_gater.py and tests/test_gpu_loss_rows.py) for the answer: equal uniforms must give equal bits (torch.equal), both directions.
Then the device-resident state, graph replay of a gated PyramidPlan, and a gated SlicePlan against the module composition at the bars of
tests/test_gpu_slice_plan.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_ref as PR
from conftest import rel_err

pytestmark = pytest.mark.gpu

SMALL = [(2, 1, 8, 8), (2, 1, 5, 3), (1, 1, 1, 1)]
ODD = [(3, 1, 17, 23)]
# the kernels sweep a level with a grid stride once it is past 2048 workgroups of 256: one level that is (529,200 elements)
ODD_AND_LARGE = ODD + [(3, 1, 420, 420)]
SEED, STEP = 5, 3
TAU, THR = 0.3, 0.5
MODES = ("gumbel", "hard_st", "bernoulli_detach", "deterministic")


def _inputs(shapes, p_min, seed=11):
    """Per level: the p edges of oracle.loss_rows.gater_edge_grid(p_min) (every clamp bound and its neighbours), then randn around the
    unit interval so that values fall below 0, inside and above 1."""
    from oracle.loss_rows import gater_edge_grid
    grid = gater_edge_grid(p_min)[0]
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in shapes:
        n = int(np.prod(shp))
        edges = grid.reshape(-1) if n >= grid.numel() else grid[0, 0, :, 0]
        out.append(torch.cat([edges, 0.5 + 0.6 * torch.randn(n, generator=g)])[:n].reshape(shp).contiguous().cuda())
    return out


def _uniforms(shape, seed, step, stream_id):
    u1, u2 = PR.uniform_arrays(seed, step, stream_id, int(np.prod(shape)))
    return torch.from_numpy(u1).reshape(shape).cuda(), torch.from_numpy(u2).reshape(shape).cuda()


def _cfgs(mode, n, p_min, stream_ids=None):
    from mga_yolo_amd import GateConfig
    return [GateConfig(mode, TAU, p_min, THR, stream_id=None if stream_ids is None else stream_ids[l]) for l in range(n)]


def _new_fwd(ps, cfgs, state):
    """mgagate_forward on a hand-filled table -> (outs, msofts): msoft is not something the autograd entry point returns."""
    from mga_yolo_amd import _binding, _lib
    n = len(ps)
    outs, msofts = [torch.full_like(p, -7.0) for p in ps], [torch.full_like(p, -7.0) for p in ps]
    levels = (_lib.GateLevel * n)()
    for l, (p, c) in enumerate(zip(ps, cfgs)):
        _binding.fill_gate(levels[l], p, outs[l], msofts[l], None, None, c.code(), c.stream(l), c.tau, c.p_min, c.threshold)
    _binding.call("mgagate_forward", ps[0].device, levels, n, state.data_ptr())
    return outs, msofts


def _new_bwd(ps, msofts, gouts, cfgs):
    from mga_yolo_amd import _binding, _lib
    n = len(ps)
    gps = [torch.full_like(p, -7.0) for p in ps]
    levels = (_lib.GateLevel * n)()
    for l, (p, c) in enumerate(zip(ps, cfgs)):
        _binding.fill_gate(levels[l], p, None, msofts[l], gouts[l], gps[l], c.code(), c.stream(l), c.tau, c.p_min, c.threshold)
    _binding.call("mgagate_backward", ps[0].device, levels, n)
    return gps


def _old_fwd(p, u1, u2, p_min, hard):
    """mgapmg_forward: the existing one-level kernel on uploaded uniforms -> (out, msoft)"""
    from mga_yolo_amd import _binding, _lib
    out, msoft = torch.empty_like(p), torch.empty_like(p)
    cfg = _lib.PmgCfg(TAU, p_min, THR, int(hard))
    _binding.call("mgapmg_forward", p.device, p.data_ptr(), u1.data_ptr(), u2.data_ptr(), out.data_ptr(), msoft.data_ptr(), p.numel(), C.byref(cfg))
    return out, msoft


def _old_bwd(p, msoft, gout, p_min, hard):
    from mga_yolo_amd import _binding, _lib
    gp = torch.empty_like(p)
    cfg = _lib.PmgCfg(TAU, p_min, THR, int(hard))
    _binding.call("mgapmg_backward", p.device, p.data_ptr(), msoft.data_ptr(), gout.data_ptr(), gp.data_ptr(), p.numel(), C.byref(cfg))
    return gp


def _clamped(p, p_min):
    q = p.clamp(0.0, 1.0)
    return q.clamp_min(p_min) if p_min > 0 else q


def _expected(mode, p, p_min, seed, step, stream_id):
    """(out, msoft | None) of one level, from the restatement's uniforms and the existing kernel / torch"""
    if mode == "deterministic":
        return _clamped(p, p_min), None
    u1, u2 = _uniforms(p.shape, seed, step, stream_id)
    if mode == "bernoulli_detach":
        return (u1 < _clamped(p, p_min)).float(), None
    return _old_fwd(p, u1, u2, p_min, mode == "hard_st")


# ---- 1, 2: bits, forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_min", [0.0, 0.2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shapes", [SMALL, ODD_AND_LARGE], ids=["small3", "odd+large"])
def test_forward_bits_equal_the_existing_kernel_on_the_restatements_uniforms(built_lib, shapes, mode, p_min):
    from mga_yolo_amd import gate_state, prob_mask_gate_pyramid
    ps = _inputs(shapes, p_min)
    cfgs = _cfgs(mode, len(ps), p_min)
    state = gate_state(SEED, STEP)
    outs, msofts = _new_fwd(ps, cfgs, state)
    torch.cuda.synchronize()
    for l, p in enumerate(ps):
        want, want_soft = _expected(mode, p, p_min, SEED, STEP, l)
        assert torch.equal(outs[l], want), (l, float((outs[l] - want).abs().max()))
        if want_soft is not None:
            assert torch.equal(msofts[l], want_soft), l
            if mode == "gumbel":
                assert torch.equal(outs[l], msofts[l])
            else:
                assert set(outs[l].unique().tolist()) <= {0.0, 1.0}
        else:
            assert bool((msofts[l] == -7.0).all())                   # the modes without a soft sample leave msoft alone
    # the autograd entry point is the same call
    outs2 = prob_mask_gate_pyramid(ps, gate_state(SEED, STEP), cfgs)
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2))
    # a level run alone under its stream id is that level of the pyramid call
    if len(ps) > 1:
        l = 1
        alone, alone_soft = _new_fwd([ps[l]], _cfgs(mode, 1, p_min, stream_ids=[l]), gate_state(SEED, STEP))
        assert torch.equal(alone[0], outs[l]) and torch.equal(alone_soft[0], msofts[l])
        if mode == "gumbel":                                         # ... and under another stream id it is not
            other, _ = _new_fwd([ps[l]], _cfgs(mode, 1, p_min, stream_ids=[l + 1]), gate_state(SEED, STEP))
            assert not torch.equal(other[0], outs[l])


def test_mixed_modes_share_one_call(built_lib):
    """Levels of all four modes in one launch: each is what it is alone."""
    from mga_yolo_amd import GateConfig, gate_state
    shapes = SMALL + ODD
    ps = _inputs(shapes, 0.2)
    cfgs = [GateConfig(m, TAU, 0.2, THR) for m in ("deterministic", "hard_st", "bernoulli_detach", "gumbel")]
    state = gate_state(SEED, STEP)
    outs, msofts = _new_fwd(ps, cfgs, state)
    for l, (p, c) in enumerate(zip(ps, cfgs)):
        want, want_soft = _expected(c.mode, p, 0.2, SEED, STEP, l)
        assert torch.equal(outs[l], want), l
        if want_soft is not None:
            assert torch.equal(msofts[l], want_soft), l
    assert state.tolist() == [SEED, STEP + 1, 0, 0]


# ---- 3: the device-resident state -------------------------------------------------------------------------------------------------------
def test_state_advances_only_when_noise_is_drawn(built_lib):
    from mga_yolo_amd import GateConfig, gate_state
    ps = _inputs(SMALL, 0.0)
    seed, step = 2 ** 40 + 7, 2 ** 32 - 1                            # the step's carry into its high word rides along
    state = gate_state(seed, step)
    cfgs = _cfgs("gumbel", len(ps), 0.0)
    first, _ = _new_fwd(ps, cfgs, state)
    assert state.tolist() == [seed, step + 1, 0, 0]
    second, _ = _new_fwd(ps, cfgs, state)
    assert state.tolist() == [seed, step + 2, 0, 0]
    for l, p in enumerate(ps):
        assert torch.equal(first[l], _expected("gumbel", p, 0.0, seed, step, l)[0]), l
        assert torch.equal(second[l], _expected("gumbel", p, 0.0, seed, step + 1, l)[0]), l
    assert not torch.equal(first[0], second[0])
    # deterministic levels only (by mode, or a gate in eval): the state is not touched
    for det in (_cfgs("deterministic", len(ps), 0.0), [GateConfig("gumbel", TAU, 0.0, THR, training=False)] * len(ps)):
        outs, _ = _new_fwd(ps, det, state)
        assert state.tolist() == [seed, step + 2, 0, 0]
        assert all(torch.equal(o, _clamped(p, 0.0)) for o, p in zip(outs, ps))
    # one noisy level among deterministic ones is a noisy call
    _new_fwd(ps, [GateConfig("deterministic"), GateConfig("bernoulli_detach"), GateConfig("deterministic")], state)
    assert state.tolist() == [seed, step + 3, 0, 0]


# ---- 4: backward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_min", [0.0, 0.2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shapes", [SMALL, ODD], ids=["small3", "odd"])
def test_backward_equals_the_existing_kernel_and_autograd_delivers_it(built_lib, shapes, mode, p_min):
    from mga_yolo_amd import gate_state, prob_mask_gate_pyramid
    ps = _inputs(shapes, p_min)
    cfgs = _cfgs(mode, len(ps), p_min)
    g = torch.Generator().manual_seed(3)
    gouts = [torch.randn(p.shape, generator=g).cuda() for p in ps]
    outs, msofts = _new_fwd(ps, cfgs, gate_state(SEED, STEP))
    gps = _new_bwd(ps, msofts, gouts, cfgs)
    for l, p in enumerate(ps):
        if mode in ("gumbel", "hard_st"):
            want = _old_bwd(p, msofts[l], gouts[l], p_min, mode == "hard_st")
            assert bool((want != 0).any()) or p.numel() == 1
        elif mode == "bernoulli_detach":
            want = torch.zeros_like(p)
        else:
            q = p.clone().requires_grad_(True)
            _clamped(q, p_min).backward(gouts[l])
            want = q.grad
        assert torch.equal(gps[l], want), (l, float((gps[l] - want).abs().max()))
    # the same tensors through autograd
    leaves = [p.clone().requires_grad_(True) for p in ps]
    outs2 = prob_mask_gate_pyramid(leaves, gate_state(SEED, STEP), cfgs)
    torch.autograd.backward(list(outs2), gouts)
    for l in range(len(ps)):
        assert torch.equal(outs2[l], outs[l]) and torch.equal(leaves[l].grad, gps[l]), l


def test_masks_of_other_dtypes_and_ranks_enter_as_float(built_lib):
    from mga_yolo_amd import gate_state, prob_mask_gate_pyramid
    p = _inputs([(2, 1, 5, 3)], 0.0)[0]
    half = p.half()
    cfgs = _cfgs("gumbel", 1, 0.0)
    a = prob_mask_gate_pyramid([half.squeeze(1).requires_grad_(True)], gate_state(SEED, STEP), cfgs)[0]
    b = prob_mask_gate_pyramid([half.float()], gate_state(SEED, STEP), cfgs)[0]
    assert a.dtype == torch.float32 and a.shape == (2, 1, 5, 3) and torch.equal(a, b) and a.requires_grad
    with pytest.raises(RuntimeError, match="state"):
        prob_mask_gate_pyramid([p], torch.zeros(4, dtype=torch.int32, device="cuda"), cfgs)
    with pytest.raises(RuntimeError):
        prob_mask_gate_pyramid([p, p], gate_state(), cfgs)


# ---- 5: graph replay of a gated PyramidPlan ---------------------------------------------------------------------------------------------
def _cbam(shapes, seed=0):
    from mga_yolo_amd import MaskCBAM
    blocks = []
    for l, (B, Cc, H, W) in enumerate(shapes):
        torch.manual_seed(seed + 10 + l)
        b = MaskCBAM(Cc)
        with torch.no_grad():
            b.beta.fill_(0.2 * (l - 1))
        blocks.append(b.cuda())
    return blocks


def test_a_captured_gated_plan_replays_with_fresh_noise(built_lib):
    from mga_yolo_amd import GateConfig
    from mga_yolo_amd.plan import PyramidPlan
    shapes = [(2, 16, 8, 8), (2, 32, 5, 3)]
    blocks = _cbam(shapes)
    gate = [GateConfig("gumbel", TAU, 0.05, THR)] * 2
    mk = lambda: PyramidPlan(shapes, [b.block_params() for b in blocks], [b.block_config() for b in blocks], gate=gate, seed=SEED)
    plan, eager = mk(), mk()
    g = torch.Generator().manual_seed(21)
    for l, (B, Cc, H, W) in enumerate(shapes):
        x, gy = torch.randn(B, Cc, H, W, generator=g), torch.randn(B, Cc, H, W, generator=g)
        lg = 0.5 + 0.6 * torch.randn(B, 1, H, W, generator=g)
        for p_ in (plan, eager):
            p_.x[l].copy_(x); p_.gy[l].copy_(gy); p_.logits[l].copy_(lg)
    assert plan.rng_state.tolist() == [SEED, 0, 0, 0]

    def step():
        plan.forward()
        plan.backward()
    graph = plan.capture(step)
    torch.cuda.synchronize()
    s = int(plan.rng_state[1])
    assert s >= 1 and plan.rng_state.tolist() == [SEED, s, 0, 0]     # the warm-up run drew noise; the capture itself runs nothing
    masks = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert plan.rng_state.tolist() == [SEED, s + r + 1, 0, 0]
        eager.rng_state.copy_(torch.tensor([SEED, s + r, 0, 0]))
        eager.forward()
        eager.backward()
        torch.cuda.synchronize()
        for l, shp in enumerate(shapes):
            want = _expected("gumbel", plan.logits[l], 0.05, SEED, s + r, l)[0]
            assert torch.equal(plan.mask[l], want), (r, l)           # the restatement at step s + r
            for name in ("mask", "y", "gx", "glogits"):
                assert torch.equal(getattr(plan, name)[l], getattr(eager, name)[l]), (r, l, name)
            assert bool((plan.glogits[l] != 0).any())
        masks.append([m.clone() for m in plan.mask])
    plan.check_handoff()
    for a in range(3):
        for b in range(a + 1, 3):
            assert not any(torch.equal(x, y) for x, y in zip(masks[a], masks[b]))


def test_a_plan_without_a_gate_is_todays_object(built_lib):
    from mga_yolo_amd.plan import PyramidPlan
    shapes = [(2, 16, 8, 8)]
    blocks = _cbam(shapes)
    plan = PyramidPlan(shapes, [b.block_params() for b in blocks], [b.block_config() for b in blocks])
    assert plan.gate is None and not any(hasattr(plan, n) for n in ("logits", "glogits", "msoft", "rng_state"))


# ---- 6: a gated SlicePlan against the module composition ---------------------------------------------------------------------------------
def _build(shapes, hidden, seed=0):
    """tests/test_gpu_slice_plan.py's recipe"""
    from mga_yolo_amd import MGAMaskHead
    heads = []
    for l, ((B, Cc, H, W), hid) in enumerate(zip(shapes, hidden)):
        torch.manual_seed(seed + l)
        h = MGAMaskHead(Cc, hid)
        h.proj[1].eps, h.proj[1].momentum = 1e-3, 0.03
        heads.append(h.cuda().train())
    return heads, _cbam(shapes, seed)


@pytest.mark.parametrize("mode", ["gumbel", "hard_st"])
@pytest.mark.parametrize("shapes,hidden,target_hw", [
    ([(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)], [16, 32, 64], None),
    ([(3, 64, 20, 12), (3, 128, 10, 6)], [16, 32], [(80, 48), (80, 48)]),
])
def test_gated_slice_plan_equals_the_module_composition(built_lib, shapes, hidden, target_hw, mode):
    from mga_yolo_amd import GateConfig, SegLossConfig, SegmentationLoss, kendall_combine, prob_mask_gate
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES, SlicePlan
    heads, blocks = _build(shapes, hidden)
    tau, p_min, thr, step = 0.5, 0.05, 0.5, 6
    gate = [GateConfig(mode, tau, p_min, thr)] * len(shapes)
    mk = lambda gt: SlicePlan(shapes, hidden, [b.block_params() for b in blocks], [b.block_config() for b in blocks],
                              [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in heads], target_hw=target_hw,
                              scale_weights=(1.0, 0.5, 2.0), gate=gt, seed=SEED)
    plan, plain = mk(gate), mk(None)
    assert "gate" in plan.launches()["forward"] and "gate" in plan.launches()["backward"] and "gate" not in plain.launches()["forward"]
    g = torch.Generator().manual_seed(21)
    xs, gys, tgs = [], [], []
    for l, (B, Cc, H, W) in enumerate(shapes):
        th, tw = (H, W) if target_hw is None else target_hw[l]
        xs.append(torch.randn(B, Cc, H, W, generator=g).cuda())
        gys.append(torch.randn(B, Cc, H, W, generator=g).cuda())
        tgs.append((torch.rand(B, 1, th, tw, generator=g) > 0.7).float().cuda())
        for p_ in (plan, plain):
            p_.x[l].copy_(xs[l]); p_.gy[l].copy_(gys[l]); p_.targets[l].copy_(tgs[l])
    det = torch.tensor([1.3, 0.7, 2.1]).cuda()
    lv = torch.tensor([0.3, -0.4]).cuda()
    for p_ in (plan, plain):
        p_.det_loss.copy_(det); p_.log_vars.copy_(lv)
    graph = plan.capture(plan.step)
    for rm, rv, nbt in plan.head_buffers:                          # capture's warm-up run was a training step too: start over
        rm.zero_(); rv.fill_(1.0); nbt.zero_()
    plan.cbam.rng_state.copy_(torch.tensor([SEED, step, 0, 0]))
    graph.replay()
    plain.step()
    torch.cuda.synchronize()
    plan.check_handoff()
    assert plan.cbam.rng_state.tolist() == [SEED, step + 1, 0, 0]
    # ---- the same slice through the modules + autograd, the gate on the restatement's uniforms ----------------------------------------
    for h in heads:
        h.proj[1].reset_running_stats()
    xl = [x.clone().requires_grad_(True) for x in xs]
    lvl = lv.clone().requires_grad_(True)
    logits = [h(x) for h, x in zip(heads, xl)]
    masks = []
    for l, m in enumerate(logits):
        u1, u2 = _uniforms(m.shape, SEED, step, l)
        masks.append(prob_mask_gate(m.float(), u1, u2, tau, p_min, thr, hard=mode == "hard_st"))
    ys = [b([x, m]) for b, x, m in zip(blocks, xl, masks)]
    crit = SegmentationLoss(SegLossConfig(scale_weights=(1.0, 0.5, 2.0)))
    seg_total, logs = crit({k: m for k, m in zip(("p3", "p4", "p5"), logits)}, tgs)
    total = kendall_combine(det, seg_total, lvl)
    torch.autograd.backward([total.sum()] + ys, [None] + gys)
    torch.cuda.synchronize()
    assert rel_err(plan.total, total) < 1e-6 and abs(float(plan.seg_out[0]) - logs["seg_total"]) < 1e-5
    assert rel_err(plan.g_log_vars, lvl.grad) < 1e-5
    for l in range(len(shapes)):
        differs = False
        assert plan.logits[l] is plan.cbam.logits[l] and plan.logits[l] is not plan.cbam.mask[l]
        assert rel_err(plan.logits[l], logits[l]) < 1e-6, l                   # the raw head output, which the loss reads ...
        assert rel_err(plan.cbam.mask[l], masks[l]) < 1e-6, l                 # ... and the gated one, which MaskCBAM reads
        assert rel_err(plan.y[l], ys[l]) < 1e-6, l
        assert rel_err(plan.gx[l], xl[l].grad) < 1e-5, l
        sd = dict(heads[l].named_parameters())
        for k, gq, g0 in zip(HEAD_PARAM_NAMES, plan.head_grads[l], plain.head_grads[l]):
            assert rel_err(gq, sd[k].grad) < 1e-5, (l, k)                     # the head's gradients include the gate's path
            differs = differs or not torch.equal(gq, g0)
        for (name, gq), p in zip(plan.cbam.named_param_grads(l).items(), blocks[l].block_params()):
            assert rel_err(gq, p.grad) < 1e-5, (l, name)
        assert rel_err(plan.head_buffers[l][0], heads[l].proj[1].running_mean) < 1e-6
        assert rel_err(plan.head_buffers[l][1], heads[l].proj[1].running_var) < 1e-6
        assert differs, l                                                     # ... and so differ from the plan without a gate
        assert torch.equal(plain.logits[l], plan.logits[l])                   # (whose heads saw the same features)
