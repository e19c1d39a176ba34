"""The static plans of every block in both feature layouts, on the device (mga_yolo_amd/plan.py, slice.py), each against this package's own
autograd call of the same kernels -- which the other GPU tests pin to the reference's goldens and oracles:
  1. SpadePyramidPlan == mask_spade_pyramid, bit for bit (the MaskSPADE kernels are fixed-order);
  2. the mask resample (include/mgaresample.h) against F.interpolate and its autograd in fp64 on the host, and inside a plan (mask_hw=);
  3. PyramidPlan.create(channels_last=True) == mask_cbam_pyramid on channels_last inputs, bit for bit;
  4. SlicePlan.create(block=, channels_last=) == the same slice composed from the modules, as tests/test_gpu_slice_plan.py does for MaskCBAM;
  5. half-precision features against the fp32 plan."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_replays as R  # noqa: E402
import resample_oracle as RO  # noqa: E402
import spade_plan as P  # noqa: E402
from test_gpu_spade import dev, live_case  # noqa: E402,F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _fmt(cl):
    return CL if cl else torch.contiguous_format


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. SpadePyramidPlan == mask_spade_pyramid
# ------------------------------------------------------------------------------------------------------------------------------------
ROWS = [P.case(2, 32, 16, 8), P.case(2, 48, 30, 22), P.case(2, 64, 20, 44)]     # in / hidden 16; bn / hidden 48, eps 1e-3, momentum 0.3; in / hidden 32
_spade_cache = {}


def _spade_inputs(dtype):
    """The three rows' modules and inputs (seeds of tests/spade_plan.py: no ReLU pre-activation near zero), features rounded to dtype."""
    key = ("in", dtype)
    if key not in _spade_cache:
        out = []
        for c in ROWS:
            m, x, mask, gy = live_case(c.B, c.C, c.H, c.W, c.norm, seed=c.seed, hidden=c.hidden)
            m.norm.eps = c.eps
            if c.norm == "bn":
                m.norm.momentum = c.momentum
            out.append((m.cuda().train(), x.to(dtype).cuda(), mask.cuda(), gy.to(dtype).cuda()))
        _spade_cache[key] = out
    return _spade_cache[key]


def _fresh_running(m):
    if not m.spade_config().bn:
        return None
    C_ = m.cfg.channels
    return (torch.zeros(C_, device="cuda"), torch.ones(C_, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"))


def _spade_autograd(dtype, variant, masks=None):
    """One forward + backward of mask_spade_pyramid on NCHW inputs: computed once per (dtype, variant) and shared.
    variant: 'full' | 'nomask' | 'nogmask'; masks: per level a replacement mask (another resolution) or None."""
    from mga_yolo_amd import mask_spade_pyramid
    key = ("ref", dtype, variant, masks is not None)
    if key in _spade_cache:
        return _spade_cache[key]
    levels, xs, ms, ps, runs, gys = [], [], [], [], [], []
    for l, (m, x, mask, gy) in enumerate(_spade_inputs(dtype)):
        x = x.clone().requires_grad_(True)
        mk = mask if masks is None or masks[l] is None else masks[l]
        mk = None if variant == "nomask" else mk.clone().requires_grad_(variant == "full")
        p = [t.detach().clone().requires_grad_(True) for t in m.spade_params()]
        run = _fresh_running(m)
        levels.append((x, mk, p, m.spade_config(), run))
        xs.append(x); ms.append(mk); ps.append(p); runs.append(run); gys.append(gy)
    ys = mask_spade_pyramid(levels)
    torch.autograd.backward(list(ys), gys)
    torch.cuda.synchronize()
    ref = dict(y=[y.detach() for y in ys], gx=[x.grad for x in xs], gmask=[None if m is None else m.grad for m in ms],
               pg=[[t.grad for t in p] for p in ps], run=runs)
    _spade_cache[key] = ref
    return ref


def _spade_plan(dtype, cl, variant, mask_hw=None):
    from mga_yolo_amd import SpadePyramidPlan
    ins = _spade_inputs(dtype)
    plan = SpadePyramidPlan([tuple(x.shape) for _, x, _, _ in ins], [m.spade_params() for m, _, _, _ in ins],
                            [m.spade_config() for m, _, _, _ in ins], dtype=dtype, channels_last=cl, with_mask=variant != "nomask",
                            want_gmask=variant == "full", mask_hw=mask_hw)
    for l, (_, x, mask, gy) in enumerate(ins):
        plan.x[l].copy_(x); plan.gy[l].copy_(gy)
        if variant != "nomask":
            plan.mask[l].copy_(mask)
        assert plan.x[l].is_contiguous(memory_format=_fmt(cl))
    return plan


@pytest.mark.parametrize("variant", ["full", "nomask", "nogmask"])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_spade_plan_equals_the_autograd_call_bit_for_bit(dev, dtype, cl, variant):
    """Both layouts against ONE NCHW reference: the channels_last plan therefore equals the NCHW plan bit for bit as well."""
    ref = _spade_autograd(dtype, variant)
    plan = _spade_plan(dtype, cl, variant)
    plan.forward(); plan.backward()
    torch.cuda.synchronize()
    for l in range(plan.n):
        assert plan.y[l].is_contiguous(memory_format=_fmt(cl)) and plan.gx[l].is_contiguous(memory_format=_fmt(cl))
        assert torch.equal(plan.y[l], ref["y"][l]) and torch.equal(plan.gx[l], ref["gx"][l]), l
        if variant == "full":
            assert torch.equal(plan.gmask[l], ref["gmask"][l]), l
        else:
            assert plan.gmask[l] is None
        if variant != "nomask":
            for name, g, want in zip(plan.named_param_grads(l), plan.param_grads[l], ref["pg"][l]):
                assert torch.equal(g, want), (l, name)
        if ref["run"][l] is not None:
            for got, want in zip(plan.running[l], ref["run"][l]):
                assert torch.equal(got, want), l
            assert int(plan.running[l][2]) == 1


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the mask resample
# ------------------------------------------------------------------------------------------------------------------------------------
PAIRS = [((7, 5), (16, 12)), ((40, 24), (10, 6)), ((13, 17), (16, 12)), ((1, 9), (4, 9)), ((6, 1), (3, 5)), ((5, 3), (1, 1))]
FLOOR = 1e-6     # the project's fp32 forward bar (tests/test_gpu_slice_plan.py)


def _host_reference(src, gout, out_hw):
    """F.interpolate and its autograd on the host: (fp64 forward, fp64 backward, torch's own fp32 forward, torch's own fp32 backward)"""
    res = []
    for dt in (torch.float64, torch.float32):
        s = src.detach().clone().to(dt).requires_grad_(True)              # (a copy: .to() of an fp32 tensor is the tensor itself)
        d = F.interpolate(s, size=out_hw, mode="bilinear", align_corners=False)
        d.backward(gout.to(dt))
        res += [d.detach(), s.grad]
    return res


def _bar(own, ref64):
    """max(1e-6, 4 x the error of torch's own fp32 host result against the same fp64 result)"""
    return max(FLOOR, 4.0 * rel_err(own, ref64))


def _resample(direction, src, dst, in_hw, out_hw):
    from mga_yolo_amd import _binding, _lib
    lv = (_lib.ResampleLevel * 1)()
    _binding.fill_resample(lv[0], src, dst, in_hw, out_hw)
    _binding.call(f"mgaspade_resample_{direction}", src.device, lv, 1)


@pytest.mark.parametrize("in_hw,out_hw", PAIRS, ids=[f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in PAIRS])
def test_resample_against_interpolate_in_fp64(dev, in_hw, out_hw):
    B = 3
    g = torch.Generator().manual_seed(7)
    src = torch.randn(B, 1, *in_hw, generator=g)
    gout = torch.randn(B, 1, *out_hw, generator=g)
    f64, b64, f32, b32 = _host_reference(src, gout, out_hw)
    sd, gd = src.cuda(), gout.cuda()
    dst = torch.full((B, 1, *out_hw), float("nan"), device="cuda")
    gsrc = [torch.full((B, 1, *in_hw), float("nan"), device="cuda") for _ in range(2)]
    _resample("forward", sd, dst, in_hw, out_hw)
    for t in gsrc:                                                        # two runs of the backward
        _resample("backward", gd, t, in_hw, out_hw)
    torch.cuda.synchronize()
    ef, eb = rel_err(dst, f64), rel_err(gsrc[0], b64)
    print(f"resample {in_hw}->{out_hw}: forward {ef:.3e} (bar {_bar(f32, f64):.3e}) backward {eb:.3e} (bar {_bar(b32, b64):.3e})")
    assert ef <= _bar(f32, f64) and eb <= _bar(b32, b64)
    assert torch.equal(gsrc[0], gsrc[1])                                  # gather form, fixed order: the same bits
    # the adjoint identity <R s, g> = <s, R^T g> in fp64 on the device results (the two kernels share one index function)
    assert abs(float((dst.double() * gd.double()).sum() - (sd.double() * gsrc[0].double()).sum())) <= 1e-5 * float(dst.abs().sum() + 1.0)


def test_resample_of_several_levels_in_one_call(dev):
    """Every pair as one level of ONE call each way (odd and 16-byte rows side by side) equals the single calls bit for bit."""
    from mga_yolo_amd import _binding, _lib
    B = 3
    g = torch.Generator().manual_seed(8)
    n = len(PAIRS)
    srcs = [torch.randn(B, 1, *a, generator=g).cuda() for a, _ in PAIRS]
    gouts = [torch.randn(B, 1, *b, generator=g).cuda() for _, b in PAIRS]
    dsts = [torch.empty(B, 1, *b, device="cuda") for _, b in PAIRS]
    gsrcs = [torch.empty(B, 1, *a, device="cuda") for a, _ in PAIRS]
    fw, bw = (_lib.ResampleLevel * n)(), (_lib.ResampleLevel * n)()
    for l, (a, b) in enumerate(PAIRS):
        _binding.fill_resample(fw[l], srcs[l], dsts[l], a, b)
        _binding.fill_resample(bw[l], gouts[l], gsrcs[l], a, b)
    _binding.call("mgaspade_resample_forward", srcs[0].device, fw, n)
    _binding.call("mgaspade_resample_backward", srcs[0].device, bw, n)
    for l, (a, b) in enumerate(PAIRS):
        d1, g1 = torch.empty_like(dsts[l]), torch.empty_like(gsrcs[l])
        _resample("forward", srcs[l], d1, a, b)
        _resample("backward", gouts[l], g1, a, b)
        torch.cuda.synchronize()
        assert torch.equal(d1, dsts[l]) and torch.equal(g1, gsrcs[l]), l


def test_spade_plan_with_masks_at_another_resolution(dev):
    """mask_hw=[(10,6), None, (16,12)]: the plan resamples in its own launches what the autograd call resamples with torch's operator.
    The two resamples differ by rounding only, so every result is held to the resample's own bar: max(1e-6, 4 x the error of torch's fp32
    host resample of these masks against fp64) -- the larger of the forward's and the backward's figure over the two levels."""
    mask_hw = [(10, 6), None, (16, 12)]
    g = torch.Generator().manual_seed(9)
    ins = _spade_inputs(torch.float32)
    small = [None if hw is None else torch.randn(x.shape[0], 1, *hw, generator=g) for hw, (_, x, _, _) in zip(mask_hw, ins)]
    bar = FLOOR
    for s, (_, x, _, _) in zip(small, ins):
        if s is not None:
            out_hw = tuple(x.shape[-2:])
            f64, b64, f32, b32 = _host_reference(s, torch.randn(s.shape[0], 1, *out_hw, generator=g), out_hw)
            bar = max(bar, _bar(f32, f64), _bar(b32, b64))
    ref = _spade_autograd(torch.float32, "full", [None if s is None else s.cuda() for s in small])
    plan = _spade_plan(torch.float32, False, "full", mask_hw)
    for l, s in enumerate(small):
        if s is not None:
            plan.mask[l].fill_(float("nan"))                              # the plan's forward must overwrite it from mask_src
            plan.mask_src[l].copy_(s)
    graph = plan.capture(lambda: (plan.forward(), plan.backward()))     # the resample launches are capturable like the rest
    for run in plan.running:
        if run[0] is not None:
            run[0].zero_(); run[1].fill_(1.0); run[2].zero_()
    graph.replay()
    torch.cuda.synchronize()
    report = []
    for l in range(plan.n):
        got = dict(y=plan.y[l], gx=plan.gx[l], gmask=plan.gmask[l] if small[l] is None else plan.gmask_src[l])
        want = dict(y=ref["y"][l], gx=ref["gx"][l], gmask=ref["gmask"][l])
        got.update(zip(plan.named_param_grads(l), plan.param_grads[l])); want.update(zip(plan.named_param_grads(l), ref["pg"][l]))
        for k in got:
            assert got[k] is not None and want[k] is not None and got[k].shape == want[k].shape, (l, k)
            e = rel_err(got[k], want[k])
            print(f"mask_hw level {l} {k}: {e:.3e} (bar {bar:.3e})")
            if not e <= bar:
                report.append((l, k, e))
    assert not report, (report, bar)
    assert torch.equal(plan.y[1], ref["y"][1]) and torch.equal(plan.gmask[1], ref["gmask"][1])     # the level without a resample: the same bits


def test_spade_plan_with_a_mask_at_eight_times_the_level(dev):
    """mask_hw=[(8H, 8W), None, None], the workload's ratio at P3.  After a captured replay the plan's resampled mask and its dL/dmask at
    the mask's own resolution are the bits of stand-alone calls of the two entry points on the plan's tensors, every element is within
    the resample's own bar (tests/resample_oracle.py: K x terms, exactly 0 where the terms are 0), and the 60 of 64 source
    pixels per 8 x 8 cell that no destination reads get a gradient of exactly 0."""
    ins = _spade_inputs(torch.float32)
    B, _, H, W = ins[0][1].shape
    big = (8 * H, 8 * W)
    plan = _spade_plan(torch.float32, False, "full", [big, None, None])
    plan.mask_src[0].copy_(torch.randn(B, 1, *big, generator=torch.Generator().manual_seed(11)))
    graph = plan.capture(lambda: (plan.forward(), plan.backward()))
    plan.mask[0].fill_(float("nan")); plan.gmask_src[0].fill_(float("nan"))   # the replay must write both
    graph.replay()
    torch.cuda.synchronize()
    alone_f, alone_b = torch.full_like(plan.mask[0], float("nan")), torch.full_like(plan.gmask_src[0], float("nan"))
    _resample("forward", plan.mask_src[0], alone_f, big, (H, W))
    _resample("backward", plan.gmask[0], alone_b, big, (H, W))
    torch.cuda.synchronize()
    assert torch.equal(plan.mask[0], alone_f) and torch.equal(plan.gmask_src[0], alone_b)
    op = RO.Resample(big, (H, W))
    kf, kb = RO.load_k()
    rf, _, nzf, badf = RO.ratio(plan.mask[0], *op.forward(plan.mask_src[0]))
    rb, zb, nzb, badb = RO.ratio(plan.gmask_src[0], *op.backward(plan.gmask[0]))
    print(f"mask_hw 8x: forward {rf:.3f} (K {kf:.3f}) backward {rb:.3f} (K {kb:.3f}), {zb} of {plan.gmask_src[0].numel()} zero-terms elements")
    assert badf == 0 and badb == 0 and nzf == 0 and nzb == 0 and rf <= kf and rb <= kb
    assert bool(torch.isfinite(plan.gmask[0]).all()) and float(plan.gmask[0].abs().max()) > 0
    assert float((plan.gmask_src[0] == 0).double().mean()) >= 0.90


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. PyramidPlan.create(channels_last=True) == mask_cbam_pyramid on channels_last inputs
# ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)]
HIDDEN = [16, 32, 64]


def _cbam_blocks(shapes=SHAPES, seed=0):
    from mga_yolo_amd import MaskCBAM
    blocks = []
    for l, (_, C_, _, _) in enumerate(shapes):
        torch.manual_seed(seed + 10 + l)
        b = MaskCBAM(C_)
        with torch.no_grad():
            b.beta.fill_(0.2 * (l - 1))
        blocks.append(b.cuda())
    return blocks


@pytest.mark.parametrize("dtype,gated", [(torch.float32, False), (torch.bfloat16, False), (torch.float32, True)], ids=["fp32", "bf16", "fp32-gate"])
def test_cbam_plan_channels_last_equals_the_autograd_call_bit_for_bit(built_lib, dtype, gated):
    from mga_yolo_amd import GateConfig, PyramidPlan, gate_state, mask_cbam_pyramid, prob_mask_gate_pyramid
    blocks = _cbam_blocks()
    gate = [GateConfig("deterministic")] * 3 if gated else None
    plan = PyramidPlan.create(SHAPES, [b.block_params() for b in blocks], [b.block_config() for b in blocks], dtype=dtype, channels_last=True,
                              gate=gate)
    g = torch.Generator().manual_seed(5)
    xs, ms, gys = [], [], []
    for l, (B, C_, H, W) in enumerate(SHAPES):
        xs.append(torch.randn(B, C_, H, W, generator=g).to(dtype).cuda().contiguous(memory_format=CL))
        ms.append((torch.rand(B, 1, H, W, generator=g) * 1.4 - 0.2).cuda() if gated else torch.randn(B, 1, H, W, generator=g).cuda())
        gys.append(torch.randn(B, C_, H, W, generator=g).to(dtype).cuda().contiguous(memory_format=CL))
        plan.x[l].copy_(xs[l]); plan.gy[l].copy_(gys[l]); (plan.logits if gated else plan.mask)[l].copy_(ms[l])
        assert plan.x[l].is_contiguous(memory_format=CL) and not plan.x[l].is_contiguous()
    plan.forward(); plan.backward()
    plan.check_handoff()                                                  # synchronises; no hand-off ran, no status word is set
    assert not plan.gate_active() and not plan.fold_active()
    xl = [x.clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs]
    ml = [m.clone().requires_grad_(True) for m in ms]
    pl = [[p.detach().clone().requires_grad_(True) for p in b.block_params()] for b in blocks]
    masks = prob_mask_gate_pyramid(ml, gate_state(0, 0), gate) if gated else ml
    ys = mask_cbam_pyramid([(x, m, p, b.block_config()) for x, m, p, b in zip(xl, masks, pl, blocks)])
    torch.autograd.backward(list(ys), gys)
    torch.cuda.synchronize()
    for l in range(3):
        assert plan.y[l].is_contiguous(memory_format=CL) and plan.gx[l].is_contiguous(memory_format=CL)
        assert torch.equal(plan.y[l], ys[l]) and torch.equal(plan.gx[l], xl[l].grad), l
        assert torch.equal((plan.glogits if gated else plan.gmask)[l], ml[l].grad), l
        for (name, gq), p in zip(plan.named_param_grads(l).items(), pl[l]):
            assert torch.equal(gq, p.grad), (l, name)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. SlicePlan.create(block=, channels_last=) == the module composition
# ------------------------------------------------------------------------------------------------------------------------------------
_build, _block_args = R.build_modules, R.block_args     # the module-side reference lives in tests/plan_replays.py, shared with test_gpu_plan_replays.py


def _make_slice(block, cl, shapes, hidden, heads, blocks, **kw):
    from mga_yolo_amd import SlicePlan
    params, cfgs, running = _block_args(block, blocks)
    return SlicePlan.create(shapes, hidden, params, cfgs, [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in heads],
                            block=block, channels_last=cl, block_running=running, scale_weights=(1.0, 0.5, 2.0), **kw)


def _reset_running(plan):
    for rm, rv, nbt in plan.head_buffers:
        rm.zero_(); rv.fill_(1.0); nbt.zero_()
    if plan.block_name == "spade":
        for rm, rv, nbt in plan.block.running:
            if rm is not None:
                rm.zero_(); rv.fill_(1.0); nbt.zero_()


COMBOS = [("eca", False), ("eca", True), ("spade", False), ("spade", True), ("cbam", True)]
SLICE_ROWS = [
    ([(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)], [16, 32, 64], None, "nearest"),
    ([(3, 64, 20, 12), (3, 128, 10, 6)], [16, 32], [(80, 48), (80, 48)], "bilinear"),     # full-resolution soft targets, read bilinearly
]


@pytest.mark.parametrize("shapes,hidden,target_hw,resize", SLICE_ROWS, ids=["p3p4p5", "two-levels-bilinear"])
@pytest.mark.parametrize("block,cl", COMBOS, ids=[f"{b}-{'channels_last' if c else 'nchw'}" for b, c in COMBOS])
def test_slice_plan_equals_the_module_composition(built_lib, block, cl, shapes, hidden, target_hw, resize):
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES
    heads, blocks = _build(block, shapes, hidden)
    plan = _make_slice(block, cl, shapes, hidden, heads, blocks, target_hw=target_hw, target_resize=resize)
    g = torch.Generator().manual_seed(21)
    xs, gys, tgs = [], [], []
    for l, (B, C_, H, W) in enumerate(shapes):
        th, tw = (H, W) if target_hw is None else target_hw[l]
        xs.append(torch.randn(B, C_, H, W, generator=g).cuda().contiguous(memory_format=_fmt(cl)))
        gys.append(torch.randn(B, C_, H, W, generator=g).cuda().contiguous(memory_format=_fmt(cl)))
        t = torch.rand(B, 1, th, tw, generator=g)
        tgs.append((t if resize == "bilinear" else (t > 0.7).float()).cuda())                 # soft targets in [0,1] for the bilinear row
        plan.x[l].copy_(xs[l]); plan.gy[l].copy_(gys[l]); plan.targets[l].copy_(tgs[l])
        assert plan.x[l].is_contiguous(memory_format=_fmt(cl))
    det = torch.tensor([1.3, 0.7, 2.1]).cuda()
    lv = torch.tensor([0.3, -0.4]).cuda()
    plan.det_loss.copy_(det); plan.log_vars.copy_(lv)
    graph = plan.capture(plan.step)
    _reset_running(plan)                                                  # capture's warm-up run was a training step too: start over
    graph.replay()
    torch.cuda.synchronize()
    plan.check_handoff()
    # ---- the same slice through the modules + autograd --------------------------------------------------------------------------------
    for h in heads:
        h.proj[1].reset_running_stats()
    c = R.module_composition(heads, blocks, xs, gys, tgs, det, lv, resize)     # (sets MGA_PROB_MODE for the bilinear row's loss)
    xl, lvl, logits, ys, total, logs = c.xl, c.lvl, c.logits, c.ys, c.total, c.logs
    assert rel_err(plan.total, total) < 1e-6 and abs(float(plan.seg_out[0]) - logs["seg_total"]) < 1e-5
    assert rel_err(plan.g_log_vars, lvl.grad) < 1e-5
    params, _, running = _block_args(block, blocks)
    for l in range(len(shapes)):
        assert rel_err(plan.logits[l], logits[l]) < 1e-6 and rel_err(plan.y[l], ys[l]) < 1e-6, l
        assert plan.y[l].is_contiguous(memory_format=_fmt(cl)) and plan.gx[l].is_contiguous(memory_format=_fmt(cl))
        assert rel_err(plan.gx[l], xl[l].grad) < 1e-5, l                 # the block's part + the head's part, accumulated in the GEMM epilogue
        sd = dict(heads[l].named_parameters())
        for k, gq in zip(HEAD_PARAM_NAMES, plan.head_grads[l]):
            assert rel_err(gq, sd[k].grad) < 1e-5, (l, k)
        for (name, gq), p in zip(plan.block.named_param_grads(l).items(), params[l]):
            assert rel_err(gq, p.grad) < 1e-5, (l, name)
        assert rel_err(plan.head_buffers[l][0], heads[l].proj[1].running_mean) < 1e-6
        assert rel_err(plan.head_buffers[l][1], heads[l].proj[1].running_var) < 1e-6
        if running is not None and running[l] is not None:
            assert rel_err(plan.block.running[l][0], running[l][0]) < 1e-6 and rel_err(plan.block.running[l][1], running[l][1]) < 1e-6
            assert int(plan.block.running[l][2]) == int(running[l][2]) == 1
    # replaying the graph again is a new training step on the same inputs: same outputs, running statistics move on
    rm = plan.head_buffers[0][0].clone()
    y0 = plan.y[0].clone()
    srm = plan.block.running[1][0].clone() if block == "spade" else None
    graph.replay(); torch.cuda.synchronize()
    assert torch.equal(plan.y[0], y0) and not torch.equal(plan.head_buffers[0][0], rm)
    assert int(plan.head_buffers[0][2]) == 2
    if block == "spade":
        assert not torch.equal(plan.block.running[1][0], srm) and int(plan.block.running[1][2]) == 2


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. half precision
# ------------------------------------------------------------------------------------------------------------------------------------
def _relu_flips(plan, ref):
    """MaskSPADE levels: how many pre-activations of the shared conv, relu(conv3x3(sigmoid(logits))), have another sign in `plan` than in `ref`
    (recomputed with torch from each plan's own logits).  A flipped branch moves dL/dh at that place from 0 to its full value."""
    out = []
    for l in range(plan.n):
        w0, b0 = ref.block.params[l][:2]
        pre = [F.conv2d(torch.sigmoid(p_.logits[l]), w0, b0, padding=1) for p_ in (ref, plan)]
        out.append(int(((pre[0] > 0) != (pre[1] > 0)).sum()))
    return out


def _pin_relu_branches(blocks, margin=0.25):
    """Give every hidden channel of MaskSPADE's shared conv a bias whose magnitude exceeds anything the conv can add: the conv's input is
    sigmoid(mask) in (0, 1), so |conv3x3| < sum_k |w0[c, k]|, and with |b0[c]| = that sum + margin the pre-activation of channel c keeps the
    sign of b0[c] at every pixel, at least `margin` from zero, whatever the mask is.  Signs alternate: even channels pass (h varies with the
    mask and carries gradient), odd channels are cut."""
    with torch.no_grad():
        for b in blocks:
            w0, b0 = b.shared[0].weight, b.shared[0].bias
            sign = torch.ones_like(b0)
            sign[1::2] = -1.0
            b0.copy_(sign * (w0.abs().sum(dim=(1, 2, 3)) + margin))


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)], ids=["fp16", "bf16"])
@pytest.mark.parametrize("block", ["spade", "eca"])
def test_slice_plan_with_half_precision_features(built_lib, block, dtype, tol):
    """Against the fp32 plan on the same rounded inputs, at the tolerances of tests/test_gpu_slice_plan.py's half-precision test: 4e-3 (fp16) /
    3e-2 (bf16), twice that for gradients and the bucket.

    The two plans do not see the same mask: the mask is the heads' logits, which half-precision features move (by 2e-4 in fp16, 2e-3 in
    bf16, measured).  MaskSPADE puts a ReLU behind a conv of that mask, and a tolerance that comes from the precision of a number format can
    only bound a function that is continuous between the two inputs: with the modules' initial zero biases, a handful of the 28 000
    pre-activations lie closer to zero than the logits move and take the other branch, and everything behind the ReLU's derivative then
    differs by a branch, not by a rounding (measured so: 2 pre-activations of another sign at level 0 in fp16 gave dL/dmask 3.4e-2 and gx
    3.6e-2 off there while the other levels, without one, sat at 5e-4 to 1.4e-3).  No choice of seed keeps 28 000 values further
    from zero than the bar lets the mask move, so the inputs fix the branches instead (_pin_relu_branches): the comparison is then one of
    roundings alone, which is what the bars are for.  The test asserts that no pre-activation changes sign and prints every figure.  Branches
    that switch from pixel to pixel are covered bit for bit by the tests above, where both sides see the same mask."""
    heads, blocks = _build(block, SHAPES, HIDDEN)
    if block == "spade":
        _pin_relu_branches(blocks)
    ref, plan = (_make_slice(block, False, SHAPES, HIDDEN, heads, blocks, dtype=dt) for dt in (torch.float32, dtype))
    assert plan.x[0].dtype == dtype and plan.gx[0].dtype == dtype and plan.logits[0].dtype == torch.float32
    g = torch.Generator().manual_seed(33)
    for l, (B, C_, H, W) in enumerate(SHAPES):
        x = torch.randn(B, C_, H, W, generator=g).to(dtype)
        gy = torch.randn(B, C_, H, W, generator=g).to(dtype)
        t = (torch.rand(B, 1, H, W, generator=g) > 0.7).float()
        for p_ in (ref, plan):
            p_.x[l].copy_(x); p_.gy[l].copy_(gy); p_.targets[l].copy_(t)
    for p_ in (ref, plan):
        p_.det_loss.copy_(torch.tensor([1.3, 0.7, 2.1])); p_.log_vars.copy_(torch.tensor([0.3, -0.4]))
        p_.step()
    torch.cuda.synchronize()
    report = []

    def check(name, got, want, bar):
        e = rel_err(got, want)
        print(f"{block} {dtype} {name}: {e:.3e} (bar {bar:.1e})")
        if not e < bar:
            report.append((name, e))
    check("total", plan.total, ref.total, tol)
    for l in range(3):
        check(f"logits{l}", plan.logits[l], ref.logits[l], tol)
        check(f"y{l}", plan.y[l].float(), ref.y[l], tol)
        check(f"gx{l}", plan.gx[l].float(), ref.gx[l], 2 * tol)
    check("grad_bucket", plan.grad_bucket, ref.grad_bucket, 2 * tol)
    if block == "spade":
        flips = _relu_flips(plan, ref)
        print(f"{block} {dtype} ReLU pre-activations of another sign per level: {flips}; dL/dmask: "
              f"{[f'{rel_err(plan.block.gmask[l], ref.block.gmask[l]):.3e}' for l in range(3)]}")
        assert flips == [0, 0, 0], flips                               # the inputs' own condition: both plans took the same branches
        for l in range(3):                                             # and the passing channels do vary with the mask
            h = F.relu(F.conv2d(torch.sigmoid(ref.logits[l]), *ref.block.params[l][:2], padding=1))
            assert float(h[:, 0::2].std()) > 1e-3 and float(h[:, 1::2].abs().max()) == 0.0, l
    assert not report, report
    g2 = plan.capture(plan.step)                                       # graph-capturable like the fp32 plan
    g2.replay(); torch.cuda.synchronize()
