"""MaskSPADE on channels_last features (MGASPADE_LAYOUT_NHWC, csrc/spade_nhwc.cuh and the NHWC instantiations of csrc/spade.cuh).

The rule under test: a channels_last level gives, bit for bit, what the same data gives as an NCHW level -- every output, gradient and
running statistic, every element type and norm mode, with and without a mask.  The NCHW kernels are pinned to the fp64 oracle and the
goldens by tests/test_gpu_spade.py and tests/test_gpu_spade_paths.py; three rows are compared with the oracle here as well (the
project's standing bars, rel_err <= 1e-4 and elem_err < 1e-3), so that this file does not rest on the NCHW kernels alone.  The shapes are
the rows of tests/spade_plan.py: the smallest at which these kernels take each of their paths."""
import os
import sys

import pytest
import torch

from conftest import rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spade_plan as P  # noqa: E402
from test_gpu_spade import ELEM, KEYS, TOL, dev, live_case, oracle_of, run  # noqa: E402,F401  (dev: the module's device fixture)
from test_gpu_spade_paths import check_fp32, forward_peak, inputs, oracle, run_with  # noqa: E402  (oracle: one cache for both files)

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _is_cl(t):
    return t.dim() == 4 and t.is_contiguous(memory_format=CL) and not t.is_contiguous()


def cl(t):
    return t.contiguous(memory_format=CL)


def first_difference(c, name, a, b):
    """Where two tensors that should be equal first differ; for a feature- or mask-shaped one its tile and place in the tile."""
    if a.shape != b.shape:
        return f"{name}: shapes {tuple(a.shape)} / {tuple(b.shape)}"
    idx = (a != b).nonzero()
    if not len(idx):
        return None
    at = tuple(int(i) for i in idx[0])
    msg = f"{name}: {len(idx)} of {a.numel()} differ, first at {at}: {a[at].item()!r} / {b[at].item()!r}"
    if a.dim() == 4 and tuple(a.shape[-2:]) == (c.H, c.W):
        (ty, tx), (r, col) = P.locate(c.H, c.W, at[2], at[3])
        t = P.tiling(c.H, c.W)
        msg += f" = (b,c,y,x); tile (ty,tx) = ({ty},{tx}) of {t.tiles_y}x{t.tiles_x} tiles of {t.TH} rows x {t.TW} columns, row {r} column {col} of the tile"
    return msg


def both_layouts(dev, c, dtype=torch.float32, masked=True, train=True):
    """The row's module and data run as NCHW and as channels_last (x and gy both), from the same initial state ->
    (NCHW results, channels_last results); the module's buffers after the step are among them."""
    m, x, mask, gy = inputs(c, dtype)
    m = m.to(dev).train(train)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    xd, md, gd = x.to(dev), (mask.to(dev) if masked else None), gy.to(dev)
    out = []
    for conv in (lambda t: t, cl):
        m.load_state_dict(state)
        m.zero_grad()
        got = run(m, conv(xd), md, conv(gd))
        got.update({k: v.clone() for k, v in m.state_dict().items() if k.split(".")[-1] in BUFFERS})
        got["params_without_grad"] = [k for k, p in m.named_parameters() if p.grad is None]
        out.append(got)
    return out


def assert_same_bits(c, a, b, keys=None):
    report = []
    for k in keys or [k for k in a if k != "params_without_grad"]:
        if a[k] is None or b[k] is None:
            if a[k] is not b[k]:
                report.append(f"{k}: one run has no value")
            continue
        d = first_difference(c, k, a[k].cpu(), b[k].cpu())
        if d:
            report.append(d)
    assert not report, "\n".join([c.what] + report)


@pytest.mark.parametrize("c", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_every_row_bit_for_bit(dev, c):
    base, got = both_layouts(dev, c)
    assert base["y"].is_contiguous() and base["gx"].is_contiguous()
    assert _is_cl(got["y"]) and _is_cl(got["gx"])
    assert set(got) == set(base) and all(k in got for k in ["y", "gx", "gmask"] + KEYS)
    if c.norm == "bn":
        assert all(any(k.endswith(b) for k in got) for b in BUFFERS) and int(got["norm.num_batches_tracked"]) == 1
    assert_same_bits(c, base, got)


ORACLE = [(2, 48, 30, 22), (2, 80, 60, 10), (3, 1024, 32, 20)]


@pytest.mark.parametrize("shape", ORACLE, ids=[P.case_id(P.case(*s)) for s in ORACLE])
def test_channels_last_rows_against_the_oracle(dev, shape):
    c = P.case(*shape)
    m, x, mask, gy = inputs(c)
    want, ctx = oracle(c)
    m = m.to(dev)
    got = run(m, cl(x.to(dev)), mask.to(dev), cl(gy.to(dev)))
    assert _is_cl(got["y"]) and _is_cl(got["gx"])
    report = check_fp32(c, got, want, ["y", "gx", "gmask"] + KEYS, " channels_last")
    if c.norm == "bn":
        for k, w in zip(("running_mean", "running_var"), ctx["new_running"]):
            r = rel_err(getattr(m.norm, k), w)
            print(f"{P.case_id(c)} {k} rel_err {r:.3e}")
            if not r <= TOL:
                report.append(f"{k} {r:.3e}")
    assert not report, "\n".join([c.what] + report)


HALF = [(2, 48, 30, 22), (2, 80, 60, 10), (2, 16, 1, 37)]


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", HALF, ids=[P.case_id(P.case(*s)) for s in HALF])
def test_half_precision_rows_bit_for_bit(dev, shape, dtype):
    c = P.case(*shape)
    base, got = both_layouts(dev, c, DTYPES[dtype])
    assert got["y"].dtype == DTYPES[dtype] and _is_cl(got["y"]) and _is_cl(got["gx"])
    assert_same_bits(c, base, got)


NOMASK = P.Case(3, 48, 17, 23, "in", 16, 12, 1e-6, 0.1, *([None] * 10), "no mask: statistics and the two element-wise kernels alone")


@pytest.mark.parametrize("norm,train", [("in", True), ("bn", True), ("bn", False)])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_no_mask_path_bit_for_bit(dev, norm, train, dtype):
    c = NOMASK._replace(norm=norm)
    base, got = both_layouts(dev, c, DTYPES[dtype], masked=False, train=train)
    assert _is_cl(got["y"]) and _is_cl(got["gx"])
    assert len(got["params_without_grad"]) == len(KEYS) == len(base["params_without_grad"])
    if norm == "bn":
        assert int(got["norm.num_batches_tracked"]) == (1 if train else 0)
    assert_same_bits(c, base, got)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_backward_variants_bit_for_bit(dev, dtype):
    c = P.case(2, 80, 60, 10)
    m, x, mask, gy = inputs(c, DTYPES[dtype])
    m = m.to(dev)
    xd, md, gd = x.to(dev), mask.to(dev), gy.to(dev)
    for x_grad, mask_grad in ((True, False), (False, True), (False, False)):
        base = {k: (None if v is None else v.clone()) for k, v in run_with(m, xd, md, gd, x_grad, mask_grad).items()}
        got = run_with(m, cl(xd), md, cl(gd), x_grad, mask_grad)
        assert (got["gx"] is not None) == x_grad and (got["gmask"] is not None) == mask_grad and all(got[k] is not None for k in KEYS)
        assert _is_cl(got["y"]) and (not x_grad or _is_cl(got["gx"]))
        assert_same_bits(c, base, got)


@pytest.mark.parametrize("shape,dtype", [((2, 48, 30, 22), "fp32"), ((2, 80, 60, 10), "fp16")])
def test_forward_without_gradients_keeps_no_gamma_and_gives_the_same_bits(dev, shape, dtype):
    from mga_yolo_amd import _lib
    c, dtype = P.case(*shape), DTYPES[dtype]
    m, x, mask, gy = inputs(c, dtype)
    m = m.to(dev)
    xd, md = x.to(dev), mask.to(dev)
    y_nchw, _ = forward_peak(m, xd, md, False)
    xc = cl(xd)
    y_grad, peak_grad = forward_peak(m, xc, md, True)
    y_off, peak_off = forward_peak(m, xc, md, False)
    assert _is_cl(y_off) and _is_cl(y_grad)
    assert torch.equal(y_grad, y_off) and torch.equal(y_off, y_nchw)
    plane = xd.numel() * xd.element_size()
    base = _lib.spade_ctx_bytes(c.B, c.C, c.H, c.W, c.hidden) - P.a16(xd.numel() * 4)
    print(f"{P.case_id(c)} {dtype}: peak with gradients {peak_grad} B, without {peak_off} B (y / gamma plane set {plane} B, rest of ctx {base} B)")
    assert peak_grad >= base + 2 * plane and peak_off < base + plane + plane // 2


# one call over five levels: channels_last masked (batch norm), NCHW masked, channels_last without a mask, channels_last whose mask needs
# no gradient, NCHW batch norm
MIXED = [((2, 48, 30, 22), "full", True), ((2, 64, 20, 44), "full", False), ((2, 16, 1, 37), "nomask", True), ((2, 64, 32, 4), "nogmask", True),
         ((2, 32, 7, 60), "full", False)]


def mixed_step(levels, together):
    from mga_yolo_amd import mask_spade, mask_spade_pyramid
    xs = [x.clone().requires_grad_(True) for _, x, _, _, _ in levels]
    ms = [None if kind == "nomask" else k.clone().requires_grad_(kind == "full") for _, _, k, _, kind in levels]
    for m, *_ in levels:
        m.zero_grad()
        if m.spade_config().bn:
            m.norm.reset_running_stats()
    run_of = lambda m: (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if m.spade_config().bn else None
    args = [(x, k, m.spade_params(), m.spade_config(), run_of(m)) for (m, *_), x, k in zip(levels, xs, ms)]
    ys = mask_spade_pyramid(args) if together else [mask_spade(*a) for a in args]
    torch.autograd.backward(list(ys), [gy for _, _, _, gy, _ in levels])
    torch.cuda.synchronize()
    out = []
    for (m, *_, kind), x, k, y in zip(levels, xs, ms, ys):
        assert (k is not None and k.grad is not None) == (kind == "full")
        assert all((p.grad is None) == (kind == "nomask") for p in m.parameters())
        assert _is_cl(y) == _is_cl(x) and _is_cl(x.grad) == _is_cl(x) and y.is_contiguous() == x.is_contiguous()
        out += [y.detach().clone(), x.grad.clone()] + ([k.grad.clone()] if kind == "full" else [])
        out += [p.grad.clone() for p in m.parameters() if p.grad is not None] + [v.clone() for v in m.buffers()]
    return out


def test_one_call_over_levels_of_both_layouts_equals_single_calls_bit_for_bit(dev):
    levels = []
    for shape, kind, nhwc in MIXED:
        m, x, mask, gy = inputs(P.case(*shape))
        conv = cl if nhwc else (lambda t: t)
        levels.append((m.to(dev), conv(x.to(dev)), mask.to(dev), conv(gy.to(dev)), kind))
    assert [_is_cl(lv[1]) for lv in levels] == [nhwc for _, _, nhwc in MIXED]
    a, b = mixed_step(levels, True), mixed_step(levels, False)
    assert len(a) == len(b)
    differ = [i for i, (p, q) in enumerate(zip(a, b)) if not torch.equal(p, q)]
    assert not differ, differ
    # and every level equals its run in the other layout
    flipped = [(m, (x.contiguous() if _is_cl(x) else cl(x)), k, (gy.contiguous() if _is_cl(gy) else cl(gy)), kind) for m, x, k, gy, kind in levels]
    f = mixed_step(flipped, True)
    differ = [i for i, (p, q) in enumerate(zip(a, f)) if not torch.equal(p, q)]
    assert not differ, differ


def step_on(m, x, mask, gy):
    """run() of tests/test_gpu_spade.py on x itself (no clone: x keeps its storage, offset and strides)."""
    m.zero_grad()
    x.grad = None
    x.requires_grad_(True)
    mk = mask.clone().requires_grad_(True)
    y = m([x, mk])
    y.backward(gy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "gx": x.grad, "gmask": mk.grad, **{k: p.grad for k, p in m.named_parameters()}}


def test_gy_of_the_other_layout_and_misaligned_storage(dev):
    c = P.case(2, 80, 60, 10)
    m, x, mask, gy = inputs(c)
    m = m.to(dev)
    xd, md, gd = x.to(dev), mask.to(dev), gy.to(dev)
    base = run(m, xd, md, gd)
    m.zero_grad()                                               # (to None: the gradients of `base` stay as they are)
    got = run(m, cl(xd), md, gd)                                # channels_last x, NCHW-contiguous gy
    assert _is_cl(got["y"]) and _is_cl(got["gx"])
    assert_same_bits(c, base, got)
    m.zero_grad()
    got = run(m, xd, md, cl(gd))                                # and the reverse
    assert got["y"].is_contiguous() and got["gx"].is_contiguous()
    assert_same_bits(c, base, got)
    # channels_last strides over storage that starts 4 bytes off a 16-byte boundary
    buf = torch.empty(xd.numel() + 1, device=dev)
    xv = buf[1:].view(c.B, c.H, c.W, c.C).permute(0, 3, 1, 2)
    xv.copy_(xd)
    assert _is_cl(xv) and xv.data_ptr() % 16 == 4
    got = step_on(m, xv, md, cl(gd))
    assert _is_cl(got["y"]) and _is_cl(got["gx"])
    assert_same_bits(c, base, got)


def test_channels_last_step_launches_only_library_kernels(dev):
    m, x, mask, gy = live_case(4, 64, 40, 40, "in", seed=3, hidden=32)
    m = m.to(dev)
    xd, md, gd = cl(x.to(dev)).requires_grad_(True), mask.to(dev).requires_grad_(True), cl(gy.to(dev))
    m([xd, md]).backward(gd)                                    # warm: sizes, the kernels' LDS limits
    m.zero_grad()
    xd.grad = md.grad = None
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        y = m([xd, md])
        y.backward(gd)
        torch.cuda.synchronize()
    assert _is_cl(y) and _is_cl(xd.grad)
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    kernels = [n for n in names if n.startswith(("k_", "void mgacbam", "mgacbam")) or "mgacbam::" in n]
    others = [n for n in names if n not in kernels and not n.lower().startswith(("memset", "memcpy"))]
    assert kernels, names
    assert any("k_spade" in n and "nhwc" in n for n in kernels), kernels
    assert not [n for n in names if "copy" in n.lower() or "contiguous" in n.lower()], names
    assert not others, others


def test_graph_capture_and_replay_of_a_channels_last_step(dev):
    c = P.case(2, 64, 20, 44)
    m, x, mask, gy = inputs(c)
    m = m.to(dev)
    xs, ks, gs = cl(x.to(dev)).requires_grad_(True), mask.to(dev).requires_grad_(True), cl(gy.to(dev))

    def step():
        y = m([xs, ks])
        return [y] + list(torch.autograd.grad(y, [xs, ks] + list(m.parameters()), gs))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    with torch.no_grad():
        xs.mul_(0.5).add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = step()
    torch.cuda.synchronize()
    assert _is_cl(eager[0]) and _is_cl(eager[1]) and _is_cl(replayed[0]) and _is_cl(replayed[1])
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager))


def test_fp16_autocast_gradscaler_step_through_the_module(dev):
    """The module on a channels_last fp16 feature inside a scaled step.  Everything around the block is element-wise or runs on an
    NCHW copy of its output (the same reduction order in both runs), so the two runs must agree to the bit."""
    import copy
    from mga_yolo_amd import MaskSPADE
    torch.manual_seed(4)
    spade = MaskSPADE(64, hidden=32).to(dev)
    g = torch.Generator().manual_seed(6)
    x0, mask0 = torch.randn(2, 64, 24, 24, generator=g).to(dev), torch.randn(2, 1, 24, 24, generator=g).to(dev)

    def step(mod, x):
        x = x.clone().requires_grad_(True)
        mask = mask0.clone().requires_grad_(True)
        opt = torch.optim.SGD(mod.parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda", dtype=torch.float16):
            z = mod([x.half(), mask])
            assert z.dtype == torch.float16
            loss = z.contiguous().float().pow(2).mean()
        scaler.scale(loss).backward()
        grads = {k: p.grad.clone() for k, p in mod.named_parameters()}
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        return z.detach(), loss.detach(), x.grad, mask.grad, grads, {k: p.detach().clone() for k, p in mod.named_parameters()}

    za, la, gxa, gma, ga, pa = step(copy.deepcopy(spade), x0)
    zb, lb, gxb, gmb, gb, pb = step(copy.deepcopy(spade), cl(x0))
    assert za.is_contiguous() and _is_cl(zb) and _is_cl(gxb)
    assert all(torch.isfinite(v).all() for v in gb.values())
    assert torch.equal(la, lb) and torch.equal(za, zb) and torch.equal(gxa, gxb) and torch.equal(gma, gmb)
    assert all(torch.equal(ga[k], gb[k]) for k in ga) and all(torch.equal(pa[k], pb[k]) for k in pa)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_two_runs_give_the_same_bits(dev, dtype):
    c = P.case(2, 80, 60, 10)
    m, x, mask, gy = inputs(c, DTYPES[dtype])
    m = m.to(dev)
    xd, md, gd = cl(x.to(dev)), mask.to(dev), cl(gy.to(dev))
    r1 = {k: v.clone() for k, v in run(m, xd, md, gd).items()}
    m.zero_grad()
    r2 = run(m, xd, md, gd)
    assert_same_bits(c, r1, r2)
