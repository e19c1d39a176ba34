"""MaskSPADE on the device (HIP kernels of csrc/spade.cuh) against the stored fixtures and the fp64 oracle (tests/spade_oracle.py).

Bars.  fp32: rel_err <= 1e-4 against the goldens / the oracle (the reference's own fp32 run sits within 1e-6 of its fp64 run, so the
project's standing bar leaves two orders of room) and elem_err < 1e-3 on y, gx, gmask (the standing element-wise bar).  fp16 / bf16: the
device against the fp64 oracle on the rounded inputs, rel_err at most twice that of the torch composition under autocast against the same
oracle.  ReLU edge of the live rows: pre-activations with |pre| < 1e-5 may take the other branch on the device; their share must be at
most 1e-4 of h and each gradient's bound is widened by the sum of those elements' own contributions, from the oracle."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, elem_err, rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spade_oracle as SO  # noqa: E402

pytestmark = pytest.mark.gpu
TOL, ELEM = 1e-4, 1e-3
KEYS = list(SO.PARAM_KEYS)
NAMES = sorted(f[len("spade_"):-len(".npz")] for f in os.listdir(GOLDEN) if f.startswith("spade_") and f.endswith(".npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mga_yolo_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def load(name):
    z = np.load(os.path.join(GOLDEN, f"spade_{name}.npz"), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}, json.loads(bytes(z["meta"]).decode())


def module_from(meta, d, dev):
    from mga_yolo_amd import MaskSPADE
    m = MaskSPADE(meta["shape"][1], hidden=meta["hidden"], mask_channels=meta["mask_channels"], norm_type=meta["norm_type"],
                  use_sigmoid_mask=meta["use_sigmoid_mask"], eps=meta["eps"])
    sd = {k[len("param."):]: v for k, v in d.items() if k.startswith("param.")}
    sd.update({k[len("run0."):]: v for k, v in d.items() if k.startswith("run0.")})
    m.load_state_dict(sd, strict=True)
    return m.to(dev).train(meta["training"])


def run(m, x, mask, gy):
    x = x.clone().requires_grad_(True)
    mask = None if mask is None else mask.clone().requires_grad_(True)
    y = m(x if mask is None else [x, mask])
    y.backward(gy)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "gx": x.grad}
    if mask is not None:
        out["gmask"] = mask.grad
        out.update({k: p.grad for k, p in m.named_parameters()})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_every_golden_element_wise(dev, name):
    import warnings
    d, meta = load(name)
    m = module_from(meta, d, dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                    # maskc2 takes the documented torch composition (warned once)
        got = run(m, d["x"].to(dev), d["mask"].to(dev) if "mask" in d else None, d["gy"].to(dev))
    want = {"y": d["out.y"], "gx": d["out.gx"]}
    if "mask" in d:
        want["gmask"] = d["out.gmask"]
        want.update({k: d["out.g." + k] for k in KEYS})
    report = []
    for k, w in want.items():
        r, e = rel_err(got[k], w), elem_err(got[k], w)
        print(f"{name} {k} rel_err {r:.3e} elem_err {e:.3e}")
        if not r <= TOL or (k in ("y", "gx", "gmask") and not e < ELEM):
            report.append(f"{k} rel {r:.3e} elem {e:.3e}")
    for k, v in m.state_dict().items():
        if k.startswith("norm."):
            r = rel_err(v.double(), d["out." + k].double())
            print(f"{name} {k} rel_err {r:.3e}")
            if not r <= TOL:
                report.append(f"{k} {r:.3e}")
    assert not report, report


LIVE = [(32, 64, 80, 80, "in"), (32, 128, 40, 40, "bn"), (32, 256, 20, 20, "in"), (8, 256, 160, 160, "in")]


def live_case(B, C, H, W, norm, seed=77, hidden=64):
    from mga_yolo_amd import MaskSPADE
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    mask = torch.randn(B, 1, H, W, generator=g)
    gy = torch.randn(B, C, H, W, generator=g)
    torch.manual_seed(seed)
    m = MaskSPADE(C, hidden=hidden, norm_type=norm)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k in KEYS:
                v.add_(0.05 * torch.randn(v.shape, generator=g))
    return m, x, mask, gy


def oracle_of(m, x, mask, gy, norm, eps=1e-6, momentum=0.1):
    params = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in KEYS}
    runs = (m.norm.running_mean.detach().cpu().clone(), m.norm.running_var.detach().cpu().clone()) if norm == "bn" else None
    y, ctx = SO.forward(x, mask, params, norm, True, True, eps, runs, momentum)
    g = SO.backward(gy, ctx)
    g["y"] = y
    return g, ctx


@pytest.mark.parametrize("B,C,H,W,norm", LIVE)
def test_live_oracle_at_training_sizes(dev, B, C, H, W, norm):
    torch.set_num_threads(16)
    m, x, mask, gy = live_case(B, C, H, W, norm)
    want, ctx = oracle_of(m, x, mask, gy, norm)
    share, widen = SO.relu_edge(gy, ctx)
    print(f"|pre| < 1e-5: share {share:.3e} of h")
    assert share <= 1e-4
    m = m.to(dev)
    got = run(m, x.to(dev), mask.to(dev), gy.to(dev))
    report = []
    for k in ["y", "gx", "gmask"] + KEYS:
        scale = float(want[k].abs().max())
        r = rel_err(got[k], want[k])
        bound = TOL + widen.get(k, 0.0) / scale
        print(f"({B},{C},{H},{W}) {norm} {k} rel_err {r:.3e} bound {bound:.3e}")
        if not r <= bound:
            report.append(f"{k} {r:.3e} > {bound:.3e}")
    if norm == "bn":
        for k, w in zip(("running_mean", "running_var"), ctx["new_running"]):
            r = rel_err(getattr(m.norm, k), w)
            print(f"{k} rel_err {r:.3e}")
            if not r <= TOL:
                report.append(f"{k} {r:.3e}")
        assert int(m.norm.num_batches_tracked) == 1
    assert not report, report


# Channel counts at which the kernels take their tail paths, masked, forward and backward: C % 32 == 16 (the last channel round of the
# transposed convolution holds 16 channels) and 64 < C < 256 on a grid small enough for the forward's channel block to be halved to a
# size that does not divide C (80 -> 48 + 32, 144 -> 48 + 48 + 48, 112 -> 64 + 48, 240 -> 64 x 3 + 48).  B = 2, so that a channel
# block running past C would land in the next sample.  Seeds chosen on the CPU by the generator's rule: no fp64 pre-activation with
# |pre| < 1e-5, so the plain bar holds for every tensor and nothing is widened.
TAILS = [(2, 48, 17, 23, "in", 64, 64), (2, 80, 20, 20, "in", 64, 73), (2, 144, 10, 10, "bn", 32, 65), (2, 112, 9, 11, "in", 16, 63),
         (2, 240, 8, 8, "bn", 64, 65)]


@pytest.mark.parametrize("B,C,H,W,norm,hidden,seed", TAILS)
def test_channel_tails_masked_forward_and_backward(dev, B, C, H, W, norm, hidden, seed):
    m, x, mask, gy = live_case(B, C, H, W, norm, seed=seed, hidden=hidden)
    want, ctx = oracle_of(m, x, mask, gy, norm)
    assert SO.min_abs_pre(ctx) >= 1e-5
    m = m.to(dev)
    got = run(m, x.to(dev), mask.to(dev), gy.to(dev))
    errs = {k: rel_err(got[k], want[k]) for k in ["y", "gx", "gmask"] + KEYS}
    print(f"({B},{C},{H},{W}) {norm} hidden {hidden}", {k: f"{v:.3e}" for k, v in errs.items()})
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("B,C,H,W,norm", [(4, 64, 40, 40, "in"), (2, 128, 17, 23, "bn")])
def test_half_precision_against_the_oracle_on_rounded_inputs(dev, dtype, B, C, H, W, norm):
    from mga_yolo_amd.functional import spade_compose
    m, x, mask, gy = live_case(B, C, H, W, norm, seed=91)
    x, gy = x.to(dtype), gy.to(dtype)
    want, _ = oracle_of(m, x.float(), mask, gy.float(), norm)
    m = m.to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    got = run(m, x.to(dev), mask.to(dev), gy.to(dev))
    m.load_state_dict(state)
    m.zero_grad()
    xr, mr = x.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True)
    cfg = m.spade_config()
    running = (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if cfg.bn else None
    with torch.autocast("cuda", dtype=dtype):
        yr = spade_compose(xr, mr, m.spade_params(), cfg, running)
    yr.backward(gy.to(dev))
    ref = {"y": yr.detach(), "gx": xr.grad, "gmask": mr.grad, **{k: p.grad for k, p in m.named_parameters()}}
    report = []
    for k in ["y", "gx", "gmask"] + KEYS:
        a, b = rel_err(got[k].float(), want[k]), rel_err(ref[k].float(), want[k])
        print(f"{dtype} ({B},{C},{H},{W}) {norm} {k}: device {a:.3e}  torch composition {b:.3e}")
        if not a <= 2 * b:
            report.append(f"{k} device {a:.3e} > 2 x {b:.3e}")
    assert not report, report


def pyramid_inputs(dev, dtype=torch.float32):
    out = []
    for i, (C, H, W, norm) in enumerate([(64, 40, 40, "in"), (128, 20, 20, "bn"), (256, 10, 10, "in")]):
        m, x, mask, gy = live_case(2, C, H, W, norm, seed=50 + i, hidden=32)
        out.append((m.to(dev), x.to(dev, dtype), mask.to(dev), gy.to(dev, dtype)))
    return out


def pyramid_step(levels, together):
    from mga_yolo_amd import mask_spade, mask_spade_pyramid
    xs = [x.clone().requires_grad_(True) for _, x, _, _ in levels]
    ms = [k.clone().requires_grad_(True) for _, _, k, _ in levels]
    for m, *_ in levels:
        m.zero_grad()
        if m.spade_config().bn:
            m.norm.reset_running_stats()
    run_of = lambda m: (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if m.spade_config().bn else None
    if together:
        ys = mask_spade_pyramid([(x, k, m.spade_params(), m.spade_config(), run_of(m)) for (m, *_), x, k in zip(levels, xs, ms)])
    else:
        ys = [mask_spade(x, k, m.spade_params(), m.spade_config(), run_of(m)) for (m, *_), x, k in zip(levels, xs, ms)]
    torch.autograd.backward(list(ys), [gy for *_, gy in levels])
    torch.cuda.synchronize()
    out = []
    for (m, *_), x, k, y in zip(levels, xs, ms, ys):
        out += [y.detach().clone(), x.grad.clone(), k.grad.clone()] + [p.grad.clone() for p in m.parameters()] + [v.clone() for v in m.buffers()]
    return out


def test_pyramid_call_equals_single_calls_bit_for_bit(dev):
    levels = pyramid_inputs(dev)
    a, b = pyramid_step(levels, True), pyramid_step(levels, False)
    assert len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_two_runs_give_the_same_bits(dev, dtype):
    levels = pyramid_inputs(dev, dtype)
    a, b = pyramid_step(levels, True), pyramid_step(levels, True)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    m, x, mask, gy = live_case(8, 64, 80, 80, "in", seed=5)           # several tiles per split-K chunk
    m = m.to(dev)
    r1 = run(m, x.to(dev, dtype), mask.to(dev), gy.to(dev, dtype))
    m.zero_grad()
    r2 = run(m, x.to(dev, dtype), mask.to(dev), gy.to(dev, dtype))
    assert all(torch.equal(r1[k], r2[k]) for k in r1)


def test_bn_running_statistics_train_then_eval(dev):
    m, x, mask, gy = live_case(4, 32, 12, 20, "bn", seed=8, hidden=16)
    m = m.to(dev)
    xd = x.to(dev)
    for step in range(1, 4):
        m([xd * step, mask.to(dev)])
    rm, rv = torch.zeros(32, dtype=torch.float64), torch.ones(32, dtype=torch.float64)
    for step in range(1, 4):
        xs = (x * step).double()
        rm = 0.9 * rm + 0.1 * xs.mean(dim=(0, 2, 3))
        rv = 0.9 * rv + 0.1 * xs.var(dim=(0, 2, 3), unbiased=True)
    assert rel_err(m.norm.running_mean, rm) <= TOL and rel_err(m.norm.running_var, rv) <= TOL
    assert int(m.norm.num_batches_tracked) == 3
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    got = run(m, xd, mask.to(dev), gy.to(dev))
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    params = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in KEYS}
    y, ctx = SO.forward(x, mask, params, "bn", False, True, 1e-6, (m.norm.running_mean.cpu(), m.norm.running_var.cpu()))
    want = SO.backward(gy, ctx)
    want["y"] = y
    errs = {k: rel_err(got[k], want[k]) for k in ["y", "gx", "gmask"] + KEYS}
    print(errs)
    assert all(e <= TOL for e in errs.values()), errs


@pytest.mark.parametrize("norm,train", [("in", True), ("bn", True), ("bn", False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_no_mask_path(dev, norm, train, dtype):
    m, x, _, gy = live_case(3, 48, 17, 23, norm, seed=12, hidden=16)
    m = m.to(dev).train(train)
    x, gy = x.to(dtype), gy.to(dtype)
    runs = (m.norm.running_mean.cpu().clone(), m.norm.running_var.cpu().clone()) if norm == "bn" else None
    y, ctx = SO.forward(x.float(), None, None, norm, train, True, 1e-6, runs)
    want = SO.backward(gy.float(), ctx)
    got = run(m, x.to(dev), None, gy.to(dev))
    tol = TOL if dtype == torch.float32 else 2 ** -9       # one rounding of the output to fp16 (2^-11 relative) at up to ~4 sigma of the scale
    errs = {"y": rel_err(got["y"].float(), y), "gx": rel_err(got["gx"].float(), want["gx"])}
    print(errs)
    assert all(e <= tol for e in errs.values()), errs
    assert all(p.grad is None for p in m.parameters())


def test_fallbacks_agree_with_the_kernels(dev):
    """Where both apply: a channels_last feature and a half-size mask enter the kernels after one torch step on the device, and the torch
    composition (what the shapes outside the kernels' limits run) gives the kernels' result within the bar."""
    import warnings
    from mga_yolo_amd import MaskSPADE
    from mga_yolo_amd.functional import spade_compose
    m, x, mask, gy = live_case(2, 64, 24, 24, "in", seed=21, hidden=32)
    m = m.to(dev)
    base = run(m, x.to(dev), mask.to(dev), gy.to(dev))
    m.zero_grad()
    cl = run(m, x.to(dev).contiguous(memory_format=torch.channels_last), mask.to(dev), gy.to(dev))
    assert all(torch.equal(base[k], cl[k]) for k in base)
    m.zero_grad()
    xr, mr = x.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True)
    yr = spade_compose(xr, mr, m.spade_params(), m.spade_config())
    yr.backward(gy.to(dev))
    comp = {"y": yr.detach(), "gx": xr.grad, "gmask": mr.grad, **{k: p.grad for k, p in m.named_parameters()}}
    errs = {k: rel_err(base[k], comp[k]) for k in base}
    print(errs)
    assert all(e <= TOL for e in errs.values()), errs
    # a mask at half the feature's size: resampled on the device, then the kernels
    small = torch.randn(2, 1, 12, 12, generator=torch.Generator().manual_seed(3))
    params = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in KEYS}
    y, ctx = SO.forward(x, small, params, "in", True, True, 1e-6)
    want = SO.backward(gy, ctx)
    m.zero_grad()
    got = run(m, x.to(dev), small.to(dev), gy.to(dev))
    errs = {"y": rel_err(got["y"], y), **{k: rel_err(got[k], want[k]) for k in ["gx", "gmask"] + KEYS}}
    print(errs)
    assert all(e <= TOL for e in errs.values()), errs
    # outside the limits: the composition runs on the device, warned about once per reason
    odd = MaskSPADE(24, hidden=8).to(dev)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        from mga_yolo_amd import functional as Fn
        Fn._spade_warned.clear()
        xo = torch.randn(2, 24, 9, 9, device=dev)
        y1 = odd([xo, torch.randn(2, 1, 9, 9, device=dev)])
        odd([xo, torch.randn(2, 1, 9, 9, device=dev)])
    assert y1.is_cuda and len([i for i in w if "torch composition" in str(i.message)]) == 1


def test_fp16_autocast_gradscaler_step_through_the_module(dev):
    from mga_yolo_amd import MaskSPADE
    torch.manual_seed(4)
    net = torch.nn.ModuleDict(dict(stem=torch.nn.Conv2d(3, 64, 3, padding=1), head=torch.nn.Conv2d(64, 1, 1), spade=MaskSPADE(64, hidden=32),
                                   out=torch.nn.Conv2d(64, 8, 1))).to(dev)
    ref = __import__("copy").deepcopy(net)
    img = torch.randn(2, 3, 32, 32, device=dev)

    def step(n, composed):
        from mga_yolo_amd.functional import spade_compose
        opt = torch.optim.SGD(n.parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda", dtype=torch.float16):
            f = n["stem"](img)
            mask = n["head"](f)
            s = n["spade"]
            z = spade_compose(f, mask, s.spade_params(), s.spade_config()) if composed else s([f, mask])
            assert z.dtype == torch.float16
            loss = n["out"](z).float().pow(2).mean()
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        return float(loss), {k: p.detach().float().clone() for k, p in n.named_parameters()}, {k: p.grad.clone() for k, p in n.named_parameters()}

    la, pa, ga = step(net, False)
    lb, pb, gb = step(ref, True)
    assert all(torch.isfinite(g).all() for g in ga.values())
    assert abs(la - lb) <= 2e-2 * abs(lb)
    errs = {k: rel_err(pa[k], pb[k]) for k in pa}
    print(la, lb, errs)
    assert all(e <= 2e-2 for e in errs.values()), errs          # two fp16 pipelines after one SGD step: the fp16 slice tests' tolerance


def test_graph_capture_and_replay_of_forward_and_backward(dev):
    m, x, mask, gy = live_case(2, 64, 20, 20, "bn", seed=31, hidden=32)
    m = m.to(dev)
    xs, ks, gs = x.to(dev).requires_grad_(True), mask.to(dev).requires_grad_(True), gy.to(dev)

    def step():
        y = m([xs, ks])
        grads = torch.autograd.grad(y, [xs, ks] + list(m.parameters()), gs)
        return [y] + list(grads)

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
    m.norm.reset_running_stats()
    with torch.no_grad():
        xs.mul_(0.5).add_(0.1)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    rm = m.norm.running_mean.clone()
    m.norm.reset_running_stats()
    eager = step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(replayed, eager))
    assert torch.equal(rm, m.norm.running_mean) and int(m.norm.num_batches_tracked) == 1
