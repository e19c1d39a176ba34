"""MaskSPADE on the device at the paths tests/test_gpu_spade.py does not reach: the 8- and 4-wide pixel tilings, hidden 48, C up to the
limit of 1024 (split-K chunks over two samples), the forward that keeps no gamma, a backward without dL/dmask, thin and tiny grids, eps /
momentum other than the defaults, and launch groups of mixed levels.  The rows and what each is for are the table of tests/spade_plan.py;
tests/test_spade_plan.py proves on the CPU that every row takes the paths it declares and meets the seed rule (no fp64 pre-activation
with |pre| < 1e-5: no ReLU branch can differ, nothing is widened).

Bars, the project's standing ones.  fp32: rel_err <= 1e-4 on every tensor and elem_err < 1e-3 on y, gx, gmask against the fp64 oracle.
fp16 / bf16: rel_err against the oracle on the rounded inputs at most twice that of the torch composition under autocast.  Where two
calls run the same launches on the same inputs the results are compared bit for bit."""
import os
import sys

import pytest
import torch

from conftest import elem_err, rel_err

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spade_plan as P  # noqa: E402
from test_gpu_spade import ELEM, KEYS, TOL, dev, live_case, oracle_of, run  # noqa: E402,F401  (dev: the module's device fixture)

pytestmark = pytest.mark.gpu
HALF = [(2, 48, 30, 22), (2, 80, 60, 10), (3, 1024, 32, 20)]
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
_oracles = {}


def inputs(c, dtype=torch.float32):
    """(module on the host with the row's eps / momentum, x, mask, gy): x and gy rounded to dtype, the mask stays fp32."""
    m, x, mask, gy = live_case(c.B, c.C, c.H, c.W, c.norm, seed=c.seed, hidden=c.hidden)
    m.norm.eps = c.eps
    if c.norm == "bn":
        m.norm.momentum = c.momentum
    return m, x.to(dtype), mask, gy.to(dtype)


def oracle(c, dtype=torch.float32):
    """The fp64 oracle of a row on the inputs rounded to dtype: computed once, shared by every test that needs it, never written to."""
    key = (P.case_id(c), dtype)
    if key not in _oracles:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        m, x, mask, gy = inputs(c, dtype)
        _oracles[key] = oracle_of(m, x.float(), mask, gy.float(), c.norm, c.eps, c.momentum)
    return _oracles[key]


def where(c, got, want, by_elem=False):
    """The worst element of a feature- or mask-shaped tensor (by_elem: in elem_err's measure, else in rel_err's): its (b, c, y, x), its
    tile and its place in the tile."""
    d = (got.detach().double().cpu() - want.double()).abs()
    if by_elem:
        d = d / want.double().abs().clamp_min(1e-3 * float(want.abs().max()))
    if d.dim() != 4 or tuple(d.shape[-2:]) != (c.H, c.W):
        return f"worst at {tuple(int(i) for i in torch.unravel_index(d.argmax(), d.shape))}"
    b, ch, y, x = (int(i) for i in torch.unravel_index(d.argmax(), d.shape))
    (ty, tx), (r, col) = P.locate(c.H, c.W, y, x)
    t = P.tiling(c.H, c.W)
    return (f"worst at (b,c,y,x) = ({b},{ch},{y},{x}): tile (ty,tx) = ({ty},{tx}) of {t.tiles_y}x{t.tiles_x} tiles of {t.TH} rows x {t.TW} "
            f"columns, row {r} column {col} of the tile; got {float(got[b, ch, y, x]):.6e} want {float(want[b, ch, y, x]):.6e}")


def check_fp32(c, got, want, keys, tag=""):
    report = []
    for k in keys:
        r = rel_err(got[k], want[k])
        e = elem_err(got[k], want[k]) if k in ("y", "gx", "gmask") else 0.0
        print(f"{P.case_id(c)}{tag} {k} rel_err {r:.3e}" + (f" elem_err {e:.3e}" if k in ("y", "gx", "gmask") else ""))
        if not r <= TOL or not e < ELEM:
            report.append(f"{k} rel {r:.3e} elem {e:.3e}: {where(c, got[k], want[k], by_elem=r <= TOL)}")
    return report


@pytest.mark.parametrize("c", P.CASES, ids=[P.case_id(c) for c in P.CASES])
def test_every_row_element_wise_against_the_oracle(dev, c):
    m, x, mask, gy = inputs(c)
    want, ctx = oracle(c)
    m = m.to(dev)
    got = run(m, x.to(dev), mask.to(dev), gy.to(dev))
    report = check_fp32(c, got, want, ["y", "gx", "gmask"] + KEYS)
    if c.norm == "bn":
        for k, w in zip(("running_mean", "running_var"), ctx["new_running"]):
            r = rel_err(getattr(m.norm, k), w)
            print(f"{P.case_id(c)} {k} rel_err {r:.3e}")
            if not r <= TOL:
                report.append(f"{k} {r:.3e}")
        assert int(m.norm.num_batches_tracked) == 1
    assert not report, "\n".join([c.what] + report)


def compose(m, x, mask, gy, dtype, grad=True):
    """The block's torch composition under autocast on the module's current state (the yardstick of the half-precision bar)."""
    from mga_yolo_amd.functional import spade_compose
    cfg = m.spade_config()
    running = (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if cfg.bn else None
    xr, mr = x.clone().requires_grad_(grad), mask.clone().requires_grad_(grad)
    with torch.autocast("cuda", dtype=dtype):
        yr = spade_compose(xr, mr, m.spade_params(), cfg, running)
    if not grad:
        return {"y": yr.detach()}
    yr.backward(gy)
    return {"y": yr.detach(), "gx": xr.grad, "gmask": mr.grad, **{k: p.grad for k, p in m.named_parameters()}}


def check_half(c, dtype, got, ref, want, keys, tag=""):
    report = []
    for k in keys:
        a, b = rel_err(got[k].float(), want[k]), rel_err(ref[k].float(), want[k])
        print(f"{P.case_id(c)}{tag} {dtype} {k}: device {a:.3e}  torch composition {b:.3e}")
        if not a <= 2 * b:
            report.append(f"{k} device {a:.3e} > 2 x {b:.3e}: {where(c, got[k].float(), want[k])}")
    return report


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", HALF, ids=[P.case_id(P.case(*s)) for s in HALF])
def test_half_precision_rows_against_the_oracle_on_rounded_inputs(dev, shape, dtype):
    c, dtype = P.case(*shape), DTYPES[dtype]
    m, x, mask, gy = inputs(c, dtype)
    want, _ = oracle(c, dtype)
    m = m.to(dev)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    xd, md, gd = x.to(dev), mask.to(dev), gy.to(dev)
    got = run(m, xd, md, gd)
    m.load_state_dict(state)
    m.zero_grad()
    ref = compose(m, xd, md, gd, dtype)
    report = check_half(c, dtype, got, ref, want, ["y", "gx", "gmask"] + KEYS)
    assert not report, "\n".join([c.what] + report)


def forward_peak(m, xd, md, grad):
    """One forward -> (y, bytes the call allocated at its peak above what was allocated before it)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.set_grad_enabled(grad):
        y = m([xd, md])
    torch.cuda.synchronize()
    return y.detach(), torch.cuda.max_memory_allocated() - before


@pytest.mark.parametrize("shape,dtype", [((2, 48, 30, 22), "fp32"), ((2, 80, 60, 10), "fp32"), ((2, 80, 60, 10), "fp16")])
def test_forward_without_gradients_keeps_no_gamma_and_gives_the_same_bits(dev, shape, dtype):
    """torch.no_grad() runs k_spade_fwd<T, false>: the same products (explicit fmaf) and accumulation order, minus the store of gamma.
    That it IS the other instantiation shows in what the call allocates: ctx without the gamma planes."""
    from mga_yolo_amd import _lib
    c, dtype = P.case(*shape), DTYPES[dtype]
    m, x, mask, gy = inputs(c, dtype)
    want, _ = oracle(c, dtype)
    m = m.to(dev)
    assert all(p.requires_grad for p in m.parameters())        # the module as a user holds it: only the grad mode says "inference"
    xd, md = x.to(dev), mask.to(dev)
    y_grad, peak_grad = forward_peak(m, xd, md, True)
    y_off, peak_off = forward_peak(m, xd, md, False)
    assert torch.equal(y_grad, y_off)
    plane = xd.numel() * xd.element_size()                     # y, and gamma where it is kept
    base = _lib.spade_ctx_bytes(c.B, c.C, c.H, c.W, c.hidden) - P.a16(xd.numel() * 4)
    print(f"{P.case_id(c)} {dtype}: peak with gradients {peak_grad} B, without {peak_off} B (y / gamma plane set {plane} B, rest of ctx {base} B)")
    assert peak_grad >= base + 2 * plane and peak_off < base + plane + plane // 2
    if dtype == torch.float32:
        report = check_fp32(c, {"y": y_off}, want, ["y"], " no_grad")
    else:
        report = check_half(c, dtype, {"y": y_off}, compose(m, xd, md, None, dtype, grad=False), want, ["y"], " no_grad")
    assert not report, "\n".join([c.what] + report)
    if c.norm != "bn":
        return
    assert int(m.norm.num_batches_tracked) == 2                # a training-mode forward updates the statistics whatever the grad mode
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    y_eval, peak_eval = forward_peak(m, xd, md, False)
    y_eval_grad, _ = forward_peak(m, xd, md, True)
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    assert torch.equal(y_eval, y_eval_grad) and peak_eval < base + plane + plane // 2
    import spade_oracle as SO
    params = {k: v.detach().cpu() for k, v in m.state_dict().items() if k in KEYS}
    y64, _ = SO.forward(x, mask, params, "bn", False, True, c.eps, (m.norm.running_mean.cpu(), m.norm.running_var.cpu()))
    report = check_fp32(c, {"y": y_eval}, {"y": y64}, ["y"], " eval no_grad")
    assert not report, report


def run_with(m, x, mask, gy, x_grad, mask_grad):
    """run() of tests/test_gpu_spade.py with the two input gradients asked for or not."""
    m.zero_grad()
    x, mask = x.clone().requires_grad_(x_grad), mask.clone().requires_grad_(mask_grad)
    y = m([x, mask])
    y.backward(gy)
    torch.cuda.synchronize()
    return {"y": y.detach(), "gx": x.grad, "gmask": mask.grad, **{k: p.grad for k, p in m.named_parameters()}}


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_backward_without_mask_gradient_or_without_feature_gradient(dev, dtype):
    """The same launches minus k_spade_gmask: everything else comes out bit for bit; dL/dx not being asked for changes no launch."""
    c, dtype = P.case(2, 80, 60, 10), DTYPES[dtype]
    m, x, mask, gy = inputs(c, dtype)
    m = m.to(dev)
    xd, md, gd = x.to(dev), mask.to(dev), gy.to(dev)
    full = run_with(m, xd, md, gd, True, True)
    assert full["gx"] is not None and full["gmask"] is not None and all(full[k] is not None for k in KEYS)
    nomask = run_with(m, xd, md, gd, True, False)
    assert nomask["gmask"] is None
    assert all(torch.equal(nomask[k], full[k]) for k in ["y", "gx"] + KEYS)
    nox = run_with(m, xd, md, gd, False, True)
    assert nox["gx"] is None
    assert all(torch.equal(nox[k], full[k]) for k in ["y", "gmask"] + KEYS)
    params_only = run_with(m, xd, md, gd, False, False)
    assert params_only["gx"] is None and params_only["gmask"] is None
    assert all(torch.equal(params_only[k], full[k]) for k in ["y"] + KEYS)


# One call over seven levels (the limit is 8).  Five masked levels with a mask gradient share a signature and split 4 + 1 over two
# launch groups, four tilings and hidden 16 / 64 / 48 / 32 / 32 sharing the groups' dynamic LDS size; one level has no mask; one has a
# mask that needs no gradient (the forward groups it with the masked ones, 4 + 2; the backward launches it alone).
PYRAMID = [((2, 32, 16, 8), "full"), ((2, 16, 1, 37), "nomask"), ((2, 80, 60, 10), "full"), ((2, 48, 30, 22), "full"),
           ((2, 64, 32, 4), "nogmask"), ((2, 32, 7, 60), "full"), ((3, 32, 5, 3), "full")]


def mixed_step(levels, together):
    """pyramid_step of tests/test_gpu_spade.py for levels (module, x, mask, gy, kind)."""
    from mga_yolo_amd import mask_spade, mask_spade_pyramid
    xs = [x.clone().requires_grad_(True) for _, x, _, _, _ in levels]
    ms = [None if kind == "nomask" else k.clone().requires_grad_(kind == "full") for _, _, k, _, kind in levels]
    for m, *_ in levels:
        m.zero_grad()
        if m.spade_config().bn:
            m.norm.reset_running_stats()
    run_of = lambda m: (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if m.spade_config().bn else None
    if together:
        ys = mask_spade_pyramid([(x, k, m.spade_params(), m.spade_config(), run_of(m)) for (m, *_), x, k in zip(levels, xs, ms)])
    else:
        ys = [mask_spade(x, k, m.spade_params(), m.spade_config(), run_of(m)) for (m, *_), x, k in zip(levels, xs, ms)]
    torch.autograd.backward(list(ys), [gy for _, _, _, gy, _ in levels])
    torch.cuda.synchronize()
    out = []
    for (m, *_, kind), x, k, y in zip(levels, xs, ms, ys):
        assert (k is not None and k.grad is not None) == (kind == "full")
        assert all((p.grad is None) == (kind == "nomask") for p in m.parameters())
        out += [y.detach().clone(), x.grad.clone()] + ([k.grad.clone()] if kind == "full" else [])
        out += [p.grad.clone() for p in m.parameters() if p.grad is not None] + [v.clone() for v in m.buffers()]
    return out


def test_one_call_over_seven_mixed_levels_equals_single_calls_bit_for_bit(dev):
    assert len(PYRAMID) == 7 < P.MAX_LEVELS + 1 and sum(kind == "full" for _, kind in PYRAMID) == P.GROUP_MAX + 1
    levels = []
    for shape, kind in PYRAMID:
        m, x, mask, gy = inputs(P.case(*shape))
        levels.append((m.to(dev), x.to(dev), mask.to(dev), gy.to(dev), kind))
    assert {P.case(*s).tw for s, kind in PYRAMID if kind == "full"} == {4, 8, 16, 32}
    a, b = mixed_step(levels, True), mixed_step(levels, False)
    assert len(a) == len(b)
    differ = [i for i, (p, q) in enumerate(zip(a, b)) if not torch.equal(p, q)]
    assert not differ, differ
