"""Every library call of the eager path goes out through ONE helper (mga_yolo_amd/_binding.py: call), which looks torch's current stream up
on every call.  Each block runs forward and backward on the default stream (twice) and once inside torch.cuda.stream(side), on the same inputs.

Bar: an output the two default-stream runs give bit-identically must come out bit-identical on the side stream; one that differs between
them (floating-point atomics) may differ from the first run by no more than the second run does.

A helper that kept the first stream it saw would put the side run's kernels on the default stream.  So that this cannot pass by luck, the
side run's inputs are zero-filled buffers that the side stream fills (device-to-device) behind some unrelated work of its own: kernels on any
other stream read zeros.  Shapes: B=2, H=W=8, C=16 (hidden 16 for MaskSPADE, its minimum); contiguous and channels_last x where a block has
channels-last kernels."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, CH, H, W = 2, 16, 8, 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from mga_yolo_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _leaf(t):
    return t.detach().requires_grad_(True)


# Each case: inputs(cl) -> {name: host tensor} and run(device inputs) -> {name: output}.  cl: x in torch.channels_last.
def _feature_inputs(seed, cl, extra):
    g = _g(seed)
    d = dict(x=torch.randn(B, CH, H, W, generator=g), mask=torch.randn(B, 1, H, W, generator=g), gy=torch.randn(B, CH, H, W, generator=g))
    d.update({k: 0.3 * torch.randn(s, generator=g) for k, s in extra.items()})
    if cl:
        d["x"], d["gy"] = (d[k].contiguous(memory_format=torch.channels_last) for k in ("x", "gy"))
    return d


def _grads(out, leaves):
    out.update({"g" + k: t.grad for k, t in leaves.items()})
    return out


CBAM_P = dict(w1=(4, CH), b1=(4,), w2=(CH, 4), b2=(CH,), wsa=(1, 3, 7, 7), beta=())


def cbam_run(d):
    from mga_yolo_amd import BlockConfig, mask_cbam
    lv = {k: _leaf(d[k]) for k in ("x", "mask", *CBAM_P)}
    y = mask_cbam(lv["x"], lv["mask"], *(lv[k] for k in CBAM_P), BlockConfig(hidden=4))
    y.backward(d["gy"])
    return _grads(dict(y=y.detach()), lv)


ECA_P = dict(w=(1, 1, 3), beta=())


def eca_run(d):
    from mga_yolo_amd import EcaConfig, mask_eca
    lv = {k: _leaf(d[k]) for k in ("x", "mask", *ECA_P)}
    y = mask_eca(lv["x"], lv["mask"], lv["w"], lv["beta"], EcaConfig(k=3))
    y.backward(d["gy"])
    return _grads(dict(y=y.detach()), lv)


HEAD_P = dict(w1=(8, CH, 1, 1), gamma=(8,), beta=(8,), wh=(1, 8, 3, 3), bh=(1,), gl=(B, 1, H, W))


def head_run(d):
    from mga_yolo_amd import mask_head
    lv = {k: _leaf(d[k]) for k in ("x", "w1", "gamma", "beta", "wh", "bh")}
    rm, rv = torch.zeros(8, device=d["x"].device), torch.ones(8, device=d["x"].device)
    nbt = torch.zeros((), dtype=torch.int64, device=d["x"].device)
    logits = mask_head(lv["x"], lv["w1"], lv["gamma"], lv["beta"], rm, rv, nbt, lv["wh"], lv["bh"], eps=1e-3, momentum=0.03, training=True)
    logits.backward(d["gl"])
    return _grads(dict(logits=logits.detach(), running_mean=rm, running_var=rv, num_batches_tracked=nbt), lv)


SPADE_P = dict(w0=(16, 1, 3, 3), b0=(16,), wg=(CH, 16, 3, 3), bg=(CH,), wb=(CH, 16, 3, 3), bb=(CH,))


def spade_run(d):
    from mga_yolo_amd import SpadeConfig, mask_spade
    lv = {k: _leaf(d[k]) for k in ("x", "mask", *SPADE_P)}
    y = mask_spade(lv["x"], lv["mask"], [lv[k] for k in SPADE_P], SpadeConfig(hidden=16))
    y.backward(d["gy"])
    return _grads(dict(y=y.detach()), lv)


def gate_inputs(cl):
    g = _g(5)
    return dict(p=torch.rand(B, 1, H, W, generator=g), u1=torch.rand(B, 1, H, W, generator=g), u2=torch.rand(B, 1, H, W, generator=g),
                gout=torch.randn(B, 1, H, W, generator=g))


def gate_run(d):
    from mga_yolo_amd import prob_mask_gate
    p = _leaf(d["p"])
    out = prob_mask_gate(p, d["u1"], d["u2"], tau=0.7, p_min=0.05)
    out.backward(d["gout"])
    return dict(out=out.detach(), gp=p.grad)


def resize_inputs(cl):
    return dict(src=torch.randn(B, 1, H, W, generator=_g(6)))


def resize_run(d):
    from mga_yolo_amd import resize_nearest
    return dict(up=resize_nearest(d["src"], 13, 11), down=resize_nearest(d["src"], 3, 5))        # (a gather: no backward)


def seg_inputs(cl):
    g = _g(7)
    return dict(p3=torch.randn(B, 1, H, W, generator=g), p4=torch.randn(B, 1, H // 2, W // 2, generator=g),
                t3=(torch.rand(B, 1, 2 * H, 2 * W, generator=g) > 0.5).float(), t4=(torch.rand(B, 1, 2 * H, 2 * W, generator=g) > 0.5).float())


def seg_run(d):
    from mga_yolo_amd import SegLossConfig, SegmentationLoss
    p3, p4 = _leaf(d["p3"]), _leaf(d["p4"])
    total, logs = SegmentationLoss(SegLossConfig(scale_weights=(1.0, 0.5, 0.25)))({"p3": p3, "p4": p4}, [d["t3"], d["t4"]])
    total.backward()
    return dict(total=total.detach(), gp3=p3.grad, gp4=p4.grad, logs=torch.tensor([logs[k] for k in sorted(logs)], dtype=torch.float64))


def kendall_inputs(cl):
    g = _g(8)
    return dict(det=torch.rand(3, generator=g), seg=torch.rand((), generator=g), log_vars=0.2 * torch.randn(2, generator=g),
                gt=torch.randn(3, generator=g))


def kendall_run(d):
    from mga_yolo_amd import kendall_combine
    lv = {k: _leaf(d[k]) for k in ("det", "seg", "log_vars")}
    total = kendall_combine(lv["det"], lv["seg"], lv["log_vars"])
    total.backward(d["gt"])
    return _grads(dict(total=total.detach()), lv)


CASES = {
    "mask_cbam": (lambda cl: _feature_inputs(1, cl, CBAM_P), cbam_run, True),
    "mask_eca": (lambda cl: _feature_inputs(2, cl, ECA_P), eca_run, True),
    "mask_head": (lambda cl: _feature_inputs(3, cl, HEAD_P), head_run, True),
    "mask_spade": (lambda cl: _feature_inputs(4, cl, SPADE_P), spade_run, False),
    "prob_mask_gate": (gate_inputs, gate_run, False),
    "resize_nearest": (resize_inputs, resize_run, False),
    "SegmentationLoss": (seg_inputs, seg_run, False),
    "kendall_combine": (kendall_inputs, kendall_run, False),
}
PARAMS = [(name, cl) for name, (_, _, has_cl) in CASES.items() for cl in ((False, True) if has_cl else (False,))]


def run_default(name, cl, dev):
    """The case on the current stream -> {output name: tensor}, synchronised."""
    inputs, run, _ = CASES[name]
    out = run({k: v.to(dev) for k, v in inputs(cl).items()})
    torch.cuda.synchronize(dev)
    return out


@pytest.fixture(scope="module")
def busy(dev):
    """Unrelated work for the side stream (warmed up here, so the timed part of a test never pays a library's first-call set-up)."""
    a = torch.randn(2048, 2048, device=dev) / 64
    b = torch.empty_like(a)
    torch.mm(a, a, out=b)
    torch.cuda.synchronize(dev)
    return a, b


def run_side(name, cl, dev, busy):
    inputs, run, _ = CASES[name]
    src = {k: v.to(dev) for k, v in inputs(cl).items()}
    staged = {k: torch.zeros_like(v) for k, v in src.items()}          # (zeros_like keeps channels_last)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(16):
            torch.mm(busy[0], busy[0], out=busy[1])
        for k in staged:
            staged[k].copy_(src[k])
        out = run(staged)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    return out


@pytest.mark.parametrize("name,cl", PARAMS, ids=[f"{n}-{'channels_last' if c else 'contiguous'}" for n, c in PARAMS])
def test_side_stream_run_equals_default_stream_run(dev, busy, name, cl):
    a, a2 = run_default(name, cl, dev), run_default(name, cl, dev)
    b = run_side(name, cl, dev, busy)
    assert sorted(a) == sorted(a2) == sorted(b)
    bad = []
    for k in sorted(a):
        assert a[k] is not None and a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert bool(torch.isfinite(a[k].double()).all()), k
        if k in ("y", "gx") and cl:
            assert b[k].is_contiguous(memory_format=torch.channels_last) and a[k].is_contiguous(memory_format=torch.channels_last), k
        own = float((a2[k].double() - a[k].double()).abs().max())
        got = float((b[k].double() - a[k].double()).abs().max())
        same = torch.equal(a[k], a2[k])
        print(f"{name} cl={int(cl)} {k}: default twice {'bit-identical' if same else f'max|diff|={own:.3e}'}; side vs default max|diff|={got:.3e}")
        if (same and not torch.equal(a[k], b[k])) or got > own:
            bad.append(f"{k}: side {got:.3e} > own {own:.3e}")
    assert not bad, bad
    assert all(float(v.double().abs().max()) > 0 for v in a.values())        # (no output is trivially zero in both runs)
