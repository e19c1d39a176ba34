"""Randomised parity fuzz on the GPU box: many small random shapes / configurations of MaskCBAM and MaskECA through the HIP
path vs the oracles (1e-4 relative).  Exercises every launch-geometry branch (H*W odd / multiple of 4, C below / above the row
counts, B not a multiple of 8, generic conv sizes, no mask, raw-probability masks, tiny / empty masks, hidden 1..48).  Every MaskCBAM
case runs again on channels_last features against the same oracle result; some cases are replaced, for that second run alone, by a
larger shape (several tiles per chunk, or scalar lanes with C > 64) of the channels-last tiling.  What the channels-last runs draw comes
from a second generator seeded by the case index: the NCHW cases are those of the original stream.
    python tests/fuzz/fuzz_parity.py [n_cases] [seed]
"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from conftest import rel_err, synth
from oracle import maskcbam_oracle as O, maskeca_oracle as E
from mga_yolo_amd import functional as F

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
CL = torch.channels_last
# channels-last shapes past the NCHW pool's 28 x 28: more than 64 tiles per sample (rp >= 2, ragged last chunk) for 4..64 lanes per pixel,
# and scalar lanes (C % 4 != 0) with C > 64 (several channel-group passes, a partial 64-channel fold block)
CL_EXTRA = [(2, 130, 48, 47), (1, 16, 190, 190), (2, 256, 40, 52), (1, 68, 101, 99), (3, 130, 23, 17), (1, 322, 37, 61), (2, 40, 120, 41),
            (1, 200, 46, 50)]


def cbam_device(x, mask, gy, p, k, use_sig, fmt):
    xd = x.cuda().to(memory_format=fmt).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(True)
    ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    y = F.mask_cbam(xd, md, *ps, F.BlockConfig(hidden=p.w1.shape[0], k=k, use_sigmoid_mask=use_sig))
    y.backward(gy.cuda().to(memory_format=fmt))
    B_, C_, H_, W_ = x.shape
    if fmt is CL and C_ > 1 and H_ * W_ > 1:
        assert y.is_contiguous(memory_format=CL) and xd.grad.is_contiguous(memory_format=CL), "y / gx came back in another layout"
    return dict(y=y, gx=xd.grad, gmask=None if md is None else md.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad,
                gb2=ps[3].grad, gwsa=ps[4].grad, gbeta=ps[5].grad)


def errors(got, want, gy, x):
    # parameter gradients (and gmask) are long signed sums that may cancel to ~0: on top of 1e-4 relative allow the fp32
    # rounding of their terms, 1e-7 of |gy|.|x| (absolute)
    floor = 1e-7 * float(gy.norm() * x.norm())
    errs = {}
    for k_ in want:
        if want[k_] is None:
            continue
        wv = want[k_].double()
        dv = (got[k_].detach().double().cpu() - wv).abs().max()
        tol = 1e-4 * float(wv.abs().max()) + (floor if k_ not in ("y", "gx") else 0.0)
        errs[k_] = 1e-4 * float(dv) / max(tol, 1e-30)          # normalised so that the bar stays "< 1e-4"
    return errs, floor


def report(it, block, shape, kind, layout, got, want, errs, floor):
    global bad
    worst = max(errs.values()) if errs else 0.0
    if not worst < 1e-4:
        bad += 1
        B_, C_, H_, W_ = shape
        print(f"FAIL case {it}: {block} {layout} B={B_} C={C_} H={H_} W={W_} mask={kind} -> {({k_: f'{v:.2e}' for k_, v in errs.items() if v >= 1e-4})}", flush=True)
        for k_, v in errs.items():
            if v >= 1e-4 and want[k_].numel() <= 16:
                print(f"   {k_}: got {got[k_].detach().cpu().flatten().tolist()} want {want[k_].flatten().tolist()} floor {floor:.3e}", flush=True)


for it in range(n):
    rng2 = random.Random(1_000_003 * (it + 1))
    B = rng.choice([1, 2, 3, 5, 8, 9, 16])
    C = rng.choice([1, 2, 3, 7, 8, 16, 24, 48, 64, 96, 130, 256, 320])
    H, W = rng.randint(1, 28), rng.randint(1, 28)
    kind = rng.choice(["randn", "sparse", "mixed", "none", "all_negative", "tiny", "prob"])
    if kind == "mixed" and B < 2:
        kind = "randn"
    use_sig = kind != "prob"
    x, mask, gy = synth(B, C, H, W, seed=1000 + it, mask_kind=kind, x_kind=rng.choice(["randn", "relu", "quantized"]))
    block = rng.choice(["cbam", "cbam", "eca"])
    try:
        if block == "cbam":
            r = rng.choice([1, 2, 4, 16]); k = rng.choice([1, 3, 5, 7, 7, 9])
            p = O.Params.default_init(C, r=r, k=k, seed=it)
            with torch.no_grad():
                for t in (p.w1, p.b1, p.w2, p.b2, p.wsa):
                    t.add_(0.3 * torch.randn(t.shape))
                p.beta.fill_(rng.uniform(-1.5, 1.5))
            cfg = O.Config(use_sigmoid_mask=use_sig)
            y_o, c = O.forward(x, mask, p, cfg)
            g_o = O.backward(gy, x, mask, p, cfg, c)
            got = cbam_device(x, mask, gy, p, k, use_sig, torch.contiguous_format)
            want = dict(y=y_o, **g_o)
        else:
            p = E.EcaParams.default_init(C, seed=it)
            with torch.no_grad():
                p.w.add_(0.3 * torch.randn(p.w.shape)); p.beta.fill_(rng.uniform(-1.5, 1.5))
            cfg = E.EcaConfig(use_sigmoid_mask=use_sig)
            y_o, t = E.forward(x, mask, p, cfg)
            g_o = E.backward(gy, x, mask, p, cfg, t)
            xd = x.cuda().requires_grad_(True)
            md = None if mask is None else mask.cuda().requires_grad_(True)
            w, beta = p.w.cuda().requires_grad_(True), p.beta.cuda().requires_grad_(True)
            y = F.mask_eca(xd, md, w, beta, F.EcaConfig(k=p.w.shape[-1], use_sigmoid_mask=use_sig))
            y.backward(gy.cuda())
            got = dict(y=y, gx=xd.grad, gmask=None if md is None else md.grad, gw=w.grad, gbeta=beta.grad)
            want = dict(y=y_o, **g_o)
        errs, floor = errors(got, want, gy, x)
        report(it, block, (B, C, H, W), kind, "nchw", got, want, errs, floor)
    except Exception as ex:   # noqa: BLE001
        bad += 1
        print(f"ERROR case {it}: {block} B={B} C={C} H={H} W={W} mask={kind}: {type(ex).__name__}: {ex}", flush=True)
    if block != "cbam":
        continue
    layout = "channels_last"
    try:
        if rng2.random() < 0.2:                        # this case's channels-last run takes a larger shape (and its own oracle)
            B, C, H, W = rng2.choice(CL_EXTRA)
            layout = "channels_last(extra shape)"
            if kind == "mixed" and B < 2:
                kind = "randn"
            use_sig = kind != "prob"
            x, mask, gy = synth(B, C, H, W, seed=500000 + it, mask_kind=kind, x_kind=rng2.choice(["randn", "relu", "quantized"]))
            p = O.Params.default_init(C, r=r, k=k, seed=it)
            with torch.no_grad():
                for t in (p.w1, p.b1, p.w2, p.b2, p.wsa):
                    t.add_(0.3 * torch.randn(t.shape))
                p.beta.fill_(rng2.uniform(-1.5, 1.5))
            cfg = O.Config(use_sigmoid_mask=use_sig)
            y_o, c = O.forward(x, mask, p, cfg)
            want = dict(y=y_o, **O.backward(gy, x, mask, p, cfg, c))
        got = cbam_device(x, mask, gy, p, k, use_sig, CL)
        errs, floor = errors(got, want, gy, x)
        report(it, block, (B, C, H, W), kind, layout, got, want, errs, floor)
    except Exception as ex:   # noqa: BLE001
        bad += 1
        print(f"ERROR case {it}: {block} {layout} B={B} C={C} H={H} W={W} mask={kind}: {type(ex).__name__}: {ex}", flush=True)
print(f"fuzz: {n - bad}/{n} cases within 1e-4")
sys.exit(1 if bad else 0)
