"""Randomised parity fuzz of the mask head on the GPU box: MGAMaskHead (HIP path: mgahead_forward / mgahead_backward) vs its oracle on
random shapes -- channels / hidden widths that are not multiples of 16 or 4, odd H*W (scalar-lane path), tiny and wide images, hidden up
to 384 (several M blocks), train and eval mode, fp32 / fp16 / bf16 features, single and two-level calls.  Every case
runs again on channels_last features (a fresh module from the same state) against the same oracle result; a second generator seeded by
the case index draws the extra cases -- a hidden width of 200 / 256 / 384 at the case's shape (eval mode for some half-precision ones), in
both layouts, and for every fifth case the second level of a two-level mask_head_pyramid call, each level compared with its own oracle --
so the first run of every case is that of the original stream.
    python tests/fuzz/fuzz_head.py [n_cases] [seed]"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from oracle import maskhead_oracle as HO
from mga_yolo_amd import MGAMaskHead, mask_head_pyramid

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-20))


def check(it, desc, m, x, gl, lo, c, go, training, dt, fmt):
    """-> None when module m on the device (x in layout fmt) meets the bars against the oracle's (lo, c, go), else the failure line."""
    md = m.cuda()
    xd = x.cuda().to(memory_format=fmt).requires_grad_(True)
    y = md(xd)
    y.backward(gl.cuda())
    return compare(it, desc, md, xd, y, lo, c, go, training, dt, "channels_last" if fmt is torch.channels_last else "nchw")


def compare(it, desc, md, xd, y, lo, c, go, training, dt, layout):
    """The bars, on a module that has run forward and backward on xd."""
    hid = md.proj[0].weight.shape[0]
    B, C, H, W = xd.shape
    fmt = torch.channels_last
    if layout == "channels_last" and C > 1 and H * W > 1 and not xd.grad.is_contiguous(memory_format=fmt):
        return f"FAIL {it}: {desc} {layout}: gx came back in another layout"
    tol = {torch.float32: 2e-4, torch.float16: 6e-3, torch.bfloat16: 4e-2}[dt]
    n_px = B * H * W
    if training and n_px < 4:
        tol = max(tol, 1e-1)          # batch statistics over 1-3 values: zhat = +-1, the BatchNorm backward cancels to eps-level terms and the
                                      # fp32 oracle is itself only good to a few percent of what is left (v_exp/v_rcp SiLU: 1e-6 in, 4e-2 out)
    errs = dict(logits=rel(y.float(), lo), gx=rel(xd.grad.float(), go["gx"]), gw1=rel(md.proj[0].weight.grad.reshape(hid, C), go["gw1"]),
                ggamma=rel(md.proj[1].weight.grad, go["ggamma"]), gbeta=rel(md.proj[1].bias.grad, go["gbeta"]),
                gwh=rel(md.head.weight.grad, go["gwh"]), gbh=rel(md.head.bias.grad, go["gbh"]),
                rmean=rel(md.proj[1].running_mean, c.new_running_mean), rvar=rel(md.proj[1].running_var, c.new_running_var))
    if training and n_px < 4:
        # gx / dW1 through a BatchNorm over 2-3 values cancel to rounding noise in exact arithmetic (zhat = +-1): there is no signal to compare
        errs.pop("gx"); errs.pop("gw1")
    if n_px < 4 and dt != torch.float32:
        # one to three logits from half-precision features: the relative error of a single cancelling dot product (weights rounded to the
        # feature type for the MFMA) is not bounded by the tensor-scale tolerance -- nothing to compare at this size
        return None
    worst = max(errs, key=errs.get)
    if not errs[worst] < tol or any(v != v for v in errs.values()):
        return f"FAIL {it}: {desc} {layout}: {worst} {errs[worst]:.3e}  all={ {k: f'{v:.1e}' for k, v in errs.items()} }"
    return None


def fresh(C, hid, sd, eps_mom, training):
    m = MGAMaskHead(C, hid)
    m.load_state_dict(sd)
    m.proj[1].eps, m.proj[1].momentum = eps_mom
    return m.train(training)


def case(it, g, B, C, hid, H, W, dt, training, eps_mom, fmts):
    """One module state and input, the oracle once, then the device in each layout of fmts (a fresh module from that state each time).
    -> what a later two-level call needs of it, or None."""
    global bad
    desc = f"B={B} C={C} hid={hid} H={H} W={W} {dt} train={training}"
    try:
        torch.manual_seed(it)
        m = MGAMaskHead(C, hid)
        with torch.no_grad():
            for p_ in m.parameters():
                p_.add_(0.3 * torch.randn(p_.shape, generator=g))
            bn = m.proj[1]
            bn.running_mean.add_(0.2 * torch.randn(hid, generator=g)); bn.running_var.mul_(0.5 + torch.rand(hid, generator=g))
        bn.eps, bn.momentum = eps_mom
        m.train(training)
        x = torch.randn(B, C, H, W, generator=g).to(dt)
        gl = torch.randn(B, 1, H, W, generator=g).to(dt)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        p = HO.HeadParams.from_state_dict(sd, eps=bn.eps, momentum=bn.momentum)
        lo, c = HO.forward(x.float(), p, training)
        go = HO.backward(gl.float(), x.float(), p, c, training)
        for i, fmt in enumerate(fmts):
            if i:
                m = fresh(C, hid, sd, eps_mom, training)
            line = check(it, desc, m, x, gl, lo, c, go, training, dt, fmt)
            if line:
                bad += 1
                print(line, flush=True)
        return dict(desc=desc, C=C, hid=hid, sd=sd, eps_mom=eps_mom, training=training, dt=dt, x=x, gl=gl, lo=lo, c=c, go=go)
    except ValueError as e:                                  # one value per channel in training mode: torch raises, and so does the HIP path
        if training and B * H * W == 1 and "more than 1 value per channel" in str(e):
            return
        bad += 1
        print(f"ERROR {it}: {desc}: {type(e).__name__}: {e}", flush=True)
    except Exception as e:                                   # noqa: BLE001
        bad += 1
        print(f"ERROR {it}: {desc}: {type(e).__name__}: {e}", flush=True)
    return None


def pyramid(it, levels):
    """The levels' NCHW features in ONE mask_head_pyramid call each way (fresh modules from the cases' states), each level against the
    oracle result of its own case."""
    global bad
    desc = " + ".join(d["desc"] for d in levels)
    try:
        mods = [fresh(d["C"], d["hid"], d["sd"], d["eps_mom"], d["training"]).cuda() for d in levels]
        xds = [d["x"].cuda().requires_grad_(True) for d in levels]
        lv = []
        for m, xd, d in zip(mods, xds, levels):
            bn = m.proj[1]
            lv.append((xd, m.proj[0].weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, m.head.weight,
                       m.head.bias, bn.eps, bn.momentum, d["training"]))
        ys = mask_head_pyramid(lv)
        torch.autograd.backward(ys, [d["gl"].cuda() for d in levels])
        for i, (m, xd, y, d) in enumerate(zip(mods, xds, ys, levels)):
            line = compare(it, d["desc"], m, xd, y, d["lo"], d["c"], d["go"], d["training"], d["dt"], f"nchw, level {i} of a two-level call")
            if line:
                bad += 1
                print(line, flush=True)
    except Exception as e:                                   # noqa: BLE001
        bad += 1
        print(f"ERROR {it}: pyramid {desc}: {type(e).__name__}: {e}", flush=True)


CL = torch.channels_last
for it in range(n):
    rng2 = random.Random(1_000_003 * (it + 1))
    g = torch.Generator().manual_seed(7000 + it)
    B = rng.choice([1, 2, 3, 5, 8])
    C = rng.choice([3, 8, 20, 48, 64, 96, 128, 130, 192, 256, 320, 512])
    hid = rng.choice([1, 4, 8, 12, 16, 24, 32, 40, 64, 96, 128, 200, 256, 384])
    H, W = rng.choice([(1, 1), (1, 9), (2, 3), (5, 7), (8, 8), (9, 7), (12, 20), (17, 17), (20, 20), (16, 40), (33, 5), (40, 40),
                        (3, 160), (2, 333), (1, 500), (2, 257), (6, 100), (3, 96)])      # wide rows: k_head_out's pixels-per-thread escalation, tiny outputs per run
    if B * C * H * W > 6_000_000:
        B = 1
    dt = rng.choice([torch.float32, torch.float32, torch.float32, torch.float16, torch.bfloat16])
    training = rng.random() < 0.75
    eps_mom = rng.choice([(1e-5, 0.1), (1e-3, 0.03)])
    first = case(it, g, B, C, hid, H, W, dt, training, eps_mom, (torch.contiguous_format, CL))
    # the widest M tilings of the head kernels (hidden above 192; at 384 more than 4 waves x 4 tiles) and eval mode in half precision, at
    # this case's shape with inputs of their own, in both layouts
    if rng2.random() < 0.25:
        hid2 = rng2.choice([200, 256, 384])
        dt2 = rng2.choice([dt, torch.float16, torch.bfloat16])
        train2 = training if dt2 == torch.float32 else rng2.random() < 0.5
        case(it, torch.Generator().manual_seed(900000 + it), B, C, hid2, H, W, dt2, train2, eps_mom, (torch.contiguous_format, CL))
    # every fifth case: a two-level call, this case's level beside a second one of another shape, width and element type
    if it % 5 == 4 and first is not None:
        B3, C3, hid3 = rng2.choice([1, 2, 3]), rng2.choice([6, 20, 64, 132]), rng2.choice([8, 24, 80, 144, 384])
        H3, W3 = rng2.choice([(3, 4), (7, 5), (12, 12), (2, 333), (16, 32)])
        dt3 = rng2.choice([torch.float32, torch.float16, torch.bfloat16])
        second = case(it, torch.Generator().manual_seed(800000 + it), B3, C3, hid3, H3, W3, dt3, rng2.random() < 0.75, eps_mom,
                      (torch.contiguous_format,))
        if second is not None:
            pyramid(it, [first, second])
    if it % 50 == 49:
        print(f"  {it + 1} cases, {bad} bad", flush=True)
print(f"fuzz_head: {n} cases, {bad} bad")
sys.exit(1 if bad else 0)
