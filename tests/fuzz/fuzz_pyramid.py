"""Randomised fuzz of the multi-level entry point: 2-5 levels per call with mixed shapes, conv sizes, mask / no mask, dtypes of
their own -- exercises the launch-group partition (levels with different compile-time signatures go to different launches), the
longest-first level ordering and the XCD-aligned grids.  Every level is checked against the oracle.  After each grouped call a random
subset of its levels runs again as single-level calls (mask_cbam) with fresh inputs on the same pooled ctxs: the call composition
changes under one ctx (batches up to 32 make the launch group's channels per thread differ between the two forms).  Every call, and
every single-level re-run, runs once more with a layout drawn per level (NCHW or channels_last, at least one channels_last), against the
same oracle results: mixed-layout launch groups, and pooled ctxs that see both layouts.  Some calls run again with a level of the
channels-last tiling's larger shapes added (several tiles per chunk, scalar lanes with C > 64).  What those runs draw comes from a
second generator seeded by the call index: the NCHW calls are those of the original stream.
    python tests/fuzz/fuzz_pyramid.py [n_calls] [seed]"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from conftest import rel_err, synth
from oracle import maskcbam_oracle as O
from mga_yolo_amd import functional as F

n = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
only = {int(a.split("=", 1)[1]) for a in sys.argv if a.startswith("--only=")}       # re-run single calls of a campaign (same random stream)
repeat = max([int(a.split("=", 1)[1]) for a in sys.argv if a.startswith("--repeat=")] + [1])
bad = 0
ties = 0            # samples with a channel arg-max near-tie (their gy is zeroed, every check kept)
tie_levels = 0      # levels with at least one such sample


CL = torch.channels_last
# channels-last level shapes past the pool's: more than 64 tiles per sample (rp >= 2, ragged last chunk), scalar lanes with C > 64
CL_EXTRA = [(2, 130, 48, 47), (1, 16, 190, 190), (2, 256, 40, 52), (1, 72, 140, 120), (3, 130, 23, 17), (1, 68, 101, 99)]


def run_call(it, spec, seed0=7000, tag="", layouts=(None,)):
    """Oracle once per level of spec, then the device call once per entry of layouts (None: every level NCHW, else a memory format per
    level)."""
    global ties, tie_levels
    ref = []
    for l, (B, C, H, W, k, kind, dt, mask_grad) in enumerate(spec):
        x, mask, gy = synth(B, C, H, W, seed=seed0 + 10 * it + l, mask_kind=kind)
        x, gy = x.to(dt).float(), gy.to(dt).float()
        p = O.Params.default_init(C, k=k, seed=it + l)
        y_o, c = O.forward(x, mask, p)
        # a channel arg-max decided by less than the last bits of ca (x_c ca_c of the two best channels within 2e-6 relative): the oracle's
        # and the device's ca differ by ~1e-7, so the routed sub-gradient may go to either channel -- y agrees, gx differs at that pixel.
        # Such samples get gy = 0 on both sides: they contribute exactly nothing to any gradient, the other samples are checked in full
        if C > 1:
            u2 = (x * c.ca.reshape(B, C, 1, 1)).topk(2, dim=1).values
            tied = ((u2[:, 0] - u2[:, 1]) <= 2e-6 * u2[:, 0].abs()).flatten(1).any(dim=1)
            gy[tied] = 0
            ties += int(tied.sum())
            tie_levels += int(bool(tied.any()))
        g_o = O.backward(gy, x, mask, p, O.Config(), c)
        ref.append((y_o, g_o, gy, dt, (B, C, H, W, k, kind), (x, mask, p, mask_grad)))
    for fmts in layouts:
        device_call(it, ref, tag if fmts is None else tag + " layouts " + "".join("C" if f is CL else "N" for f in fmts),
                    fmts or [torch.contiguous_format] * len(ref))


def device_call(it, ref, tag, fmts):
    global bad
    lv = []
    for (y_o, g_o, gy, dt, (B, C, H, W, k, kind), (x, mask, p, mask_grad)), fmt in zip(ref, fmts):
        xd = x.cuda().to(dt).to(memory_format=fmt).requires_grad_(True)
        md = None if mask is None else mask.cuda().requires_grad_(mask_grad)
        ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
        lv.append((xd, md, ps, F.BlockConfig(hidden=p.w1.shape[0], k=k)))
    try:
        ys = F.mask_cbam_pyramid(lv) if len(lv) > 1 else (F.mask_cbam(lv[0][0], lv[0][1], *lv[0][2], lv[0][3]),)
        torch.autograd.backward(list(ys), [r[2].cuda().to(r[3]).to(memory_format=f) for r, f in zip(ref, fmts)])
        for l, ((xd, md, ps, _), (y_o, g_o, gy, dt, desc, _), fmt) in enumerate(zip(lv, ref, fmts)):
            if fmt is CL and desc[1] > 1 and desc[2] * desc[3] > 1 and not (ys[l].is_contiguous(memory_format=CL) and xd.grad.is_contiguous(memory_format=CL)):
                bad += 1
                print(f"FAIL call {it}{tag} level {l} {desc} {dt}: y / gx came back in another layout", flush=True)
            tol = {torch.float32: 1e-4, torch.float16: 4e-3, torch.bfloat16: 3e-2}[dt]
            floor = 1e-7 * float(gy.norm() * xd.detach().float().norm().cpu())   # absolute: fp32 rounding of a cancelling sum's terms
            checks = dict(y=(ys[l].float(), y_o), gx=(xd.grad.float(), g_o["gx"]), gw1=(ps[0].grad, g_o["gw1"]), gwsa=(ps[4].grad, g_o["gwsa"]),
                          gbeta=(ps[5].grad, g_o["gbeta"]), gw2=(ps[2].grad, g_o["gw2"]))
            if md is not None and md.requires_grad:
                checks["gmask"] = (md.grad, g_o["gmask"])
            for name, (got, want) in checks.items():
                d = (got.detach().double().cpu() - want.double()).abs()
                dv = float(d.max())
                bar = tol * float(want.double().abs().max()) + (floor if name not in ("y", "gx") else 0.0)
                if not dv <= max(bar, 1e-30):
                    bad += 1
                    where = [int(v) for v in torch.unravel_index(d.argmax(), d.shape)]
                    print(f"FAIL call {it}{tag} level {l} {desc} {dt}: {name} |diff| {dv:.2e} > {bar:.2e} at {where}, {int((d > bar).sum())} elements over the bar",
                          flush=True)
    except Exception as ex:   # noqa: BLE001
        bad += 1
        print(f"ERROR call {it}{tag}: {[r[4] for r in ref]}: {type(ex).__name__}: {ex}", flush=True)


def draw_layouts(rng2, nl):
    fmts = [rng2.choice([CL, torch.contiguous_format]) for _ in range(nl)]
    fmts[rng2.randrange(nl)] = CL
    return fmts


BUDGET = 16 << 20   # feature elements per call: the oracle runs on the CPU

for it in range(n):
    rng2 = random.Random(1_000_003 * (it + 1))
    nl = rng.randint(2, 5)
    spec = []
    for l in range(nl):
        B = rng.choice([1, 2, 4, 8, 11, 16, 32])
        C = rng.choice([8, 16, 64, 128, 192, 256])
        H, W = rng.choice([(20, 20), (8, 8), (17, 17), (5, 12), (40, 40), (3, 3)])
        if B > 11 and (H * W > 1600 or C > 256 or sum(s_[0] * s_[1] * s_[2] * s_[3] for s_ in spec) + B * C * H * W > BUDGET):
            B = rng.choice([1, 2, 4, 8, 11])        # batches of 16 / 32 (group cpt > 1) within the per-call budget
        k = rng.choice([7, 7, 3, 5, 9])
        kind = rng.choice(["randn", "sparse", "none", "mixed"]) if B > 1 else rng.choice(["randn", "none"])
        dt = rng.choice([torch.float32, torch.float32, torch.float16, torch.bfloat16])
        mask_grad = rng.random() < 0.8 if kind != "none" else False              # (drawn only when the level has a mask)
        spec.append((B, C, H, W, k, kind, dt, mask_grad))
    alone = [l for l in range(nl) if rng.random() < 0.5]                    # levels that run again on their own after the grouped call
    if only and it not in only:
        continue
    mixed = draw_layouts(rng2, nl)
    alone_fmt = {l: draw_layouts(rng2, 1) for l in alone}
    extra = None
    if rng2.random() < 0.25:                      # + a level of the channels-last tiling's larger shapes, after the call's first levels
        B, C, H, W = rng2.choice(CL_EXTRA)
        extra = spec[:rng2.randint(1, nl)] + [(B, C, H, W, rng2.choice([7, 3, 5, 9]), rng2.choice(["randn", "sparse", "none"]),
                                                rng2.choice([torch.float32, torch.float16, torch.bfloat16]), True)]
        extra = (extra, draw_layouts(rng2, len(extra)))
    for _ in range(repeat):
        run_call(it, spec, layouts=(None, mixed))
        for l in alone:
            run_call(it, [spec[l]], seed0=1000000 * (l + 1), tag=f" (level {l} alone)", layouts=(None, alone_fmt[l]))
        if extra is not None:
            run_call(it, extra[0], tag=" (+ a larger level)", layouts=(extra[1],))
    if only:
        print(f"call {it}: {[(s_[:6], str(s_[6]).replace('torch.', ''), s_[7]) for s_ in spec]}", flush=True)
print(f"pyramid fuzz: {n} calls, {bad} failures ({ties} samples in {tie_levels} levels with a channel arg-max near-tie: gy zeroed there, "
      "every check kept)")
sys.exit(1 if bad else 0)
