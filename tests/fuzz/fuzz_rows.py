"""Randomised parity fuzz of the smaller rows on the GPU box: segmentation loss (both modes, random level counts / sizes / target
resolutions / weights / dtypes) vs its oracle evaluated in fp64, and the ProbMaskGater launch vs the module's host math on the same
uniforms.  A fraction of the loss cases runs a second time at training sizes: levels up to about 30,000 pixels (several outer trips of
k_seg_partial, every slot of its batches), B up to 80 (second trip of k_seg_final's sample loop) and / or bilinear resampling of soft
targets (MGA_PROB_MODE set around the module call and restored).  What those runs draw comes from a second generator seeded by the case
index: the cases of the original stream stay what they were.
    python tests/fuzz/fuzz_rows.py [n_cases] [seed]"""
import os, random, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch
from oracle import loss_rows as LR
from oracle import segloss_oracle as SO
from mga_yolo_amd import ProbMaskGater, SegLossConfig, SegmentationLoss, prob_mask_gate

n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0


def seg_case(it, what, preds, tg, kw, dt, B, keys, bilinear=False, gscale=1.0):
    global bad
    po = {k: v.double().clone().requires_grad_(True) for k, v in preds.items()}
    to, lo = SO.forward(po, [t.double() for t in tg], SO.SegLossConfig(**kw), bilinear_targets=bilinear)
    (to * gscale).backward()
    pd = {k: v.cuda().requires_grad_(True) for k, v in preds.items()}
    saved = os.environ.pop("MGA_PROB_MODE", None)
    try:
        if bilinear:
            os.environ["MGA_PROB_MODE"] = "1"
        td, ld = SegmentationLoss(SegLossConfig(**kw))(pd, [t.cuda() for t in tg])
    finally:
        os.environ.pop("MGA_PROB_MODE", None)
        if saved is not None:
            os.environ["MGA_PROB_MODE"] = saved
    (td * gscale).backward()
    tol = {torch.float32: 1e-4, torch.float16: 6e-3, torch.bfloat16: 4e-2}[dt]     # half: the gradient is rounded to the logits' dtype
    errs = {k: abs(ld[k] - lo[k]) / max(1.0, abs(lo[k])) for k in lo}
    for k in preds:
        w = po[k].grad
        errs["g_" + k] = float((pd[k].grad.double().cpu() - w).abs().max()) / (float(w.abs().max()) + 1e-12) * (1e-4 / tol)
    worst = max(errs.values())
    if not worst < 1e-4:
        bad += 1
        shapes = {k: tuple(v.shape[-2:]) for k, v in preds.items()}
        print(f"FAIL case {it}: {what} {dt} B={B} keys={keys} shapes={shapes} ufl={kw['use_unified_focal']} -> "
              f"{({k: f'{v:.2e}' for k, v in errs.items() if v >= 1e-4})}", flush=True)


for it in range(n):
    g = torch.Generator().manual_seed(9000 + it)
    try:
        if it % 2 == 0:                                                      # ---- segmentation loss
            B = rng.choice([1, 2, 3, 7, 16])
            keys = rng.sample(["p3", "p4", "p5"], rng.randint(1, 3))
            dt = rng.choice([torch.float32, torch.float32, torch.float16, torch.bfloat16])
            preds, tg = {}, []
            for i, k in enumerate(("p3", "p4", "p5")):
                H, W = rng.randint(1, 40), rng.randint(1, 40)
                if k in keys:
                    preds[k] = (torch.randn(B, 1, H, W, generator=g) * rng.choice([0.5, 2.0, 8.0])).to(dt)
                th, tw = (H, W) if rng.random() < 0.5 else (rng.randint(1, 90), rng.randint(1, 90))
                t = (torch.rand(B, 1, th, tw, generator=g) > rng.choice([0.5, 0.9, 0.99])).float()
                tg.append(t.squeeze(1) if rng.random() < 0.3 else t)
            kw = dict(bce_weight=rng.uniform(0.2, 2), dice_weight=rng.uniform(0.2, 2), smooth=rng.choice([1.0, 0.1, 5.0]),
                      scale_weights=tuple(rng.uniform(0.2, 2) for _ in range(3)), loss_lambda=rng.uniform(0.3, 2),
                      use_unified_focal=rng.random() < 0.4, ufl_lambda=rng.uniform(0.1, 0.9), ufl_delta=rng.uniform(0.2, 0.8),
                      ufl_gamma=rng.uniform(0.2, 0.9))
            seg_case(it, "segloss", preds, tg, kw, dt, B, keys)
            rng2 = random.Random(1_000_003 * (it + 1))
            if rng2.random() < 0.4:                                          # this case again at training sizes and / or bilinear targets
                bil = rng2.random() < 0.6
                big = rng2.random() < 0.6 or not bil
                B2 = rng2.choice([B, 65, 80]) if big else B
                g2 = torch.Generator().manual_seed(950000 + it)
                ufl_bil = bil and kw["use_unified_focal"]
                preds2, tg2 = {}, []
                for i, k in enumerate(("p3", "p4", "p5")):
                    if big and i == 0:
                        H, W = rng2.choice([(1, rng2.randint(8193, 30000)), (rng2.randint(91, 173), rng2.randint(91, 173))])
                    else:
                        H, W = rng2.randint(1, 40), rng2.randint(1, 40)
                    if ufl_bil:                                              # Unified Focal decides t > 0.5 on the resampled target: small levels whose
                        H, W = rng2.randint(1, 24), rng2.randint(1, 24)      # targets are kept clear of 0.5 (oracle/loss_rows.py), no large ones
                    if k in keys:
                        preds2[k] = (torch.randn(B2, 1, H, W, generator=g2) * rng2.choice([0.5, 2.0])).to(dt)
                    th, tw = (H, W) if rng2.random() < 0.3 else (rng2.randint(1, 90), rng2.randint(1, 90))
                    if ufl_bil:
                        t0 = LR.targets_for(B2, (th, tw), True, 960000 + 10 * it + i)
                        t = LR.soft_targets_clear_of_half(B2, (th, tw), (H, W), 960000 + 10 * it + i, 1.5 * LR.ufl_margin(LR.d_row(t0, (H, W))))
                    elif bil:
                        t = torch.rand(B2, 1, th, tw, generator=g2)
                    else:
                        t = (torch.rand(B2, 1, th, tw, generator=g2) > rng2.choice([0.5, 0.9])).float()
                    tg2.append(t.squeeze(1) if rng2.random() < 0.3 else t)
                # half-precision gradients of 1 / (B H W) fall below the type's normal range: a loss scale, as a trainer's GradScaler applies
                seg_case(it, f"segloss+ ({'bilinear' if bil else 'nearest'}{', large' if big else ''})", preds2, tg2, kw, dt, B2, keys, bilinear=bil,
                         gscale=1.0 if dt == torch.float32 else 4096.0)
        else:                                                                # ---- ProbMaskGater launch
            shape = (rng.randint(1, 6), 1, rng.randint(1, 50), rng.randint(1, 50))
            p = torch.rand(shape, generator=g) * 1.8 - 0.4
            u1, u2 = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
            tau, pmin, thr, hard = rng.choice([0.3, 1.0, 2.5]), rng.choice([0.0, 0.0, 0.15]), rng.uniform(0.2, 0.8), rng.random() < 0.5
            gout = torch.randn(shape, generator=g)
            x = p.clone().requires_grad_(True)                               # host math on the same uniforms
            q = x.clamp(0.0, 1.0)
            if pmin > 0:
                q = q.clamp_min(pmin)
            lo_, hi_ = 1e-6, 1 - 1e-6
            noise = torch.log(-torch.log(u2.clamp(lo_, hi_))) - torch.log(-torch.log(u1.clamp(lo_, hi_)))
            qq = q.clamp(lo_, hi_)
            soft = torch.sigmoid((torch.log(qq) - torch.log1p(-qq) + noise) / tau)
            ref = (soft > thr).float() + (soft - soft.detach()) if hard else soft
            ref.backward(gout)
            xd = p.cuda().requires_grad_(True)
            out = prob_mask_gate(xd, u1.cuda(), u2.cuda(), tau, pmin, thr, hard)
            out.backward(gout.cuda())
            near = (soft.detach() - thr).abs() < 1e-6                        # decisions within rounding of the threshold may flip
            ok_v = bool(((out.detach().cpu() - ref.detach()).abs() <= 2e-6 + 1.0 * near.float()).all())
            gw = x.grad
            ok_g = float((xd.grad.cpu() - gw).abs().max()) <= 1e-4 * float(gw.abs().max()) + 1e-7
            if not (ok_v and ok_g):
                bad += 1
                print(f"FAIL case {it}: gater shape={shape} tau={tau} pmin={pmin} hard={hard} value_ok={ok_v} grad_ok={ok_g}", flush=True)
    except Exception as ex:   # noqa: BLE001
        bad += 1
        print(f"ERROR case {it}: {type(ex).__name__}: {ex}", flush=True)
print(f"rows fuzz: {n - bad}/{n} cases within tolerance")
sys.exit(1 if bad else 0)
