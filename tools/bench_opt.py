"""The tail of a training step after the backward -- unscale + non-finite check, clip_grad_norm_, optimizer step, EMA -- fused into the
static step's graph (mga_yolo_amd/optim.py: two launches) beside the same tail in eager torch on the same tensors, in the same process.

    python tools/bench_opt.py [--rounds 5] [--steps 200] [--out profiles/opt/bench_opt.json]

Shapes: YOLOv8n widths at 640 px (P3/P4/P5 = 64x80x80, 128x40x40, 256x20x20), the MaskCBAM slice in NCHW fp32, at batch 4 (the reference's
default) and batch 32; SGD and AdamW.  Per row, four timed things:
  fused_step   one graph: plan.step(); opt.step()
  torch_step   the graph of plan.step(), then the eager torch tail: _amp_foreach_non_finite_check_and_unscale_, clip_grad_norm_(10.0),
               the foreach torch.optim.SGD(nesterov) / AdamW in three groups, and the EMA loop as the reference writes it
               (U/utils/torch_utils.py:766-774) over the same parameters and running buffers.  GradScaler.step's found_inf.item(), a host
               synchronisation, is NOT in it: the torch side is timed at its best.
  fused_tail   opt.step() alone, as a graph of its own
  torch_tail   the eager torch tail alone
Protocol: everything is built and warmed first, then timed in alternating rounds of `steps` steps each, the clock read after a device
synchronise; a row reports each side's median over the rounds and its spread (max - min over the rounds), and whether the difference of
the medians exceeds the larger spread."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LEVELS = [(64, 80, 80), (128, 40, 40), (256, 20, 20)]
CONFIGS = {"default_b4": 4, "cfg2_b32": 32}


def make_plan(batch, dev):
    from mga_yolo_amd import MGAMaskHead, MaskCBAM, SlicePlan
    heads, blocks = [], []
    for C, _, _ in LEVELS:
        torch.manual_seed(0)
        heads.append(MGAMaskHead(C, max(8, C // 4)).to(dev).train())
        blocks.append(MaskCBAM(C).to(dev).train())
    shapes = [(batch, C, H, W) for C, H, W in LEVELS]
    plan = SlicePlan.create(shapes, [max(8, C // 4) for C, _, _ in LEVELS], [[p.detach().clone() for p in b.block_params()] for b in blocks],
                            [b.block_config() for b in blocks], [h.state_dict() for h in heads], block="cbam", device=dev)
    g = torch.Generator().manual_seed(7)
    for l, (B, C, H, W) in enumerate(shapes):
        plan.x[l].copy_(torch.nn.functional.silu(torch.randn(B, C, H, W, generator=g)).to(dev))
        plan.gy[l].copy_(torch.randn(B, C, H, W, generator=g).to(dev))
        plan.targets[l].copy_((torch.rand(B, 1, H, W, generator=g) > 0.9).float().to(dev))
    plan.det_loss.copy_(torch.tensor([1.0, 0.5, 1.5], device=dev))
    return plan


def torch_tail_of(plan, kind, dev):
    """The eager tail over the plan's own tensors -> (callable, number of tensors)"""
    from mga_yolo_amd.optim import plan_segments
    segs = plan_segments(plan, ema=True)
    trained = [s for s in segs if s.grad is not None]
    for s in trained:
        s.param.grad = s.grad                                        # the views the backward fills
    g = [[s.param for s in trained if s.group == j] for j in range(3)]
    if kind == "sgd":
        opt = torch.optim.SGD(g[0], lr=1e-5, momentum=0.9, nesterov=True)
    else:
        opt = torch.optim.AdamW(g[0], lr=1e-6, betas=(0.9, 0.999), weight_decay=0.0)
    opt.add_param_group({"params": g[1], "weight_decay": 5e-4})
    opt.add_param_group({"params": g[2], "weight_decay": 0.0})
    params, grads = [s.param for s in trained], [s.grad for s in trained]
    msd = {s.name: s.param for s in segs}
    ema = {k: v.clone() for k, v in msd.items()}
    found_inf, inv_scale = torch.zeros(1, device=dev), torch.ones(1, device=dev)
    state = dict(updates=0)

    def tail():
        torch._amp_foreach_non_finite_check_and_unscale_(grads, found_inf, inv_scale)
        torch.nn.utils.clip_grad_norm_(params, max_norm=10.0)
        opt.step()
        state["updates"] += 1
        d = 0.9999 * (1 - math.exp(-state["updates"] / 2000))
        for k, v in ema.items():
            v *= d
            v += (1 - d) * msd[k].detach()
    return tail, len(trained), len(segs)


def timed(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "opt", "bench_opt.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.steps >= 20, "at least 5 rounds of at least 20 steps"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    dev = torch.device("cuda", 0)
    rows = []
    for cfg, batch in CONFIGS.items():
        for kind in ("sgd", "adamw"):
            fused_plan, torch_plan = make_plan(batch, dev), make_plan(batch, dev)
            opt = BucketOptimizer.for_plan(fused_plan, OptConfig(kind, lr=1e-5 if kind == "sgd" else 1e-6))   # (the inputs never change: a small lr keeps 1000 steps on them tame)
            fused_graph = opt.capture(fused_plan)
            tail_graph = opt.capture(fused_plan, opt.step)
            plan_graph = torch_plan.capture(torch_plan.step)
            tail, n_trained, n_segs = torch_tail_of(torch_plan, kind, dev)
            sides = dict(fused_step=fused_graph.replay, torch_step=lambda: (plan_graph.replay(), tail()), fused_tail=tail_graph.replay,
                         torch_tail=tail, plan_alone=plan_graph.replay)
            for fn in sides.values():
                timed(fn, a.warmup, dev)
            ms = {k: [] for k in sides}
            for _ in range(a.rounds):                                # alternate the sides
                for k, fn in sides.items():
                    ms[k].append(timed(fn, a.steps, dev))
            fused_plan.check_handoff(); torch_plan.check_handoff()
            assert int(opt.found_inf) == 0 and math.isfinite(float(opt.grad_norm))
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            row = dict(config=cfg, batch=batch, optimizer=kind, tensors=n_trained, segments=n_segs, elements=int(fused_plan.grad_bucket.numel()),
                       chunks=int(sum((s.param.numel() + 1023) // 1024 for s in opt.segments)))
            for k in sides:
                row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 4), round(spread[k], 4), [round(v, 4) for v in ms[k]]
            row["step_speedup"] = round(med["torch_step"] / med["fused_step"], 2)
            row["tail_speedup"] = round(med["torch_tail"] / med["fused_tail"], 2)
            row["step_difference_exceeds_spread"] = bool(abs(med["torch_step"] - med["fused_step"]) > max(spread["torch_step"], spread["fused_step"]))
            row["tail_difference_exceeds_spread"] = bool(abs(med["torch_tail"] - med["fused_tail"]) > max(spread["torch_tail"], spread["fused_tail"]))
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
            del sides, fused_graph, tail_graph, plan_graph, opt, tail, fused_plan, torch_plan
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
