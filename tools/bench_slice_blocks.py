"""Graph-replay time of the layer-loop slice (mga_yolo_amd/slice.py) for every block, layout and element type, beside the eager module
composition of the same slice in the same process.

    python tools/bench_slice_blocks.py [--rounds 5] [--steps 40] [--out profiles/slice_blocks/bench_slice_blocks.json]

Shapes: YOLOv8n widths at 640 px (P3/P4/P5 = 64x80x80, 128x40x40, 256x20x20) at batch 32 (BASELINE.json configs[1]) and at batch 4 (the
reference's default batch).  Mask heads have hidden = C / 4 (yolov8_*.yaml, width-scaled); MaskSPADE its default hidden 64, instance norm.
Protocol: both sides are built and warmed first, then timed in alternating rounds (static, eager, static, ...) of `steps` steps each, the
clock read after a device synchronise; a row reports each side's median over the rounds and its spread (max - min over the rounds), and
whether the difference of the medians exceeds the larger spread."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

LEVELS = [(64, 80, 80), (128, 40, 40), (256, 20, 20)]
CONFIGS = {"cfg2_b32": 32, "default_b4": 4}
DTYPES = {"fp32": torch.float32, "fp16": torch.float16}


def build_modules(block, dev):
    from mga_yolo_amd import MGAMaskHead, MaskCBAM, MaskECA, MaskSPADE
    heads, blocks = [], []
    for C, _, _ in LEVELS:
        torch.manual_seed(0)
        heads.append(MGAMaskHead(C, max(8, C // 4)).to(dev).train())
        blocks.append({"cbam": MaskCBAM, "eca": MaskECA, "spade": MaskSPADE}[block](C).to(dev).train())
    return heads, blocks


def block_args(block, blocks):
    if block == "cbam":
        return [b.block_params() for b in blocks], [b.block_config() for b in blocks]
    if block == "eca":
        return [(b.conv1d.weight, b.beta) for b in blocks], [b.eca_config() for b in blocks]
    return [b.spade_params() for b in blocks], [b.spade_config() for b in blocks]


def make_row(block, cl, dtype, batch, dev):
    """-> (static step, eager step, launches): two callables over the same shapes and the same seeded inputs"""
    from mga_yolo_amd import SegLossConfig, SegmentationLoss, SlicePlan, kendall_combine
    heads, blocks = build_modules(block, dev)
    shapes = [(batch, C, H, W) for C, H, W in LEVELS]
    hidden = [max(8, C // 4) for C, _, _ in LEVELS]
    params, cfgs = block_args(block, blocks)
    plan = SlicePlan.create(shapes, hidden, params, cfgs, [h.state_dict() for h in heads], block=block, channels_last=cl, dtype=dtype, device=dev)
    fmt = torch.channels_last if cl else torch.contiguous_format
    g = torch.Generator().manual_seed(7)
    data, targets = [], []
    for l, (B, C, H, W) in enumerate(shapes):
        x = torch.nn.functional.silu(torch.randn(B, C, H, W, generator=g)).to(dev, dtype).contiguous(memory_format=fmt)
        gy = torch.randn(B, C, H, W, generator=g).to(dev, dtype).contiguous(memory_format=fmt)
        t = (torch.rand(B, 1, H, W, generator=g) > 0.9).float().to(dev)
        plan.x[l].copy_(x); plan.gy[l].copy_(gy); plan.targets[l].copy_(t)
        data.append((x.requires_grad_(True), gy)); targets.append(t)
    det = torch.tensor([1.0, 0.5, 1.5], device=dev)
    plan.det_loss.copy_(det)
    graph = plan.capture(plan.step)
    log_vars = torch.zeros(2, device=dev, requires_grad=True)
    crit = SegmentationLoss(SegLossConfig())
    leaves = [x for x, _ in data] + [log_vars] + [p for m in heads + blocks for p in m.parameters()]

    def eager():
        for t in leaves:                                         # optimizer.zero_grad(set_to_none=True), as the reference trainer does
            t.grad = None
        logits = [h(x) for h, (x, _) in zip(heads, data)]
        ys = [b([x, m]) for b, (x, _), m in zip(blocks, data, logits)]
        seg_total, _ = crit(dict(zip(("p3", "p4", "p5"), logits)), targets)
        total = kendall_combine(det, seg_total, log_vars)
        torch.autograd.backward([total.sum()] + ys, [None] + [gy for _, gy in data])

    return graph.replay, eager, plan.launches(), plan


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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", default="cbam,eca,spade")
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join("profiles", "slice_blocks", "bench_slice_blocks.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.steps >= 20, "at least 5 rounds of at least 20 steps"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    dev = torch.device("cuda", 0)
    rows = []
    for cfg in a.configs.split(","):
        for block in a.blocks.split(","):
            for cl in (False, True):
                for dname, dtype in DTYPES.items():
                    static, eager, launches, plan = make_row(block, cl, dtype, CONFIGS[cfg], dev)
                    for fn in (static, eager):                   # warm every shape on both sides
                        timed(fn, a.warmup, dev)
                    s_ms, e_ms = [], []
                    for _ in range(a.rounds):                    # alternate the two sides
                        s_ms.append(timed(static, a.steps, dev))
                        e_ms.append(timed(eager, a.steps, dev))
                    plan.check_handoff()
                    sm, em = statistics.median(s_ms), statistics.median(e_ms)
                    spread = max(max(s_ms) - min(s_ms), max(e_ms) - min(e_ms))
                    row = dict(config=cfg, batch=CONFIGS[cfg], block=block, layout="channels_last" if cl else "nchw", dtype=dname,
                               static_ms=round(sm, 4), eager_ms=round(em, 4), static_spread_ms=round(max(s_ms) - min(s_ms), 4),
                               eager_spread_ms=round(max(e_ms) - min(e_ms), 4), speedup=round(em / sm, 2),
                               difference_exceeds_spread=bool(abs(em - sm) > spread), static_rounds_ms=[round(v, 4) for v in s_ms],
                               eager_rounds_ms=[round(v, 4) for v in e_ms], launches=launches)
                    rows.append(row)
                    print(json.dumps({k: row[k] for k in ("config", "block", "layout", "dtype", "static_ms", "eager_ms", "static_spread_ms",
                                                          "eager_spread_ms", "difference_exceeds_spread")}), flush=True)
                    del static, eager, plan
                    torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
