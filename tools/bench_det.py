"""The detection criterion, forward + backward (include/mgadet.h: four launches + one), beside this repository's own torch composition of
the same criterion on the device (mga_yolo_amd.detloss._host_loss on device tensors + autograd), in the same process.

    python tools/bench_det.py [--rounds 5] [--steps 50] [--out profiles/det/bench_det.json]

Shapes: B = 32 at 640 x 640 with nc = 1 and nc = 80, B = 8 at 1280 x 1280 with nc = 1; about 8 boxes per image, fp32 features.
Per row, the timed things:
  fused_graph   DetLossPlan.forward + backward captured in a graph and replayed (what the criterion costs inside the static step)
  fused_eager   detection_loss(..., m_cap=) + autograd backward: the public call, buffers allocated and the descriptor filled per call
  torch_eager   the torch composition, forward + backward.  It cannot be captured: it sizes tensors from the labels and indexes with masks,
                which read back to the host, as the reference's criterion does
Protocol: everything is built, compared and warmed first, then timed in alternating rounds of `steps` calls each, the clock read after a
device synchronise; a row reports each side's median over the rounds and its spread (max - min over the rounds).  No figure is fixed in
advance.  bytes = every feature element read once by the loss sweep and once by the gradient sweep, plus the gradients written."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CONFIGS = {"b32_640_nc1": (32, 640, 1), "b32_640_nc80": (32, 640, 80), "b8_1280_nc1": (8, 1280, 1)}
STRIDES = (8, 16, 32)
BOXES = 8


def make(B, size, nc, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 64 + nc, size // s, size // s, generator=g).to(dev) for s in STRIDES]
    n = B * BOXES
    bidx = torch.arange(B).repeat_interleave(BOXES).float()
    wh = 0.05 + 0.45 * torch.rand(n, 2, generator=g)
    xy = wh / 2 + (1 - wh) * torch.rand(n, 2, generator=g)
    cls = torch.randint(0, nc, (n,), generator=g).float()
    return feats, bidx.to(dev), cls.to(dev), torch.cat((xy, wh), 1).to(dev)


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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "det", "bench_det.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.steps >= 20, "at least 5 rounds of at least 20 steps"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    from mga_yolo_amd import DetLossPlan, detection_loss
    from mga_yolo_amd.detloss import _host_loss
    dev = torch.device("cuda", 0)
    rows = []
    for cfg, (B, size, nc) in CONFIGS.items():
        feats, bidx, cls, bb = make(B, size, nc, dev)
        up = torch.ones(3, device=dev)
        plan = DetLossPlan.create([(B, f.shape[2], f.shape[3]) for f in feats], nc, n_cap=bidx.numel(), m_cap=BOXES, g_out=up)
        for dst, f in zip(plan.feats, feats):
            dst.copy_(f)
        plan.set_labels(bidx, cls, bb)

        def step():
            plan.forward(); plan.backward()
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()

        def fused_eager():
            xs = [f.requires_grad_(True) for f in feats]
            loss, _ = detection_loss(xs, bidx, cls, bb, nc=nc, m_cap=BOXES)
            return loss, torch.autograd.grad(loss.sum(), xs)

        def torch_eager():
            xs = [f.requires_grad_(True) for f in feats]
            loss, _, _ = _host_loss(xs, bidx, cls, bb, nc, STRIDES, (7.5, 0.5, 1.5), 10)
            return loss, torch.autograd.grad(loss.sum(), xs)
        # the sides compute the same thing: the eager call bit for bit, the torch composition to rounding
        graph.replay()
        l_f, g_f = fused_eager()
        l_t, g_t = torch_eager()
        torch.cuda.synchronize(dev)
        plan.check_status()
        assert torch.equal(plan.out, l_f) and all(torch.equal(x, y) for x, y in zip(plan.g_feats, g_f))
        rel = float(((l_f - l_t).abs() / l_t.abs().clamp(min=1e-6)).max())
        grel = max(float((x - y).abs().max() / y.abs().max().clamp(min=1e-12)) for x, y in zip(g_f, g_t))
        assert rel < 1e-4 and grel < 1e-3, (rel, grel)
        sides = dict(fused_graph=(graph.replay, a.steps), fused_eager=(fused_eager, a.steps), torch_eager=(torch_eager, a.torch_steps))
        for fn, _ in sides.values():
            timed(fn, min(a.warmup, 3) if fn is torch_eager else a.warmup, dev)
        ms = {k: [] for k in sides}
        for _ in range(a.rounds):                                    # alternate the sides
            for k, (fn, steps) in sides.items():
                ms[k].append(timed(fn, steps, dev))
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        elems = sum(f.numel() for f in feats)
        row = dict(config=cfg, B=B, size=size, nc=nc, boxes_per_image=BOXES, anchors=sum(f.shape[2] * f.shape[3] for f in feats),
                   loss=[float(v) for v in l_f], loss_rel_diff_torch=rel, grad_rel_diff_torch=grel, bytes=elems * 4 * 3)
        for k in ms:
            row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(spread[k], 5), [round(v, 5) for v in ms[k]]
        row["fused_graph_vs_torch_eager"] = round(med["torch_eager"] / med["fused_graph"], 1)
        row["fused_graph_GBps"] = round(row["bytes"] / (med["fused_graph"] * 1e-3) / 1e9, 1)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
        del graph, plan, feats
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, torch_steps=a.torch_steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
