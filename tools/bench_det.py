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
advance.  bytes = every feature element read once by the loss sweep and once by the gradient sweep, plus the gradients written.

    python tools/bench_det.py --channels-last [--dtype fp32 fp16] [--out profiles/det_nhwc/bench_det_channels_last.json]

The maps' layout instead: B = 32 at 640 x 640 with nc = 1 and nc = 80, three graph replays in alternating rounds:
  nchw          NCHW maps through DetLossPlan (forward + backward)
  copy          channels_last maps the way they went before the kernels read them in place: a copy of every level into the NCHW plan's maps,
                the NCHW kernels, a copy of every gradient level into channels_last buffers
  native        channels_last maps through DetLossPlan(channels_last=True): no copy
The three are compared bit for bit before anything is timed."""
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


def capture(step, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph


def layouts(a):
    """--channels-last: the three arms of the module docstring"""
    from mga_yolo_amd import DetLossPlan
    dev = torch.device("cuda", 0)
    cl = torch.channels_last
    rows = []
    for cfg, (B, size, nc) in list(CONFIGS.items())[:2]:
        for name in a.dtype:
            dtype = dict(fp32=torch.float32, fp16=torch.float16, bf16=torch.bfloat16)[name]
            feats, bidx, cls, bb = make(B, size, nc, dev)
            feats = [f.to(dtype) for f in feats]
            src = [f.contiguous(memory_format=cl) for f in feats]           # what a channels_last model leaves
            g_cl = [torch.empty_like(f) for f in src]
            up = torch.ones(3, device=dev)
            shapes = [(B, f.shape[2], f.shape[3]) for f in feats]
            kw = dict(n_cap=bidx.numel(), m_cap=BOXES, g_out=up, dtype=dtype)
            nchw, native = DetLossPlan.create(shapes, nc, **kw), DetLossPlan.create(shapes, nc, channels_last=True, **kw)
            for plan in (nchw, native):
                for dst, f in zip(plan.feats, feats):
                    dst.copy_(f)
                plan.set_labels(bidx, cls, bb)

            def step_nchw():
                nchw.forward(); nchw.backward()

            def step_copy():
                for dst, f in zip(nchw.feats, src):
                    dst.copy_(f)
                nchw.forward(); nchw.backward()
                for dst, g in zip(g_cl, nchw.g_feats):
                    dst.copy_(g)

            def step_native():
                native.forward(); native.backward()
            graphs = dict(nchw=capture(step_nchw, dev), copy=capture(step_copy, dev), native=capture(step_native, dev))
            for g in graphs.values():
                g.replay()
            torch.cuda.synchronize(dev)
            native.check_status()
            assert torch.equal(native.out, nchw.out) and torch.equal(native.items, nchw.items)
            assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(native.g_feats, nchw.g_feats, g_cl))
            for g in graphs.values():
                timed(g.replay, a.warmup, dev)
            ms = {k: [] for k in graphs}
            for _ in range(a.rounds):                                # alternate the arms
                for k, g in graphs.items():
                    ms[k].append(timed(g.replay, a.steps, dev))
            med = {k: statistics.median(v) for k, v in ms.items()}
            elems = sum(f.numel() for f in feats)
            row = dict(config=cfg, dtype=name, B=B, size=size, nc=nc, anchors=sum(f.shape[2] * f.shape[3] for f in feats),
                       map_bytes=elems * feats[0].element_size(), loss=[float(v) for v in native.out])
            for k in ms:
                row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(max(ms[k]) - min(ms[k]), 5), [round(v, 5) for v in ms[k]]
            pair = [c - n for c, n in zip(ms["copy"], ms["native"])]          # the interleaved pairs' own differences
            row["copy_minus_native_ms"], row["copy_minus_native_spread_ms"] = round(statistics.median(pair), 5), round(max(pair) - min(pair), 5)
            row["native_vs_nchw"] = round(med["native"] / med["nchw"], 3)
            row["native_is_the_faster"] = bool(statistics.median(pair) > max(pair) - min(pair))
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
            del graphs, nchw, native, feats, src, g_cl
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--torch-steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--channels-last", action="store_true", help="time the maps' layouts instead: NCHW, channels_last by copy, channels_last native")
    ap.add_argument("--dtype", nargs="*", default=["fp32", "fp16"], choices=["fp32", "fp16", "bf16"], help="with --channels-last")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.out = a.out or (os.path.join("profiles", "det_nhwc", "bench_det_channels_last.json") if a.channels_last else os.path.join("profiles", "det", "bench_det.json"))
    assert a.rounds >= 5 and a.steps >= 20, "at least 5 rounds of at least 20 steps"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    from mga_yolo_amd import DetLossPlan, detection_loss
    from mga_yolo_amd.detloss import _host_loss
    dev = torch.device("cuda", 0)
    rows = layouts(a) if a.channels_last else []
    for cfg, (B, size, nc) in ({} if a.channels_last else CONFIGS).items():
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
