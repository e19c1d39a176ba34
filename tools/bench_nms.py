"""The detection post-process (include/mganms.h: two launches) beside this repository's own torch composition of the same post-process on
the device, in the same process.

    python tools/bench_nms.py [--rounds 5] [--steps 20] [--out profiles/nms/bench_nms.json]

Inputs: trained-like Detect maps (background bins 0.5 n, class logits uniform in [-5.5, -2.7]; about 8 boxes per image whose anchors predict
them with a jitter of a cell and a class logit of 1.5 + n), fp32, at B = 32, 640 x 640 with nc = 1 and nc = 80, and at B = 8, 1280 x 1280
with nc = 1; each at conf 0.001 (validation: every anchor is a candidate) and 0.25 (predict).  multi_label is off, max_det 300, max_nms 30000.
Per row, the timed things:
  fused_graph   DetPostPlan.run captured in a graph and replayed (what the post-process costs behind a captured forward)
  fused_eager   detect_postprocess(feats, ...): the public call, buffers allocated and the descriptor filled per call
  torch_eager   the torch composition: the decode in about ten ops, then per image boolean-mask indexing, an argsort and a greedy NMS.
                torchvision.ops.nms is used if it imports; otherwise the IoU-matrix form: the n x n matrix of suppressions and the fixed
                point keep[j] = not any(keep[i] and M[i, j], i < j), iterated until it stops changing (the row says which).  It cannot be
                captured: every image's sizes are read back to the host.
Protocol: everything is built, compared and warmed first -- the graph replay and the eager call bit for bit, the torch composition by the
rows it keeps (reported, not asserted: random features are not guarded against near-ties) -- then timed in alternating rounds of `steps`
calls each, the clock read after a device synchronise; a row reports each side's median over the rounds and its spread (max - min over the
rounds).  No figure is fixed in advance.

    python tools/bench_nms.py --channels-last [--dtype fp32 fp16] [--out profiles/det_nhwc/bench_nms_channels_last.json]

The maps' layout instead, at B = 32, 640 x 640 with nc = 1 and nc = 80 and both thresholds, three graph replays in alternating rounds:
  nchw          NCHW maps through DetPostPlan
  copy          channels_last maps the way they went before the kernels read them in place: a copy of every level into NCHW maps, then the
                NCHW plan
  native        channels_last maps through DetPostPlan(channels_last=True): no copy
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
CONFS = (0.001, 0.25)
STRIDES = (8, 16, 32)
BOXES = 8
IOU, MAX_DET, MAX_NMS = 0.45, 300, 30000

try:
    from torchvision.ops import nms as tv_nms
except Exception:                                                  # not installed here: the IoU-matrix form stands in
    tv_nms = None


def make(B, size, nc, seed=3):
    g = torch.Generator().manual_seed(seed)
    j = torch.arange(16.0)
    feats = []
    wh = size * (0.08 + 0.4 * torch.rand(B, BOXES, 2, generator=g))
    xy = wh / 2 + (size - wh) * torch.rand(B, BOXES, 2, generator=g)
    box = torch.cat((xy - wh / 2, xy + wh / 2), -1)                # (B, BOXES, 4)
    cls = torch.randint(0, nc, (B, BOXES), generator=g)
    for s in STRIDES:
        h = size // s
        f = 0.5 * torch.randn(B, 64 + nc, h, h, generator=g)
        f[:, 64:] = -5.5 + 2.8 * torch.rand(B, nc, h, h, generator=g)
        c = (torch.arange(h) + 0.5) * s
        py, px = torch.meshgrid(c, c, indexing="ij")
        for b in range(B):
            for q in range(BOXES):
                x1, y1, x2, y2 = box[b, q].tolist()
                t = torch.stack((px - x1, py - y1, x2 - px, y2 - py)) / s                # (4, h, h)
                m = (t.amin(0) > 0) & (t.amax(0) <= 15)
                if not m.any():
                    continue
                n = int(m.sum())
                tt = (t[:, m] + torch.rand(4, n, generator=g) * 2 - 1).clamp(0, 15)     # (4, n)
                bins = -(j.view(1, 16, 1) - tt.view(4, 1, n)) ** 2 / 1.5 + 0.3 * torch.randn(4, 16, n, generator=g)
                f[b, :64][:, m] = bins.reshape(64, n)
                f[b, 64 + int(cls[b, q])][m] = 1.5 + torch.randn(n, generator=g)
        feats.append(f)
    return feats


def torch_postprocess(feats, nc, conf):
    """The composition: returns per image (rows (n, 6), kept anchor indices)."""
    from mga_yolo_amd.detpost import _decode
    boxes, prob = _decode(feats, STRIDES, nc)                      # (B, A, 4), (B, A, nc)
    out = []
    for b in range(boxes.shape[0]):
        score, c = prob[b].max(1)
        a = torch.nonzero(score > conf).flatten()
        order = score[a].argsort(descending=True, stable=True)[:MAX_NMS]
        a = a[order]
        bx, sc, cl = boxes[b][a], score[a], c[a]
        if tv_nms is not None:
            k = tv_nms(bx + cl[:, None].float() * 7680, sc, IOU)[:MAX_DET]
        else:
            area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            iw = (torch.minimum(bx[:, None, 2], bx[None, :, 2]) - torch.maximum(bx[:, None, 0], bx[None, :, 0])).clamp_(min=0)
            ih = (torch.minimum(bx[:, None, 3], bx[None, :, 3]) - torch.maximum(bx[:, None, 1], bx[None, :, 1])).clamp_(min=0)
            inter = iw.mul_(ih)
            M = (inter / (area[:, None] + area[None, :] - inter) > IOU) & (cl[:, None] == cl[None, :])
            M = M.triu_(1).float()
            keep = torch.ones(a.numel(), device=a.device)
            while True:                                            # after t iterations the first t candidates are final
                new = (keep @ M == 0).float()
                if torch.equal(new, keep):
                    break
                keep = new
            k = torch.nonzero(keep).flatten()[:MAX_DET]
        out.append((torch.cat((bx[k], sc[k, None], cl[k, None].float()), 1), a[k]))
    return out


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
    from mga_yolo_amd import DetPostPlan
    dev = torch.device("cuda", 0)
    rows = []
    for cfg, (B, size, nc) in list(CONFIGS.items())[:2]:
        if a.only and cfg not in a.only:
            continue
        made = make(B, size, nc)
        for name in a.dtype:
            dtype = dict(fp32=torch.float32, fp16=torch.float16, bf16=torch.bfloat16)[name]
            feats = [f.to(dev, dtype) for f in made]
            src = [f.contiguous(memory_format=torch.channels_last) for f in feats]
            shapes = [(B, f.shape[2], f.shape[3]) for f in feats]
            for conf in CONFS:
                kw = dict(nc=nc, strides=STRIDES, conf_thres=conf, iou_thres=IOU, max_det=MAX_DET, max_nms=MAX_NMS)
                nchw = DetPostPlan.create(shapes, feats=feats, **kw)
                staged = DetPostPlan.create(shapes, dtype=dtype, **kw)           # the copy's destination: NCHW maps of the plan's own
                native = DetPostPlan.create(shapes, feats=src, channels_last=True, **kw)

                def step_copy():
                    for dst, f in zip(staged.feats, src):
                        dst.copy_(f)
                    staged.run()
                graphs = dict(nchw=capture(nchw.run, dev), copy=capture(step_copy, dev), native=capture(native.run, dev))
                for g in graphs.values():
                    g.replay()
                torch.cuda.synchronize(dev)
                native.check_status()
                for other in (nchw, staged):
                    assert torch.equal(native.dets, other.dets) and torch.equal(native.count, other.count) and torch.equal(native.keep, other.keep)
                for g in graphs.values():
                    timed(g.replay, a.warmup, dev)
                ms = {k: [] for k in graphs}
                for _ in range(a.rounds):                            # alternate the arms
                    for k, g in graphs.items():
                        ms[k].append(timed(g.replay, a.steps, dev))
                med = {k: statistics.median(v) for k, v in ms.items()}
                row = dict(config=cfg, dtype=name, B=B, size=size, nc=nc, conf_thres=conf, kept_rows=int(native.count.sum()),
                           map_bytes=sum(f.numel() for f in feats) * feats[0].element_size())
                for k in ms:
                    row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(max(ms[k]) - min(ms[k]), 5), [round(v, 5) for v in ms[k]]
                pair = [c - n for c, n in zip(ms["copy"], ms["native"])]      # the interleaved pairs' own differences
                row["copy_minus_native_ms"], row["copy_minus_native_spread_ms"] = round(statistics.median(pair), 5), round(max(pair) - min(pair), 5)
                row["native_vs_nchw"] = round(med["native"] / med["nchw"], 3)
                row["native_is_the_faster"] = bool(statistics.median(pair) > max(pair) - min(pair))
                rows.append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
                del graphs, nchw, staged, native
            del feats, src
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--torch-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--channels-last", action="store_true", help="time the maps' layouts instead: NCHW, channels_last by copy, channels_last native")
    ap.add_argument("--dtype", nargs="*", default=["fp32", "fp16"], choices=["fp32", "fp16", "bf16"], help="with --channels-last")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.out = a.out or (os.path.join("profiles", "det_nhwc", "bench_nms_channels_last.json") if a.channels_last else os.path.join("profiles", "nms", "bench_nms.json"))
    assert a.rounds >= 5, "at least 5 rounds"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    from mga_yolo_amd import DetPostPlan, detect_postprocess
    dev = torch.device("cuda", 0)
    rows = layouts(a) if a.channels_last else []
    for cfg, (B, size, nc) in ({} if a.channels_last else CONFIGS).items():
        if a.only and cfg not in a.only:
            continue
        feats = [f.to(dev) for f in make(B, size, nc)]
        for conf in CONFS:
            kw = dict(nc=nc, strides=STRIDES, conf_thres=conf, iou_thres=IOU, max_det=MAX_DET, max_nms=MAX_NMS)
            plan = DetPostPlan.create([(B, f.shape[2], f.shape[3]) for f in feats], feats=feats, **kw)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                plan.run()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                plan.run()

            def fused_eager():
                return detect_postprocess(feats, **kw)

            def torch_eager():
                return torch_postprocess(feats, nc, conf)
            graph.replay()
            d_e, c_e, k_e = fused_eager()
            ref = torch_eager()
            torch.cuda.synchronize(dev)
            plan.check_status()
            assert torch.equal(plan.dets, d_e) and torch.equal(plan.count, c_e) and torch.equal(plan.keep, k_e)
            counts = c_e.tolist()
            same = sum(int(counts[b] == r[1].numel() and torch.equal(k_e[b, :counts[b]].long(), r[1])) for b, r in enumerate(ref))
            sides = dict(fused_graph=(graph.replay, a.steps), fused_eager=(fused_eager, a.steps), torch_eager=(torch_eager, a.torch_steps))
            for k, (fn, steps) in sides.items():
                timed(fn, 1 if k == "torch_eager" else a.warmup, dev)
            ms = {k: [] for k in sides}
            for _ in range(a.rounds):                                # alternate the sides
                for k, (fn, steps) in sides.items():
                    ms[k].append(timed(fn, steps, dev))
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            row = dict(config=cfg, B=B, size=size, nc=nc, conf_thres=conf, anchors=sum(f.shape[2] * f.shape[3] for f in feats),
                       kept_rows=sum(counts), images_torch_keeps_the_same_rows=same, torch_nms="torchvision.ops.nms" if tv_nms else "IoU matrix")
            for k in ms:
                row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(spread[k], 5), [round(v, 5) for v in ms[k]]
            row["fused_graph_vs_torch_eager"] = round(med["torch_eager"] / med["fused_graph"], 1)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
            del graph, plan
        del feats
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, torch_steps=a.torch_steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
