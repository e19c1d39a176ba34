"""The detection matching (include/ext/mgamatch.h: two launches) beside a device-side torch composition that mirrors the validator's
per-image loop, read-backs included, and beside this repository's host path, in the same process.

    python tools/bench_match.py [--rounds 5] [--steps 20] [--out profiles/match/bench_match.json]

Inputs: B = 32 images of 640 x 640, max_det = 300 and every count 300 (the validator's own settings: conf 0.001, multi_label), nc = 1 and
nc = 80, with 10 and 200 labels per image, one per cell of a 15 x 15 grid; a detection is a jittered copy of one of its image's labels, nine in
ten of the label's class.  Ten thresholds.  Per row, the timed things:
  fused_graph   DetMatchPlan.run, accumulation included, captured in a graph and replayed (what the matching costs behind a captured
                post-process); the accumulation is sized for a round and reset between rounds, outside the clock
  fused_eager   match_detections(...): the public call, buffers allocated, the descriptor filled and m_cap read back per call
  torch_loop    per image, on the device: select the image's label rows, scale them, box IoU of labels x detections, the class mask; the IoU
                matrix is read back and the ten thresholds are matched on the host by the sort / unique / unique procedure in numpy; three
                more read-backs fetch conf, the predicted and the target classes.  B x 4 read-backs a batch, as in the validator
  host          match_detections on host tensors: the batched torch-op statement of the rule
Protocol: everything is built, compared and warmed first -- the graph replay, the eager call and the host path bit for bit, the loop by its tp
(reported, not asserted: random inputs are not guarded against equal IoUs) -- then timed in alternating rounds of `steps` calls each, the
clock read after a device synchronise; a row reports each side's median over the rounds and its spread (max - min over the rounds).  No
figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

B, D, SIZE, GRID = 32, 300, 640, 15
CONFIGS = {"nc1_l10": (1, 10), "nc1_l200": (1, 200), "nc80_l10": (80, 10), "nc80_l200": (80, 200)}


def make(nc, L, seed=5):
    rs = np.random.RandomState(seed)
    cell = SIZE / GRID
    cells = np.stack([rs.permutation(GRID * GRID)[:L] for _ in range(B)])                      # (B, L)
    wh = cell * rs.uniform(0.5, 0.85, (B, L, 2))
    cxy = (np.stack((cells % GRID, cells // GRID), -1) + 0.5) * cell
    lcls = rs.randint(0, nc, (B, L)).astype(np.float32)
    pick = rs.randint(0, L, (B, D))
    bi = np.arange(B)[:, None]
    jit = 1 + rs.uniform(-0.25, 0.25, (B, D, 2))
    dxy = cxy[bi, pick] + rs.uniform(-0.1, 0.1, (B, D, 2)) * wh[bi, pick]
    dwh = wh[bi, pick] * jit
    dcls = np.where(rs.uniform(size=(B, D)) < 0.9, lcls[bi, pick], rs.randint(0, nc, (B, D)))
    conf = -np.sort(-rs.uniform(0.001, 0.99, (B, D)), 1)
    dets = np.concatenate((dxy - dwh / 2, dxy + dwh / 2, conf[..., None], dcls[..., None]), -1).astype(np.float32)
    order = rs.permutation(B * L)                                                              # the flat label list, out of order
    batch_idx = np.repeat(np.arange(B), L)[order].astype(np.float32)
    cls = lcls.reshape(-1, 1)[order]
    bboxes = (np.concatenate((cxy, wh), -1) / SIZE).reshape(-1, 4)[order].astype(np.float32)
    t = torch.from_numpy
    return t(dets), torch.full((B,), D, dtype=torch.int32), t(batch_idx), t(cls), t(bboxes)


def match_numpy(iou, thrs):
    """the host half of the loop: the pairs over a threshold by descending IoU, each detection's first pair, then each label's first"""
    out = np.zeros((iou.shape[1], len(thrs)), dtype=bool)
    for t, thr in enumerate(thrs):
        li, di = np.nonzero(iou >= thr)
        if li.size == 0:
            continue
        pairs = np.stack((li, di), 1)
        if len(pairs) > 1:
            pairs = pairs[np.argsort(iou[li, di])[::-1]]
            pairs = pairs[np.unique(pairs[:, 1], return_index=True)[1]]
            pairs = pairs[np.unique(pairs[:, 0], return_index=True)[1]]
        out[pairs[:, 1], t] = True
    return out


def torch_loop(dets, count, batch_idx, cls, bboxes, thrs):
    """The validator's loop on device tensors: per image the tp matrix and the three arrays its stats take."""
    from mga_yolo_amd.detlabels import label_boxes
    out = []
    for b in range(dets.shape[0]):
        rows = batch_idx == b
        lc, lb = cls[rows].squeeze(-1), label_boxes(bboxes[rows], SIZE, SIZE)
        p = dets[b, :int(D)]
        iw = (torch.minimum(lb[:, None, 2], p[None, :, 2]) - torch.maximum(lb[:, None, 0], p[None, :, 0])).clamp(min=0)
        ih = (torch.minimum(lb[:, None, 3], p[None, :, 3]) - torch.maximum(lb[:, None, 1], p[None, :, 1])).clamp(min=0)
        inter = iw * ih
        area_l, area_d = (lb[:, 2] - lb[:, 0]) * (lb[:, 3] - lb[:, 1]), (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
        iou = inter / (area_l[:, None] + area_d[None, :] - inter + 1e-7)
        iou = (iou * (lc[:, None] == p[:, 5])).cpu().numpy()                                   # read-back 1
        out.append((match_numpy(iou, thrs), p[:, 4].cpu().numpy(), p[:, 5].cpu().numpy(), lc.cpu().numpy()))    # read-backs 2, 3, 4
    return out


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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--slow-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out", default=os.path.join("profiles", "match", "bench_match.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least 5 rounds"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path for device tensors"
    from mga_yolo_amd import DetMatchPlan, match_detections
    dev = torch.device("cuda", 0)
    thrs = torch.linspace(0.5, 0.95, 10).tolist()
    rows = []
    for cfg, (nc, L) in CONFIGS.items():
        if a.only and cfg not in a.only:
            continue
        host_in = make(nc, L)
        dets, count, bi, cl, bx = (t.to(dev) for t in host_in)
        per_round = max(a.steps, a.warmup) + 1
        plan = DetMatchPlan.create(B, D, n_cap=bi.numel(), m_cap=min(max(L, 1), 256), imgsz=SIZE, rows_cap=per_round * B * D,
                                   tgt_cap=per_round * B * L, dets=dets, count=count)
        plan.set_labels(bi, cl, bx)
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
            return match_detections(dets, count, bi, cl, bx, imgsz=SIZE)

        def loop():
            return torch_loop(dets, count, bi, cl, bx, thrs)

        def host():
            return match_detections(*host_in, imgsz=SIZE)
        plan.reset()
        graph.replay()
        tp_e, iou_e, gt_e = fused_eager()
        tp_h, iou_h, gt_h = host()
        ref = loop()
        torch.cuda.synchronize(dev)
        plan.check_status()
        assert torch.equal(plan.tp.bool(), tp_e) and torch.equal(plan.best_iou, iou_e) and torch.equal(plan.best_gt, gt_e)
        assert torch.equal(tp_e.cpu(), tp_h) and torch.equal(iou_e.cpu(), iou_h) and torch.equal(gt_e.cpu(), gt_h)
        same = sum(int(np.array_equal(tp_h[b].numpy(), r[0])) for b, r in enumerate(ref))
        sides = dict(fused_graph=(graph.replay, a.steps), fused_eager=(fused_eager, a.steps), torch_loop=(loop, a.slow_steps), host=(host, a.slow_steps))
        for k, (fn, steps) in sides.items():
            plan.reset()
            timed(fn, 1 if steps == a.slow_steps else a.warmup, dev)
        ms = {k: [] for k in sides}
        for _ in range(a.rounds):                                    # alternate the sides
            for k, (fn, steps) in sides.items():
                plan.reset()
                ms[k].append(timed(fn, steps, dev))
        plan.check_status()
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        row = dict(config=cfg, B=B, max_det=D, nc=nc, labels_per_image=L, niou=10, true_entries=int(tp_h.sum()), images_the_loop_matches_the_same=same)
        for k in ms:
            row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(spread[k], 5), [round(v, 5) for v in ms[k]]
        row["fused_graph_vs_torch_loop"] = round(med["torch_loop"] / med["fused_graph"], 1)
        row["fused_graph_vs_host"] = round(med["host"] / med["fused_graph"], 1)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
        del graph, plan
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, slow_steps=a.slow_steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
