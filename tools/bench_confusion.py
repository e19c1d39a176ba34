"""The confusion matrix on the device (include/ext/mgaconfusion.h: two launches) beside a device-side torch composition that mirrors the
reference's per-image ConfusionMatrix.process_batch, read-back included, and beside this repository's host path, in the same process; and
the captured chain post-process -> matching -> confusion matrix beside the chain without its third stage.

    python tools/bench_confusion.py [--rounds 5] [--steps 20] [--out profiles/confusion/bench_confusion.json]

Inputs: those of tools/bench_match.py -- B = 32 images of 640 x 640, max_det = 300 and every count 300, nc = 1 and nc = 80, with 10 and 200
labels per image; conf = 0.001 (the validator's default, which the reference turns into 0.25), iou_thres 0.45.  Per row, the timed things:
  cm_graph      ConfusionPlan.run, accumulation included, captured in a graph and replayed (what the third stage costs behind a captured
                matching)
  cm_eager      confusion_matrix(...): the public call, buffers allocated, the descriptor filled and m_cap read back per call
  torch_loop    per image, on the device: select the image's label rows, scale them, filter the detections by confidence, box IoU of
                labels x detections, torch.where(iou > thr), the pairs stacked and read back; then on the host the two argsort / unique
                passes and the two Python loops over labels and detections, as the reference runs them.  Two more read-backs fetch the classes
                (.int().tolist()).  B x 3 read-backs a batch
  host          confusion_matrix on host tensors: the batched torch-op statement of the rule
  chain2, chain3  a captured DetPostPlan.run -> DetMatchPlan.run, and the same with ConfusionPlan.run behind it, on three Detect levels of
                random maps (conf 0.001, max_det 300: the counts are what the post-process keeps, reported as mean_count); their difference
                is what the third stage adds to a captured validation step
Protocol: everything is built, compared and warmed first -- the graph replay, the eager call and the host path element for element, the
loop by its matrix (reported, not asserted: random inputs are not guarded against equal IoUs) -- then timed in alternating rounds of
`steps` calls each, the clock read after a device synchronise; a row reports each side's median over the rounds and its spread (max - min
over the rounds).  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_match import B, CONFIGS, D, SIZE, make, timed  # noqa: E402

CONF, IOU_THRES = 0.001, 0.45


def torch_loop(dets, batch_idx, cls, bboxes, nc):
    """process_batch's steps per image on device tensors, restated: the batch's matrix"""
    from mga_yolo_amd.detlabels import label_boxes
    matrix = np.zeros((nc + 1, nc + 1))
    conf = 0.25 if CONF in {None, 0.001} else CONF
    for b in range(dets.shape[0]):
        rows = batch_idx == b
        gt_cls, gt_boxes = cls[rows].squeeze(-1), label_boxes(bboxes[rows], SIZE, SIZE)
        p = dets[b]
        p = p[p[:, 4] > conf]
        gt_classes = gt_cls.int().tolist()                                                     # read-back 1
        det_classes = p[:, 5].int().tolist()                                                   # read-back 2
        iw = (torch.minimum(gt_boxes[:, None, 2], p[None, :, 2]) - torch.maximum(gt_boxes[:, None, 0], p[None, :, 0])).clamp(min=0)
        ih = (torch.minimum(gt_boxes[:, None, 3], p[None, :, 3]) - torch.maximum(gt_boxes[:, None, 1], p[None, :, 1])).clamp(min=0)
        inter = iw * ih
        area_l, area_d = (gt_boxes[:, 2] - gt_boxes[:, 0]) * (gt_boxes[:, 3] - gt_boxes[:, 1]), (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
        iou = inter / (area_l[:, None] + area_d[None, :] - inter + 1e-7)
        x = torch.where(iou > IOU_THRES)
        if x[0].shape[0]:
            m = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()      # read-back 3
            if x[0].shape[0] > 1:
                m = m[m[:, 2].argsort()[::-1]]
                m = m[np.unique(m[:, 1], return_index=True)[1]]
                m = m[m[:, 2].argsort()[::-1]]
                m = m[np.unique(m[:, 0], return_index=True)[1]]
        else:
            m = np.zeros((0, 3))
        n = m.shape[0] > 0
        m0, m1, _ = m.transpose().astype(int)
        for i, gc in enumerate(gt_classes):
            j = m0 == i
            if n and sum(j) == 1:
                matrix[det_classes[m1[j].item()], gc] += 1
            else:
                matrix[nc, gc] += 1
        for i, dc in enumerate(det_classes):
            if not any(m1 == i):
                matrix[dc, nc] += 1
    return matrix


def capture(dev, *plans):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for p in plans:
            p.run()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p in plans:
            p.run()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--slow-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--out", default=os.path.join("profiles", "confusion", "bench_confusion.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least 5 rounds"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path for device tensors"
    from mga_yolo_amd import ConfusionPlan, DetMatchPlan, DetPostPlan, confusion_matrix
    dev = torch.device("cuda", 0)
    rows = []
    for cfg, (nc, L) in CONFIGS.items():
        if a.only and cfg not in a.only:
            continue
        host_in = make(nc, L)
        dets, count, bi, cl, bx = (t.to(dev) for t in host_in)
        m_cap = min(max(L, 1), 256)
        per_round = max(a.steps, a.warmup) + 1
        plan = ConfusionPlan.create(B, D, nc=nc, n_cap=bi.numel(), m_cap=m_cap, imgsz=SIZE, conf=CONF, iou_thres=IOU_THRES, dets=dets, count=count)
        plan.set_labels(bi, cl, bx)
        graph = capture(dev, plan)
        # the chain: three Detect levels of random maps, the matching and the confusion matrix on the post-process's own rows
        post = DetPostPlan.create([(B, SIZE // s, SIZE // s) for s in (8, 16, 32)], nc, conf_thres=0.001, iou_thres=0.7, max_det=D, multi_label=nc > 1)
        g = torch.Generator().manual_seed(11)
        for f in post.feats:
            v = 0.5 * torch.randn(f.shape, generator=g)                                        # about 2000 candidates an image pass conf
            hot = torch.rand(v[:, 64:].shape, generator=g) < 2000 / (8400 * nc)
            v[:, 64:] = torch.where(hot, -4 + 6 * torch.rand(hot.shape, generator=g), torch.full(hot.shape, -10.0))
            f.copy_(v)
        chains = {}
        for k in ("chain2", "chain3"):
            match = DetMatchPlan.create(B, D, n_cap=bi.numel(), m_cap=m_cap, imgsz=SIZE, rows_cap=per_round * B * D, tgt_cap=per_round * B * L,
                                        dets=post.dets, count=post.count)
            match.set_labels(bi, cl, bx)
            third = (ConfusionPlan.create(B, D, nc=nc, m_cap=m_cap, imgsz=SIZE, conf=CONF, iou_thres=IOU_THRES, dets=post.dets, count=post.count,
                                          labels=match),) if k == "chain3" else ()
            chains[k] = (capture(dev, post, match, *third), match, third)

        def cm_eager():
            return confusion_matrix(dets, count, bi, cl, bx, nc=nc, imgsz=SIZE, conf=CONF, iou_thres=IOU_THRES)

        def loop():
            return torch_loop(dets, bi, cl, bx, nc)

        def host():
            return confusion_matrix(*host_in, nc=nc, imgsz=SIZE, conf=CONF, iou_thres=IOU_THRES)
        plan.reset()
        graph.replay()
        cm_e, det_e, lab_e = cm_eager()
        cm_h, det_h, lab_h = host()
        ref = loop()
        torch.cuda.synchronize(dev)
        plan.check_status()
        assert torch.equal(plan.cm.long(), cm_e) and torch.equal(plan.det_out, det_e) and torch.equal(plan.lab_out, lab_e)
        assert torch.equal(plan.matrix(), cm_e.cpu())
        assert torch.equal(cm_e.cpu(), cm_h) and torch.equal(det_e.cpu(), det_h) and torch.equal(lab_e.cpu(), lab_h)
        same = bool(np.array_equal(ref, cm_h.numpy()))

        def reset():
            plan.reset()
            for _, match, third in chains.values():
                match.reset()
                for t in third:
                    t.reset()
        sides = dict(cm_graph=(graph.replay, a.steps), cm_eager=(cm_eager, a.steps), torch_loop=(loop, a.slow_steps), host=(host, a.slow_steps),
                     chain2=(chains["chain2"][0].replay, a.steps), chain3=(chains["chain3"][0].replay, a.steps))
        for k, (fn, steps) in sides.items():
            reset()
            timed(fn, 1 if steps == a.slow_steps else a.warmup, dev)
        for _, match, third in chains.values():
            post.check_status(); match.check_status()
            for t in third:
                t.check_status()
        ms = {k: [] for k in sides}
        for _ in range(a.rounds):                                    # alternate the sides
            for k, (fn, steps) in sides.items():
                reset()
                ms[k].append(timed(fn, steps, dev))
        plan.check_status()
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        row = dict(config=cfg, B=B, max_det=D, nc=nc, labels_per_image=L, counts_in_the_matrix=int(cm_h.sum()), the_loop_s_matrix_is_the_same=same,
                   chain_mean_count=round(float(post.count.float().clamp(min=0).mean()), 1))
        for k in ms:
            row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(spread[k], 5), [round(v, 5) for v in ms[k]]
        row["cm_graph_vs_torch_loop"] = round(med["torch_loop"] / med["cm_graph"], 1)
        row["cm_graph_vs_host"] = round(med["host"] / med["cm_graph"], 1)
        row["chain3_minus_chain2_ms"] = round(med["chain3"] - med["chain2"], 5)
        rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
        del graph, plan, chains, post
        torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, slow_steps=a.slow_steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
