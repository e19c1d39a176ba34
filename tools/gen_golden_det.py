"""Write tests/golden/det_*.npz and tests/golden/det_ratios.json from the REFERENCE's own v8DetectionLoss (data only -- no reference
text is copied).

    python tools/gen_golden_det.py --reference <checkout of the reference project>
    python tools/gen_golden_det.py --reference <checkout> --shapes [--only NAME ...]     (tests/golden/detx_*.npz, det_ratios_shapes.json:
                                                                                          the rebuilt cases of tests/det_cases.py, see shapes_main)

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of DESIGN 8 (a stand-in ``cv2``, an answered ``torchvision`` version).  The criterion is built on a stand-in model: ``model[-1]``
with ``nc``, ``reg_max = 16``, ``stride = [8, 16, 32]``, and ``args`` with the three gains.

Features are "trained-like": plain random features decode to boxes some 7.5 cells wide around every anchor, every CIoU clamps to 0 and the
box and DFL terms vanish.  Inside a box the bin logits of a side peak near the true distance, -(j - t)^2 / tau + noise with t the true
distance moved by up to a cell, and the label's class logit is raised.  Per case the generator asserts box, dfl > 0.05 and that at least
30 % of the in-box anchors overlap their box, and it re-seeds the case until, in the fp64 run,
  - the k-th and (k+1)-th metric of every ground truth differ by > 1e-4 relative (unless both are exactly 0: the tie of include/mgadet.h);
  - the two largest overlaps of every anchor several ground truths claim differ by > 1e-4 relative;
  - no in-box delta lies within 1e-3 px of 0, other than those that are exactly 0 (the box whose edges lie on anchor centres).
Recorded, from an fp32 run and from an fp64 run: loss, items, target_scores, fg_mask, target_bboxes, dL/dfeats for the upstream vectors
(1, 1, 1) and UPSTREAM.  det_ratios.json: per quantity the largest |fp32 - fp64| / (eps_fp32 * sum |terms|) over all cases, the terms from
tests/det_oracle.py -- the measurement behind the tests' bar."""
import argparse
import importlib.metadata as md
import json
import os
import sys
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
STRIDES = (8, 16, 32)
GAINS = (7.5, 0.5, 1.5)
TOPK = 10
UPSTREAM = (0.7, -1.3, 2.1)

# name -> B, (H, W) of the image, nc, rows of (image, class, x1, y1, x2, y2 in pixels[, share of its anchors trained on a box far away]); a row of zeros
# is the all-zero label
CASES = {
    # two images, plain boxes
    "b2_64_nc1": (2, (64, 64), 1, [(0, 0, 6.3, 9.1, 41.7, 50.2), (0, 0, 30.5, 20.2, 60.9, 45.1), (1, 0, 10.4, 5.7, 52.6, 58.3)]),
    # the all-zero row; a box that holds no anchor centre; a box with fewer than topk anchors inside
    "b2_64_nc3": (2, (64, 64), 3, [(0, 2, 5.2, 7.3, 38.6, 44.9), (0, 0, 0, 0, 0, 0), (0, 1, 17.1, 17.2, 19.7, 19.5),
                                   (1, 0, 20.3, 18.6, 43.8, 33.1), (1, 2, 2.7, 40.2, 61.4, 62.9)]),
    # non-square; image 1 has no box; a box larger than the image; two heavily overlapping boxes
    "b3_96x64_nc5": (3, (64, 96), 5, [(0, 4, -20.5, -12.2, 120.7, 80.3), (0, 1, 30.2, 10.6, 70.9, 50.1),
                                      (2, 3, 12.4, 8.3, 60.8, 54.6), (2, 0, 15.9, 11.2, 64.1, 57.7), (2, 2, 66.3, 20.9, 90.2, 44.5)]),
    # more than topk anchors inside; edges exactly on P3 anchor centres (x1 = 12, x2 = 44); target distances beyond 14.99 cells
    "b2_128_nc2": (2, (128, 128), 2, [(0, 1, 12.0, 20.0, 44.0, 60.0), (0, 0, 2.3, 1.6, 126.4, 125.2), (1, 0, 40.6, 30.3, 100.2, 110.8),
                                      (1, 1, 8.9, 70.4, 50.3, 120.6)]),
    # ties of the metric at exactly 0: two small boxes over the same six anchors, about half of them predicting a box far away (CIoU <= 0
    # against both, picked by both for want of ten better ones, and handed to slot 0, a box elsewhere); a third box with eight anchors
    "ties": (2, (64, 64), 2, [(0, 0, 40.3, 36.2, 62.1, 60.7), (0, 1, 9.3, 9.2, 27.6, 27.8, 0.5), (0, 0, 10.9, 11.1, 26.2, 26.9, 0.5),
                              (1, 1, 33.2, 5.1, 52.8, 22.9, 0.5)]),
    # no label at all
    "empty": (2, (64, 64), 1, []),
}


def import_reference(ref_root):
    cv2 = MagicMock(name="cv2")                            # absent from the build image; nothing of it runs on this path
    cv2.__version__, cv2.__spec__ = "4.10.0", None
    sys.modules["cv2"] = cv2
    real = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else real(n)
    sys.path.insert(0, ref_root)
    import mga_yolo  # noqa: F401  (puts the vendored detector on the path)
    from ultralytics.utils.loss import v8DetectionLoss
    return v8DetectionLoss


def make_inputs(torch, B, hw, nc, rows, seed):
    """Labels in the batch's form and trained-like features (fp64; the fp32 run rounds them once)."""
    g = torch.Generator().manual_seed(seed)
    H, W = hw
    bidx = torch.tensor([r[0] for r in rows], dtype=torch.float64)
    cls = torch.tensor([r[1] for r in rows], dtype=torch.float64)
    xyxy = torch.tensor([r[2:6] for r in rows], dtype=torch.float64).reshape(-1, 4)
    xywh = torch.stack(((xyxy[:, 0] + xyxy[:, 2]) / 2 / W, (xyxy[:, 1] + xyxy[:, 3]) / 2 / H, (xyxy[:, 2] - xyxy[:, 0]) / W,
                        (xyxy[:, 3] - xyxy[:, 1]) / H), 1) if rows else torch.zeros(0, 4, dtype=torch.float64)
    feats = []
    for s in STRIDES:
        h, w = H // s, W // s
        f = 0.5 * torch.randn(B, 64 + nc, h, w, generator=g, dtype=torch.float64)
        f[:, 64:] -= 3.0
        for r in rows:
            b, c, x1, y1, x2, y2 = r[:6]
            skip = r[6] if len(r) > 6 else 0.0
            if x2 <= x1:
                continue
            for y in range(h):
                for x in range(w):
                    px, py = (x + 0.5) * s, (y + 0.5) * s
                    if not (x1 < px < x2 and y1 < py < y2):
                        continue
                    away = bool(skip) and float(torch.rand((), generator=g, dtype=torch.float64)) < skip
                    t = torch.tensor([px - x1, py - y1, x2 - px, y2 - py], dtype=torch.float64) / s
                    if away:                                         # a box that runs 14 cells down and right of the anchor: CIoU < 0
                        t = torch.tensor([0.0, 0.0, 14.0, 14.0], dtype=torch.float64)
                    t = (t + (torch.rand(4, generator=g, dtype=torch.float64) * 2 - 1)).clamp(0, 15)
                    j = torch.arange(16, dtype=torch.float64)
                    f[b, :64, y, x] = (-(j[None] - t[:, None]) ** 2 / 1.5 + 0.3 * torch.randn(4, 16, generator=g, dtype=torch.float64)).reshape(-1)
                    f[b, 64 + int(c), y, x] = 1.5 + torch.randn((), generator=g, dtype=torch.float64)
        feats.append(f)
    return feats, bidx, cls, xywh


def run_reference(torch, Crit, feats, bidx, cls, xywh, nc, dtype, strides=STRIDES, topk=TOPK):
    """One forward and two backwards of the reference's criterion in `dtype`; also what its assigner saw (for the guards)."""
    torch.set_default_dtype(dtype)
    try:
        class Stand(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.p = torch.nn.Parameter(torch.zeros(1))
                self.model = [SimpleNamespace(nc=nc, reg_max=16, stride=torch.tensor([float(s) for s in strides]))]
                self.args = SimpleNamespace(box=GAINS[0], cls=GAINS[1], dfl=GAINS[2])
        crit = Crit(Stand(), tal_topk=topk)
        seen = {}
        asg = crit.assigner
        inner_pos, inner_fwd = asg.get_pos_mask, asg.forward

        def spy_pos(*a, **k):
            out = inner_pos(*a, **k)
            seen["mask_pos"], seen["metric"], seen["overlaps"] = (t.clone() for t in out)
            seen["anc"], seen["gt"], seen["mask_gt"] = a[4].clone(), a[3].clone(), a[5].clone()
            return out

        def spy_fwd(*a, **k):
            out = inner_fwd(*a, **k)
            seen["target_bboxes"], seen["target_scores"], seen["fg_mask"], seen["target_gt_idx"] = (t.clone() for t in out[1:])
            return out
        asg.get_pos_mask, asg.forward = spy_pos, spy_fwd
        xs = [f.to(dtype).clone().requires_grad_(True) for f in feats]
        batch = dict(batch_idx=bidx.to(dtype), cls=cls.to(dtype), bboxes=xywh.to(dtype))
        loss, items = crit(xs, batch)
        grads = {}
        for name, up in (("g1", (1.0, 1.0, 1.0)), ("gnu", UPSTREAM)):
            gs = torch.autograd.grad((loss * torch.tensor(up, dtype=dtype)).sum(), xs, retain_graph=True, allow_unused=True)
            grads[name] = [torch.zeros_like(x) if g_ is None else g_ for g_, x in zip(gs, xs)]
        return loss.detach(), items.detach(), grads, seen
    finally:
        torch.set_default_dtype(torch.float32)


def guards(torch, seen, want_terms: bool, topk=TOPK):
    """The near-tie guard on the fp64 run; returns a reason to re-seed, or None."""
    if "metric" not in seen:
        return None
    met, ov, pos = seen["metric"], seen["overlaps"], seen["mask_pos"]
    anc, gt, mgt = seen["anc"], seen["gt"], seen["mask_gt"]
    deltas = torch.cat((anc[None, None] - gt[:, :, None, :2], gt[:, :, None, 2:] - anc[None, None]), -1).amin(-1)
    inbox = (deltas > 1e-9) & mgt.bool()
    near = (deltas.abs() < 1e-3) & (deltas != 0) & mgt.bool()
    if near.any():
        return "an in-box delta within 1e-3 px of 0"
    m = torch.where(inbox, met, -torch.ones_like(met)).sort(-1, descending=True).values
    if m.shape[-1] > topk:
        a, b = m[..., topk - 1], m[..., topk].clamp(min=0)
        if ((a > 0) & (m[..., topk] >= 0) & (a - b <= 1e-4 * a)).any():
            return "k-th and (k+1)-th metric within 1e-4"
    contested = pos.sum(1) > 1
    if contested.any() and ov.shape[1] > 1:
        top = ov.sort(1, descending=True).values
        if (contested & (top[:, 0] > 0) & (top[:, 0] - top[:, 1] <= 1e-4 * top[:, 0])).any():
            return "two largest overlaps of a contested anchor within 1e-4"
    if want_terms:
        frac = float((ov[inbox] > 0).double().mean()) if inbox.any() else 0.0
        if frac < 0.30:
            return f"only {frac:.2f} of the in-box anchors overlap"
    return None


def _ratio(a, b, t, eps):
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), np.shape(b))
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    ok = t > 0
    return float((d[ok] / (eps * t[ok])).max()) if ok.any() else 0.0


def shapes_main(torch, Crit, det_oracle, only=None):
    """--shapes: tests/golden/detx_<name>.npz for the cases of tests/det_cases.py and det_ratios_shapes.json.  The features are rebuilt
    on the test machine from the recorded seed, so a record holds no tensor of the features' size: the labels, the seed, the digest, the
    reference's loss and items (fp32 and fp64 runs), its fp64 target scores and foreground mask (sparse), and per quantity the ratio of
    its fp32 run against its fp64 run.  The gradients are compared here, against the oracle, and not stored: a seed is accepted only
    where the oracle equals the reference's fp64 run on them (and on everything else) at the bars of tests/test_det_abi.py."""
    import det_cases as DC
    eps32 = float(np.finfo(np.float32).eps)
    ratios = {}
    path = os.path.join(OUT, "det_ratios_shapes.json")
    if only and os.path.exists(path):
        with open(path) as f:
            ratios = json.load(f)["cases"]
    for name, spec in DC.CASES.items():
        if only and name not in only:
            continue
        B, nc, strides, topk = spec["B"], spec["nc"], tuple(spec["strides"]), spec["topk"]
        bidx, cls, xywh = (t.double() for t in DC.labels(name))
        kw = dict(nc=nc, strides=strides, gains=GAINS, topk=topk)
        want_terms = name != "chunk_zero"
        for seed in range(100, 140):
            feats = [f.double() for f in DC.build_feats(name, seed)]
            why = None
            for tag, fs in (("fp32", feats), ("fp16", [f.half().double() for f in feats]), ("bf16", [f.bfloat16().double() for f in feats])):
                l64, i64, g64, seen = run_reference(torch, Crit, fs, bidx, cls, xywh, nc, torch.float64, strides, topk)
                why = guards(torch, seen, want_terms, topk)
                if why is not None:
                    why = f"{tag} values: {why}"
                    break
            if why is None:
                l64, i64, g64, seen = run_reference(torch, Crit, feats, bidx, cls, xywh, nc, torch.float64, strides, topk)
                raw = l64 / torch.tensor(GAINS, dtype=torch.float64) / B
                if want_terms and not (raw[0] > 0.05 and raw[2] > 0.05):
                    why = f"box {float(raw[0]):.3f} / dfl {float(raw[2]):.3f} not above 0.05"
                if not want_terms and not (raw[1] > 0 and float(seen["target_scores"].sum()) > 0):
                    why = "cls or every weight is 0"
            if why is None:
                lo = det_oracle.oracle(feats, bidx, cls, xywh, **kw)
                hi = det_oracle.oracle(feats, bidx, cls, xywh, lowest_first=False, **kw)
                same = torch.equal(lo["loss"], hi["loss"]) and torch.equal(lo["target_scores"], hi["target_scores"]) and all(
                    torch.equal(a, b) for i in range(3) for a, b in zip(lo["comp_grads"][i], hi["comp_grads"][i]))
                if not same:
                    why = "the two tie orders differ"
            if why is None:
                why = "; ".join(DC.built_for(name, lo)) or None
            if why is None:                                      # the oracle against the reference's fp64 run, as test_oracle_equals_the_reference_fp64_run
                K, t = det_oracle.K, lo["terms"]
                try:
                    det_oracle.check("loss", lo["loss"], l64, t["loss"], 1e-9 / K["loss"], K["loss"])
                    det_oracle.check("items", lo["items"], i64, t["loss"] / B, 1e-9 / K["loss"], K["loss"])
                    det_oracle.check("target_scores", lo["target_scores"], seen["target_scores"], t["target_scores"], 1e-9 / K["target_scores"],
                                     K["target_scores"])
                    for key, up in (("g1", (1.0, 1.0, 1.0)), ("gnu", UPSTREAM)):
                        for l in range(len(feats)):
                            det_oracle.check(f"{key}[{l}]", det_oracle.grads(lo, l, up), g64[key][l], det_oracle.grad_terms(t, l, up), 1e-9 / K["grad"],
                                             K["grad"])
                except AssertionError as e:
                    why = f"the oracle is not the reference: {e}"
            if why is None:
                break
            print(f"{name}: seed {seed} rejected: {why}")
        else:
            raise SystemExit(f"{name}: no seed passed the guards")
        l32, i32, g32, seen32 = run_reference(torch, Crit, feats, bidx, cls, xywh, nc, torch.float32, strides, topk)
        t = lo["terms"]
        r = dict(loss=_ratio(l32.numpy(), l64.numpy(), t["loss"].numpy(), eps32),
                 target_scores=_ratio(seen32["target_scores"].numpy(), seen["target_scores"].numpy(), t["target_scores"].numpy(), eps32))
        for key, up in (("g1", (1.0, 1.0, 1.0)), ("gnu", UPSTREAM)):
            r[key] = max(_ratio(g32[key][l].numpy(), g64[key][l].numpy(), det_oracle.grad_terms(t, l, up).numpy(), eps32) for l in range(len(feats)))
        ts = seen["target_scores"].numpy().reshape(-1)
        rec = dict(strides=np.array(strides), gains=np.array(GAINS), topk=topk, seed=seed, options=json.dumps(DC.options(name)),
                   sha256=DC.digest(DC.build_feats(name, seed)), batch_idx=bidx.numpy().astype(np.float32), cls=cls.numpy().astype(np.float32),
                   bboxes=xywh.numpy().astype(np.float32), loss_f32=l32.numpy(), items_f32=i32.numpy(), loss_f64=l64.numpy(), items_f64=i64.numpy(),
                   ts_index=np.flatnonzero(ts).astype(np.int64), ts_value=ts[np.flatnonzero(ts)],
                   fg_index=np.flatnonzero(seen["fg_mask"].numpy().reshape(-1)).astype(np.int64),
                   ratio_names=np.array(sorted(r)), ratio_values=np.array([r[k] for k in sorted(r)]))
        np.savez_compressed(DC.path(name), **rec)
        ratios[name] = r
        print(f"{name}: seed {seed}, {os.path.getsize(DC.path(name)) / 1024:.0f} KB, loss {l64.tolist()}, ratios {r}")
    worst = {k: max(r[k] for r in ratios.values()) for k in ("loss", "target_scores", "g1", "gnu")}
    with open(path, "w") as f:
        json.dump(dict(cases=ratios, worst=worst, eps="float32"), f, indent=1, sort_keys=True)
    print("worst", worst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--shapes", action="store_true", help="write the detx_* records of tests/det_cases.py instead of the six stored cases")
    ap.add_argument("--only", nargs="*", help="with --shapes: these cases only (the others' ratios are kept)")
    args = ap.parse_args()
    Crit = import_reference(args.reference)
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import det_oracle
    if args.shapes:
        return shapes_main(torch, Crit, det_oracle, args.only)
    ratios = {}
    for name, (B, hw, nc, rows) in CASES.items():
        for seed in range(100, 140):
            feats, bidx, cls, xywh = make_inputs(torch, B, hw, nc, rows, seed)
            feats = [f.float().double() for f in feats]                 # both runs start from the same fp32-representable values
            xywh, = [xywh.float().double()]
            l64, i64, g64, seen = run_reference(torch, Crit, feats, bidx, cls, xywh, nc, torch.float64)
            why = guards(torch, seen, bool(rows))
            if why is None and rows:
                raw = l64 / torch.tensor(GAINS, dtype=torch.float64) / B
                if not (raw[0] > 0.05 and raw[2] > 0.05):
                    why = f"box {float(raw[0]):.3f} / dfl {float(raw[2]):.3f} not above 0.05"
            if why is None:
                break
            print(f"{name}: seed {seed} rejected: {why}")
        else:
            raise SystemExit(f"{name}: no seed passed the guards")
        l32, i32, g32, seen32 = run_reference(torch, Crit, feats, bidx, cls, xywh, nc, torch.float32)
        A = sum((hw[0] // s) * (hw[1] // s) for s in STRIDES)
        rec = dict(B=B, nc=nc, strides=np.array(STRIDES), gains=np.array(GAINS), topk=TOPK, upstream=np.array(UPSTREAM),
                   batch_idx=bidx.numpy().astype(np.float32), cls=cls.numpy().astype(np.float32), bboxes=xywh.numpy().astype(np.float32))
        for l, f in enumerate(feats):
            rec[f"feat{l}"] = f.numpy().astype(np.float32)
        for tag, (lo, it, gr, sn) in (("f32", (l32, i32, g32, seen32)), ("f64", (l64, i64, g64, seen))):
            rec[f"loss_{tag}"], rec[f"items_{tag}"] = lo.numpy(), it.numpy()
            rec[f"target_scores_{tag}"] = sn["target_scores"].numpy() if "target_scores" in sn else np.zeros((B, A, nc))
            rec[f"fg_mask_{tag}"] = sn["fg_mask"].numpy().astype(bool) if "fg_mask" in sn else np.zeros((B, A), bool)
            rec[f"target_bboxes_{tag}"] = sn["target_bboxes"].numpy() if "target_bboxes" in sn else np.zeros((B, A, 4))
            for key, gs in gr.items():
                for l, g_ in enumerate(gs):
                    rec[f"{key}_{l}_{tag}"] = g_.numpy()
        path = os.path.join(OUT, f"det_{name}.npz")
        np.savez_compressed(path, **rec)
        # fp32 run against fp64 run, in units of eps * sum |terms|
        terms = det_oracle.oracle([f.double() for f in feats], bidx, cls, xywh, nc=nc, strides=STRIDES, gains=GAINS, topk=TOPK)["terms"]
        eps = float(np.finfo(np.float32).eps)
        def ratio(a, b, t):
            t = np.broadcast_to(np.asarray(t, dtype=np.float64), np.shape(b))
            d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
            ok = t > 0
            return float((d[ok] / (eps * t[ok])).max()) if ok.any() else 0.0
        r = dict(loss=ratio(rec["loss_f32"], rec["loss_f64"], terms["loss"].numpy()),
                 target_scores=ratio(rec["target_scores_f32"], rec["target_scores_f64"], terms["target_scores"].numpy()))
        for key, up in (("g1", (1.0, 1.0, 1.0)), ("gnu", UPSTREAM)):
            r[key] = max(ratio(rec[f"{key}_{l}_f32"], rec[f"{key}_{l}_f64"], det_oracle.grad_terms(terms, l, up).numpy()) for l in range(len(feats)))
        ratios[name] = r
        print(f"{name}: seed {seed}, {os.path.getsize(path) / 1024:.0f} KB, loss {l64.tolist()}, ratios {r}")
    worst = {k: max(r[k] for r in ratios.values()) for k in ("loss", "target_scores", "g1", "gnu")}
    with open(os.path.join(OUT, "det_ratios.json"), "w") as f:
        json.dump(dict(cases=ratios, worst=worst, eps="float32"), f, indent=1, sort_keys=True)
    print("worst", worst)


if __name__ == "__main__":
    main()
