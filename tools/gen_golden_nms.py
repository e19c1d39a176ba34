"""Write tests/golden/nms_*.npz and tests/golden/nms_ratios.json from the REFERENCE's own Detect._inference and non_max_suppression (data
only -- no reference text is copied).

    python tools/gen_golden_nms.py --reference <checkout of the reference project> [--only NAME ...]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of DESIGN 8 (a stand-in ``cv2``, an answered ``torchvision`` version).  The decode runs on a stand-in head: a ``Detect(nc, ch)`` whose
``stride`` is set and whose convolutions are never called -- ``_inference`` only reads ``no``, ``nc``, ``reg_max``, ``stride`` and ``dfl``.

torchvision is absent from the build image, and ``non_max_suppression`` imports it for ``torchvision.ops.nms`` alone.  The generator supplies
that one function itself: ``_nms`` below, a plain greedy NMS with a STABLE sort, written here.  The reference therefore pins everything
AROUND the greedy core -- decode, candidates, class separation by offset, max_nms, max_det, order -- and the core itself is pinned by
tests/nms_oracle.py and by the cases whose answer is known by construction (tests/nms_cases.ANSWERS).

A seed is accepted only if
  - the reference's fp32 run, its fp64 run and the oracle give the same kept anchors and classes in the same order, under both of the
    oracle's tie orders (the `ties` case apart, where the other order must differ).  A case with parity=False (nms_cases.CASES: the cut of
    max_nms falls inside a group of equal scores, which the reference orders with an unstable argsort) is held to its construction and the
    oracle instead: the reference decodes it, nothing of its lists is compared or stored, and it has no entry in nms_ratios.json;
  - no candidate probability lies within 1e-5 relative of conf_thres, no compared pair's IoU within 1e-4 of iou_thres, with the class
    offset and without it (nms_oracle.guards), on the fp32 features and on their fp16- and bf16-rounded values;
  - the case holds what it was built for (nms_cases.built_for, ANSWERS).
nms_ratios.json: per case the largest |fp32 run - fp64 run| / (eps_fp32 * terms) over the kept rows' coordinates and scores, the terms from
the oracle -- the measurement behind the tests' bar."""
import argparse
import importlib.metadata as md
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")


def _nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms's contract: the indices kept, by descending score; equal scores in index order (a stable sort)."""
    import torch
    order = scores.sort(descending=True, stable=True).indices
    b = boxes[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    alive = torch.ones(b.shape[0], dtype=torch.bool)
    keep = []
    for i in range(b.shape[0]):
        if not alive[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        inter = (torch.minimum(b[i, 2], r[:, 2]) - torch.maximum(b[i, 0], r[:, 0])).clamp(min=0) * \
                (torch.minimum(b[i, 3], r[:, 3]) - torch.maximum(b[i, 1], r[:, 1])).clamp(min=0)
        alive[i + 1:] &= ~(inter / (area[i] + area[i + 1:] - inter) > iou_threshold)
    return order[torch.tensor(keep, dtype=torch.long)]


def import_reference(ref_root):
    cv2 = MagicMock(name="cv2")                            # absent from the build image; nothing of it runs on this path
    cv2.__version__, cv2.__spec__ = "4.10.0", None
    sys.modules["cv2"] = cv2
    tv = types.ModuleType("torchvision")                   # what non_max_suppression imports: torchvision.ops.nms
    tv.__version__, tv.ops = "0.25.0", types.ModuleType("torchvision.ops")
    tv.ops.nms = _nms
    sys.modules["torchvision"], sys.modules["torchvision.ops"] = tv, tv.ops
    real = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else real(n)
    sys.path.insert(0, ref_root)
    import mga_yolo  # noqa: F401  (puts the vendored detector on the path)
    from ultralytics.nn.modules.head import Detect
    from ultralytics.utils.ops import non_max_suppression
    return Detect, non_max_suppression


def run_reference(torch, Detect, ref_nms, feats, k, dtype):
    """The reference's decode and post-process in `dtype`: per image the (n, 6) rows and the kept anchor indices."""
    head = Detect(nc=k["nc"], ch=(16,) * len(feats)).to(dtype).eval()
    head.stride = torch.tensor([float(s) for s in k["strides"]], dtype=dtype)
    with torch.no_grad():
        pred = head._inference([f.to(dtype).clone() for f in feats])
        out, idx = ref_nms(pred.clone(), conf_thres=k["conf_thres"], iou_thres=k["iou_thres"], agnostic=k["agnostic"],
                           multi_label=k["multi_label"], max_det=k["max_det"], max_nms=k["max_nms"], return_idxs=True)
    return pred, [o.double().numpy().reshape(-1, 6) for o in out], [i.numpy().reshape(-1).astype(np.int64) for i in idx]


def same_set(o, rows, idx):
    for b in range(len(rows)):
        n = int(o["count"][b])
        if n != rows[b].shape[0] or not np.array_equal(o["keep"][b, :n], idx[b]) or not np.array_equal(o["dets"][b, :n, 5], rows[b][:, 5]):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", nargs="*", help="these cases only (the others' ratios are kept)")
    args = ap.parse_args()
    Detect, ref_nms = import_reference(args.reference)
    import torch
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import nms_cases as NC
    import nms_oracle as O
    path = os.path.join(OUT, "nms_ratios.json")
    ratios = {}
    if args.only and os.path.exists(path):
        with open(path) as f:
            ratios = json.load(f)["cases"]
    for name, spec in NC.CASES.items():
        if args.only and name not in args.only:
            continue
        k = NC.kw(name)
        parity = name in NC.PARITY
        for seed in range(100, 140):
            feats = NC.build_feats(name, seed)
            np_feats = [f.numpy() for f in feats]
            why = []
            for tag, fs in (("fp32", np_feats), ("fp16", [f.half().float().numpy() for f in feats]), ("bf16", [f.bfloat16().float().numpy() for f in feats])):
                why += [f"{tag} values: {w}" for w in O.guards(O.oracle(feats=fs, **k))]
            lo, hi = O.oracle(feats=np_feats, **k), O.oracle(feats=np_feats, lowest_first=False, **k)
            if not why:
                pred32, r32, i32 = run_reference(torch, Detect, ref_nms, feats, k, torch.float32)
                pred64, r64, i64 = run_reference(torch, Detect, ref_nms, feats, k, torch.float64)
                if parity and not (same_set(lo, r32, i32) and same_set(lo, r64, i64)):
                    why.append("the reference's runs and the oracle keep different rows")
                if parity and (name == "ties") == same_set(hi, r64, i64):
                    why.append("the other tie order: " + ("the same rows" if name == "ties" else "different rows"))
                if not torch.allclose(NC.ref_decode(feats, k["strides"], k["nc"]), pred32, rtol=1e-5, atol=1e-4):
                    why.append("nms_cases.ref_decode is not the reference's decode")      # (the same ops but for the DFL's sum, a conv there)
                why += O.guards(O.oracle(pred=pred32.numpy(), **k))
            if not why:
                why = NC.built_for(name, feats)
            if not why and name in NC.ANSWERS:
                ka, kc = NC.ANSWERS[name]
                if parity and ([a.tolist() for a in i64] != ka or [r[:, 5].astype(int).tolist() for r in r64] != kc):
                    why.append(f"the answer by construction is {ka}, the reference kept {[a.tolist() for a in i64]}")
                got = [lo["keep"][b, :lo["count"][b]].tolist() for b in range(spec["B"])]
                if got != ka or [lo["dets"][b, :lo["count"][b], 5].astype(int).tolist() for b in range(spec["B"])] != kc:
                    why.append(f"the answer by construction is {ka}, the oracle kept {got}")
            if not why:
                break
            print(f"{name}: seed {seed} rejected: {'; '.join(why)}")
            if "puts" in spec:
                raise SystemExit(f"{name}: a case by construction does not depend on the seed")
        else:
            raise SystemExit(f"{name}: no seed passed the guards")
        rec = dict(k, strides=np.array(k["strides"]), seed=seed)
        if NC.elements(name) <= NC.STORE_WHOLE:
            for l, f in enumerate(np_feats):
                rec[f"feat{l}"] = f
        else:
            rec["sha256"] = NC.digest(feats)
        if not parity:
            np.savez_compressed(NC.path(name), **rec)
            ratios.pop(name, None)
            print(f"{name}: no parity, {os.path.getsize(NC.path(name)) / 1024:.0f} KB, counts {lo['count'].tolist()}, candidates {lo['n_cand']}")
            continue
        B = spec["B"]
        r = 0.0
        for b in range(B):
            n = r64[b].shape[0]
            if n:
                r = max(r, O.ratio(r32[b][:, :5], r64[b][:, :5], lo["terms"][b, :n, :5]))
        # the oracle against the reference's fp64 run: the same scores but for the order of a few fp64 roundings; the coordinates within half
        # an fp32 eps, because the reference's xywh2xyxy writes fp32 whatever it is given (ops.empty_like)
        for b in range(B):
            n = r64[b].shape[0]
            if n:
                assert O.ratio(lo["dets"][b, :n, 4], r64[b][:, 4], lo["terms"][b, :n, 4]) < 1e-6, f"{name}: the oracle is not the reference"
                assert O.ratio(lo["dets"][b, :n, :4], r64[b][:, :4], lo["terms"][b, :n, :4]) <= 0.5, f"{name}: the oracle is not the reference"
        rec.update(ratio=r, ref_count=np.array([x.shape[0] for x in r64], dtype=np.int64),
                   ref_dets_f32=np.concatenate(r32).astype(np.float32), ref_dets_f64=np.concatenate(r64), ref_keep_all=np.concatenate(i64))
        np.savez_compressed(NC.path(name), **rec)
        ratios[name] = r
        print(f"{name}: seed {seed}, {os.path.getsize(NC.path(name)) / 1024:.0f} KB, counts {rec['ref_count'].tolist()}, candidates {lo['n_cand']}, ratio {r:.3f}")
    with open(path, "w") as f:
        json.dump(dict(cases=ratios, worst=max(ratios.values()), eps="float32"), f, indent=1, sort_keys=True)
    print("worst", max(ratios.values()))


if __name__ == "__main__":
    main()
