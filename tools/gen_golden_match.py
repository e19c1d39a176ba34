"""Write tests/golden/match_*.npz and tests/golden/match_ratios.json from the REFERENCE's own DetectionValidator.update_metrics (data only -- no
reference text is copied).

    python tools/gen_golden_match.py --reference <checkout of the reference project> [--only NAME ...]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of tools/gen_golden_nms.py.  `update_metrics` runs on a stand-in validator: a SimpleNamespace with `iouv`, `niou`, `args`, `device`,
`seen`, `metrics = DetMetrics()` and the reference's own `_prepare_batch`, `_prepare_pred`, `_process_batch` and `match_predictions` bound
to it -- the four methods the loop calls.  A case is one batch; the prediction list is the case's live detection rows per image, the labels
the rows before its n word.  With single_cls the labels' classes are zeroed for the reference, as its dataset would have them.

A seed is accepted only if
  - for every class-matched pair the fp64 IoU is farther than 1e-4 from every threshold;
  - except in the cases of match_cases.TWINS (`dup`, `dup_far`), a detection's two largest class-matched IoUs differ by more than 1e-4 (match_oracle.oracle's guards);
  - the case holds what it was built for (match_cases.built_for, ANSWERS);
  - the reference's answer equals the oracle's, under the rule and under the literal procedure (the cases with parity=False apart:
    construction only).
match_ratios.json: per case the largest |reference fp32 box_iou of a detection's best pair - fp64 oracle| / (eps_fp32 * term), the term from
the oracle -- the measurement behind the GPU tests' bar."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_nms import import_reference  # noqa: E402


def stand_in(torch, V, DetMetrics, iouv, single_cls):
    s = types.SimpleNamespace(iouv=torch.from_numpy(np.asarray(iouv, np.float32)), niou=len(iouv), device=torch.device("cpu"), seen=0,
                              metrics=DetMetrics(), confusion_matrix=None,
                              args=types.SimpleNamespace(single_cls=bool(single_cls), plots=False, visualize=False, save_json=False,
                                                         save_txt=False, save_conf=False, conf=0.001))
    for m in ("_prepare_batch", "_prepare_pred", "_process_batch", "match_predictions"):
        setattr(s, m, types.MethodType(getattr(V, m), s))
    return s


def reference_batch(torch, c):
    """The case as the validator's loop takes it: the prediction list and the batch dict"""
    B, D = c["dets"].shape[:2]
    dets = torch.from_numpy(c["dets"])
    preds = []
    for b in range(B):
        k = min(max(int(c["count"][b]), 0), D)
        preds.append(dict(bboxes=dets[b, :k, :4].clone(), conf=dets[b, :k, 4].clone(), cls=dets[b, :k, 5].clone(), extra=dets[b, :k, 6:].clone()))
    n = len(c["batch_idx"]) if c["n"] is None else c["n"]
    cls = torch.from_numpy(c["cls"][:n].copy())
    if c["single_cls"]:
        cls = cls * 0
    H, W = c["hw"]
    batch = dict(batch_idx=torch.from_numpy(c["batch_idx"][:n].copy()), cls=cls, bboxes=torch.from_numpy(c["bboxes"][:n].copy()),
                 img=torch.empty(B, 0, H, W), ori_shape=[(H, W)] * B, ratio_pad=[None] * B, im_file=[f"{b}.jpg" for b in range(B)])
    return preds, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", nargs="*", help="these cases only (the others' ratios are kept)")
    args = ap.parse_args()
    import_reference(args.reference)
    import torch
    from ultralytics.models.yolo.detect.val import DetectionValidator as V
    from ultralytics.utils.metrics import DetMetrics, box_iou
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import match_cases as MC
    import match_oracle as O
    path = os.path.join(OUT, "match_ratios.json")
    ratios = {}
    if args.only and os.path.exists(path):
        with open(path) as f:
            ratios = json.load(f)["cases"]
    for name, spec in MC.CASES.items():
        if args.only and name not in args.only:
            continue
        for seed in range(100, 140):
            c = MC.build(name, seed)
            o = MC.oracle(name, c)
            why = [g for g in o["guards"] if not (name in MC.TWINS and "two largest" in g)]
            why += MC.built_for(name, c, o)
            B, D = c["dets"].shape[:2]
            T = len(c["iouv"])
            if not why:
                preds, batch = reference_batch(torch, c)
                s = stand_in(torch, V, DetMetrics, c["iouv"], c["single_cls"])
                V.update_metrics(s, preds, batch)
                ref_tp = np.zeros((B, D, T), bool)
                ref_iou = np.zeros((B, D), np.float32)
                for b in range(B):
                    k = preds[b]["cls"].shape[0]
                    ref_tp[b, :k] = s.metrics.stats["tp"][b]
                    pb = s._prepare_batch(b, batch)
                    if k and len(pb["cls"]):
                        iou = box_iou(pb["bboxes"], preds[b]["bboxes"]) * (pb["cls"][:, None] == preds[b]["cls"])
                        ref_iou[b, :k] = iou.max(0).values.numpy()
                if s.seen != B:
                    why.append("the reference did not see every image")
                if name in MC.PARITY:
                    if not np.array_equal(ref_tp, o["tp"]):
                        why.append("the reference's tp is not the rule's")
                    if not np.array_equal(ref_tp, MC.oracle(name, c, use_procedure=True)["tp"]):
                        why.append("the reference's tp is not the literal procedure's")
            if not why and name in MC.ANSWERS:
                a = MC.ANSWERS[name]
                k = len(a["tp"])
                if o["tp"][0, :k].tolist() != a["tp"] or o["best_gt"][0, :k].tolist() != a["best_gt"]:
                    why.append(f"the answer by construction is {a}, the oracle gives {o['tp'][0, :k].tolist()} {o['best_gt'][0, :k].tolist()}")
                w = MC.BUILT_AGAINST.get(name)
                if w and np.array_equal(MC.oracle(name, c, wrong=w)["tp"], o["tp"]):
                    why.append(f"the wrong rule {w} gives the same answer")
            if not why:
                break
            print(f"{name}: seed {seed} rejected: {'; '.join(why)}")
            if spec.get("construct"):
                raise SystemExit(f"{name}: a case by construction does not depend on the seed")
        else:
            raise SystemExit(f"{name}: no seed passed the guards")
        r = O.ratio(ref_iou, o["best_iou"], o["term"])
        assert np.isfinite(r), f"{name}: the reference's IoU is not 0 where the oracle's is"
        rec = dict(seed=seed, ratio=r, hw=np.array(c["hw"]), single_cls=c["single_cls"], n=-1 if c["n"] is None else c["n"], m_cap=c["m_cap"],
                   **{k: c[k] for k in ("dets", "count", "batch_idx", "cls", "bboxes", "iouv")},
                   ref_tp=ref_tp, ref_best_iou_f32=ref_iou, stats_len=np.array([len(v) for v in s.metrics.stats["tp"]], np.int64))
        for key, lst in s.metrics.stats.items():                   # the lists update_metrics left, image after image
            for b, v in enumerate(lst):
                rec[f"stats_{key}_{b}"] = np.asarray(v)
        np.savez_compressed(MC.path(name), **rec)
        ratios[name] = r
        print(f"{name}: seed {seed}, {os.path.getsize(MC.path(name)) / 1024:.0f} KB, pairs {o['pairs']}, true {int(o['tp'].sum())}, ratio {r:.3f}")
    with open(path, "w") as f:
        json.dump(dict(cases=ratios, worst=max(ratios.values()), eps="float32"), f, indent=1, sort_keys=True)
    print("worst", max(ratios.values()))


if __name__ == "__main__":
    main()
