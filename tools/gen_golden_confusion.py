"""Write tests/golden/confusion_*.npz from the REFERENCE's own ConfusionMatrix.process_batch (data only -- no reference text is copied).

    python tools/gen_golden_confusion.py --reference <checkout of the reference project> [--only NAME ...]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of tools/gen_golden_nms.py; the batch and the stand-in validator whose `_prepare_batch` / `_prepare_pred` form what process_batch
takes are those of tools/gen_golden_match.py.  A case is one batch.  Every image gets a FRESH ConfusionMatrix, so the record holds the
per-image matrices (B, nc + 1, nc + 1): that pins more than their sum does.  The validator's `conf` argument is passed as the case states
it (0.001 where the case means the default), so the reference's own substitution runs.

A seed is accepted only if
  - every fp64 IoU is farther than 1e-4 from iou_thres, a detection's two largest qualifying IoUs differ by more than 1e-4 and so do a
    label's two largest claimants' (confusion_oracle.oracle's guards; the cases by construction, whose IoUs are exact in fp32, apart from
    the first, and confusion_cases.TWINS apart from the other two);
  - the case holds what it was built for (confusion_cases.built_for, ANSWERS, BUILT_AGAINST);
  - the reference's per-image matrices equal the oracle's, under the rule and under the literal procedure (the cases with parity=False
    apart: construction only)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_match import reference_batch, stand_in  # noqa: E402
from gen_golden_nms import import_reference  # noqa: E402


def reference_matrices(torch, V, DetMetrics, ConfusionMatrix, c):
    """the reference's matrix of every image of the case, each from a ConfusionMatrix of its own"""
    B, nc = len(c["count"]), c["nc"]
    preds, batch = reference_batch(torch, c)
    s = stand_in(torch, V, DetMetrics, np.linspace(0.5, 0.95, 10), c["single_cls"])
    out = np.zeros((B, nc + 1, nc + 1), np.int64)
    for b in range(B):
        pbatch, predn = s._prepare_batch(b, batch), s._prepare_pred(preds[b])
        m = ConfusionMatrix(names={i: str(i) for i in range(nc)})
        m.process_batch(predn, pbatch, conf=c["conf"], iou_thres=c["iou_thres"])
        assert np.array_equal(m.matrix, np.round(m.matrix)) and m.matrix.shape == (nc + 1, nc + 1)
        out[b] = m.matrix.astype(np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", nargs="*", help="these cases only")
    args = ap.parse_args()
    import_reference(args.reference)
    import torch
    from ultralytics.models.yolo.detect.val import DetectionValidator as V
    from ultralytics.utils.metrics import ConfusionMatrix, DetMetrics
    torch.set_num_threads(1)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import confusion_cases as CC
    for name, spec in CC.CASES.items():
        if args.only and name not in args.only:
            continue
        for seed in range(100, 140):
            c = CC.build(name, seed)
            o = CC.oracle(name, c)
            why = [g for g in o["guards"] if not (name in CC.TWINS and "two largest" in g)]
            why += CC.built_for(name, c, o)
            ref = None
            if not why:
                ref = reference_matrices(torch, V, DetMetrics, ConfusionMatrix, c)
                if name in CC.PARITY:
                    if not np.array_equal(ref, o["per_image"]):
                        why.append("the reference's matrices are not the rule's")
                    if not np.array_equal(ref, CC.oracle(name, c, use_procedure=True)["per_image"]):
                        why.append("the reference's matrices are not the literal procedure's")
            if not why and name in CC.ANSWERS:
                a = CC.ANSWERS[name]
                rows = np.nonzero(c["batch_idx"] == 0)[0]
                if not np.array_equal(o["cm"], CC.answer_matrix(name)) or o["det_out"][0].tolist() != a["det_out"] \
                        or o["lab_out"][rows].tolist() != a["lab_out"]:
                    why.append(f"the answer by construction is {a}, the oracle gives {o['cm'].tolist()} {o['det_out'][0].tolist()} {o['lab_out'][rows].tolist()}")
                w = CC.BUILT_AGAINST.get(name)
                if w and np.array_equal(CC.oracle(name, c, wrong=w)["cm"], o["cm"]):
                    why.append(f"the wrong rule {w} gives the same answer")
            if not why:
                break
            print(f"{name}: seed {seed} rejected: {'; '.join(why)}")
            if spec.get("construct"):
                raise SystemExit(f"{name}: a case by construction does not depend on the seed")
        else:
            raise SystemExit(f"{name}: no seed passed the guards")
        np.savez_compressed(CC.path(name), seed=seed, hw=np.array(c["hw"]), nc=c["nc"], conf=c["conf"], iou_thres=c["iou_thres"],
                            single_cls=c["single_cls"], n=-1 if c["n"] is None else c["n"], m_cap=c["m_cap"],
                            **{k: c[k] for k in ("dets", "count", "batch_idx", "cls", "bboxes")}, ref_per_image=ref)
        print(f"{name}: seed {seed}, {os.path.getsize(CC.path(name)) / 1024:.0f} KB, counts {int(o['cm'].sum())}, off the diagonal {o['offdiag']}, "
              f"most claimants of a label {o['claims']}")


if __name__ == "__main__":
    main()
