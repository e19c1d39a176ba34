"""Write tests/golden/ap_*.npz from the REFERENCE's own ap_per_class (data only -- no reference text is copied).

    python tools/gen_golden_ap.py --reference <checkout of the reference project> [--only NAME ...]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of tools/gen_golden_nms.py.  A record holds a case's four inputs (tests/ap_cases.py rebuilds them from the recorded seed) and the
twelve arrays the reference returns for them, ref0 .. ref11.

A case is written only if
  - no two rows of one class share a confidence (ap_cases.distinct_within_class), so that the reference's unstable argsort cannot matter
    -- the cases of ap_cases.TIES are answered by construction and get no record;
  - the reference's outputs equal the oracle's literal procedure's and its parallel rule's: everything exactly, ap within
    128 * 2^-53 * (the sum of its absolute trapezoid terms)."""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_nms import import_reference  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--only", nargs="*", help="these cases only")
    args = ap.parse_args()
    import_reference(args.reference)
    from ultralytics.utils.metrics import ap_per_class
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import ap_cases as AC
    import ap_oracle as AO
    from mga_yolo_amd.detap import _finish
    for name in AC.PARITY:
        if args.only and name not in args.only:
            continue
        c = AC.build(name)
        if not AC.distinct_within_class(c):
            raise SystemExit(f"{name}: two rows of one class share a confidence")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            ref = ap_per_class(c["tp"], c["conf"], c["pred_cls"], c["target_cls"])
        ref = tuple(np.asarray(r) for r in ref)
        lit, ap_abs = AO.procedure(c["tp"], c["conf"], c["pred_cls"], c["target_cls"])
        AO.assert_tuple(ref, lit, ap_abs, name + ": the reference against the literal procedure")
        dense = AO.rule(c["tp"], c["conf"], c["pred_cls"], c["target_cls"], c["nc"])
        AO.assert_tuple(ref, _finish(dense), AO.compact(dense)["ap_abs"], name + ": the reference against the rule")
        np.savez_compressed(AC.path(name), seed=AC.SEED, nc=c["nc"], **{k: c[k] for k in ("tp", "conf", "pred_cls", "target_cls")},
                            **{f"ref{i}": r for i, r in enumerate(ref)})
        print(f"{name}: {os.path.getsize(AC.path(name)) / 1024:.0f} KB, {c['tp'].shape[0]} rows, {len(ref[6])} classes with labels, "
              f"mAP50 {ref[5][:, 0].mean() if len(ref[6]) else float('nan'):.4f}")


if __name__ == "__main__":
    main()
