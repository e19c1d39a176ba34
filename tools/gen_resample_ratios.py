#!/usr/bin/env python3
"""Writes tests/golden/resample_ratios.json: the worst ratio |torch's fp32 host result - oracle| / terms of F.interpolate(mode="bilinear",
align_corners=False) and of its autograd over the cases of tests/resample_oracle.py (the named cases and the sweep of every size pair
in 1..40 on either axis), forward and backward separately.  The device tests hold the resample kernels to K = 2 x these figures
(DESIGN 7f-1).  Pure torch on the CPU; data only.

    python tools/gen_resample_ratios.py [--check]      # --check: recompute and compare with the stored file, write nothing"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resample_oracle as RO  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    named, sweep = RO.torch_ratios(RO.NAMED), RO.torch_ratios(RO.sweep_cases())
    assert named["nonzero_at_zero_terms"] == 0 and sweep["nonzero_at_zero_terms"] == 0, "torch is not 0 at a zero-terms element"
    groups = dict(named["groups"], **sweep["groups"])
    rec = dict(forward=max(named["forward"], sweep["forward"]), backward=max(named["backward"], sweep["backward"]),
               eps32=RO.EPS32, cases=len(RO.NAMED) + len(RO.sweep_cases()),
               groups={k: dict(forward=v[0], backward=v[1]) for k, v in groups.items()},
               zero_terms=dict(named=[named["zero_terms"], named["elements"]], sweep=[sweep["zero_terms"], sweep["elements"]]),
               torch=torch.__version__.split("+")[0])
    print(json.dumps(rec, indent=1))
    if args.check:
        with open(RO.RATIOS) as f:
            old = json.load(f)
        ok = all(rec[k] <= 2.0 * old[k] for k in ("forward", "backward"))
        print("stored:", old["forward"], old["backward"], "-> within K" if ok else "-> OUTSIDE K")
        return 0 if ok else 1
    with open(RO.RATIOS, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
