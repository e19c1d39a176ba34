"""Forward + backward of the three MGAMaskHead levels through mask_head_pyramid on channels_last features, in four forms (prints one
JSON line):

  A         channels_last x through the channels-last GEMM kernels (MGAHEAD_LAYOUT_NHWC); gx comes back channels_last
  B_module  the same data the way the NCHW-only head took it: x.contiguous() in, the NCHW kernels -- the module's own cost with the copy in
  B_cl      B_module plus gx converted back to channels_last (what autograd's add into a channels_last neighbour's gradient costs)
  C         NCHW inputs through the NCHW kernels (reference point)

Usage: python tools/bench_head_layout.py [--workloads cfg2,cfg3,cfg4] [--dtypes f32,f16,bf16] [--rounds 12] [--iters 10]
Timing: device events around `iters` steps, forms alternated round by round after a warm-up; median and spread (min, max) per form, in ms
per step.  The workloads are bench.WORKLOADS (P3/P4/P5 shapes and batch), hidden = C / 4 as bench.py's slice uses; training mode."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mga_yolo_amd import MGAMaskHead  # noqa: E402
from mga_yolo_amd import functional as F  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CL = torch.channels_last


def setup(workload, dtype):
    _, B, shapes = bench.WORKLOADS[workload]
    g = torch.Generator(device="cuda").manual_seed(7)
    lv = []
    for i, (C, H, W) in enumerate(shapes):
        torch.manual_seed(i)
        m = MGAMaskHead(C, max(C // 4, 1)).cuda().train()
        x = torch.randn(B, C, H, W, device="cuda", generator=g).to(dtype)
        gl = torch.randn(B, 1, H, W, device="cuda", generator=g).to(dtype)
        lv.append(dict(m=m, x_cl=x.to(memory_format=CL), x=x, gl=gl))
    return lv


def step(lv, form):
    levels, gls = [], []
    for d in lv:
        m = d["m"]
        bn = m.proj[1]
        x = d["x_cl"] if form == "A" else (d["x"] if form == "C" else d["x_cl"].contiguous())   # B: the parent's _ready copy
        levels.append((x.detach().requires_grad_(True), m.proj[0].weight, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                       bn.num_batches_tracked, m.head.weight, m.head.bias, bn.eps, bn.momentum, True))
        gls.append(d["gl"])
    ys = F.mask_head_pyramid(levels)
    gx = torch.autograd.grad(ys, [l[0] for l in levels], gls)
    if form == "B_cl":                                                   # the channels_last neighbour's gradient layout
        gx = [g.contiguous(memory_format=CL) for g in gx]
    return ys, gx


def time_form(lv, form, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        step(lv, form)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="cfg2,cfg3,cfg4")
    ap.add_argument("--dtypes", default="f32,f16,bf16")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forms", default="A,B_module,B_cl,C")
    args = ap.parse_args()
    forms = args.forms.split(",")
    out = {}
    for wl in args.workloads.split(","):
        for dn in args.dtypes.split(","):
            lv = setup(wl, DT[dn])
            for f in forms:
                for _ in range(args.warmup):
                    step(lv, f)
            torch.cuda.synchronize()
            t = {f: [] for f in forms}
            for r in range(args.rounds):
                order = forms if r % 2 == 0 else forms[::-1]
                for f in order:
                    t[f].append(time_form(lv, f, args.iters))
            res = {f: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for f, v in t.items()}
            if "A" in res and "B_cl" in res:
                res["A_faster_than_B_cl"] = res["A"]["max"] < res["B_cl"]["min"]
            if "A" in res and "C" in res:
                res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
            out[f"{wl}.{dn}"] = res
            del lv
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="bench_head_layout", ms_per_step=out, rounds=args.rounds, iters=args.iters)))


if __name__ == "__main__":
    main()
