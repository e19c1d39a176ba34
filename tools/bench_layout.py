"""Forward + backward of MaskCBAM through mask_cbam_pyramid on channels_last features, in three forms (prints one JSON line):

  A         channels_last x / gy through the channels-last kernels (MGACBAM_LAYOUT_NHWC); y and gx come back channels_last
  B_module  the same data the way the NCHW-only library took it: x.contiguous() in, gy contiguous, the NCHW kernels -- the module's own
            cost without the conversions
  B_cl      B_module plus the conversions a channels_last neighbour adds: x and gy to NCHW, y and gx back to channels_last
  C         NCHW inputs through the NCHW kernels (reference point)

Usage: python tools/bench_layout.py [--workloads cfg2,cfg3,cfg4] [--dtypes f32,f16,bf16] [--rounds 12] [--iters 10]
Timing: device events around `iters` steps, forms alternated round by round after a warm-up; median and spread (min, max) per form, in ms
per step.  The workloads are bench.WORKLOADS (P3/P4/P5 shapes and batch)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mga_yolo_amd import functional as F  # noqa: E402
from oracle import maskcbam_oracle as O  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CL = torch.channels_last


def setup(workload, dtype):
    _, B, shapes = bench.WORKLOADS[workload]
    g = torch.Generator(device="cuda").manual_seed(7)
    lv = []
    for C, H, W in shapes:
        x = torch.randn(B, C, H, W, device="cuda", generator=g).to(dtype)
        m = torch.randn(B, 1, H, W, device="cuda", generator=g)
        gy = torch.randn(B, C, H, W, device="cuda", generator=g).to(dtype)
        p = O.Params.default_init(C)
        ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
        lv.append(dict(x_cl=x.to(memory_format=CL), x=x, m=m.requires_grad_(True), gy_cl=gy.to(memory_format=CL), gy=gy, ps=ps,
                       cfg=F.BlockConfig(hidden=p.w1.shape[0])))
    return lv


def step(lv, form):
    levels, gys = [], []
    for d in lv:
        if form == "A":
            x, gy = d["x_cl"], d["gy_cl"]
        elif form == "C":
            x, gy = d["x"], d["gy"]
        else:
            x, gy = d["x_cl"].contiguous(), d["gy_cl"].contiguous()      # the parent's _ready / _aligned copies
        levels.append((x.detach().requires_grad_(True), d["m"], d["ps"], d["cfg"]))
        gys.append(gy)
    ys = F.mask_cbam_pyramid(levels)
    gx = torch.autograd.grad(ys, [l[0] for l in levels], gys)
    if form == "B_cl":                                                   # the channels_last neighbours convert y and gx back
        ys = [y.contiguous(memory_format=CL) for y in ys]
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
            if "A" in res and "B_module" in res:
                res["A_faster_than_B_module"] = res["A"]["max"] < res["B_module"]["min"]
            if "A" in res and "C" in res:
                res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
            out[f"{wl}.{dn}"] = res
            del lv
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="bench_layout", ms_per_step=out, rounds=args.rounds, iters=args.iters)))


if __name__ == "__main__":
    main()
