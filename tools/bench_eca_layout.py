"""Forward + backward of MaskECA through mask_eca_pyramid on channels_last features, in three forms (prints one JSON line):

  A   channels_last x / gy through the channels-last kernels (MGACBAM_LAYOUT_NHWC); y and gx come back channels_last
  B   the same channels_last data the way the NCHW-only block took it: x.contiguous() and gy.contiguous() in, the NCHW kernels, y and gx
      converted back to channels_last as a channels_last neighbour would.  This is the copy path emulated inside ONE build (the NCHW kernels
      are the same code before and after the channels-last path was added), not a second build of an older commit
  C   NCHW inputs through the NCHW kernels (reference point)

Usage: python tools/bench_eca_layout.py [--workloads cfg2,cfg3,cfg4] [--dtypes f32,f16,bf16] [--rounds 10] [--iters 10] [--warmup 10]
Timing: device events around `iters` steps, forms alternated round by round after `warmup` steps per form; median and spread (min, max)
per form, in ms per step.  The workloads are bench.WORKLOADS (P3/P4/P5 shapes and batch); `bytes` is the block's algorithmic traffic
(3 E forward + 5 E backward elements), so bytes / median is the achieved rate of form A."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from mga_yolo_amd import MaskECA  # noqa: E402
from mga_yolo_amd import functional as F  # noqa: E402

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
        torch.manual_seed(0)
        blk = MaskECA(C)
        lv.append(dict(x_cl=x.to(memory_format=CL), x=x, m=m.requires_grad_(True), gy_cl=gy.to(memory_format=CL), gy=gy,
                       w=blk.conv1d.weight.detach().cuda().requires_grad_(True), beta=blk.beta.detach().cuda().requires_grad_(True),
                       cfg=blk.eca_config()))
    return lv


def step(lv, form):
    levels, gys = [], []
    for d in lv:
        if form == "A":
            x, gy = d["x_cl"], d["gy_cl"]
        elif form == "C":
            x, gy = d["x"], d["gy"]
        else:
            x, gy = d["x_cl"].contiguous(), d["gy_cl"].contiguous()      # the copies the NCHW-only block made
        levels.append((x.detach().requires_grad_(True), d["m"], d["w"], d["beta"], d["cfg"]))
        gys.append(gy)
    ys = F.mask_eca_pyramid(levels)
    gx = torch.autograd.grad(ys, [l[0] for l in levels], gys)
    if form == "B":                                                      # the channels_last neighbours convert y and gx back
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forms", default="A,B,C")
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
            E = sum(d["x"].numel() for d in lv)
            res["bytes"] = 8 * E * lv[0]["x"].element_size()
            if "A" in res and "B" in res:
                res["A_faster_than_B"] = res["A"]["max"] < res["B"]["min"]     # beyond the spread of the rounds
            if "A" in res and "C" in res:
                res["A_over_C"] = round(res["A"]["median"] / res["C"]["median"], 3)
            out[f"{wl}.{dn}"] = res
            del lv
            torch.cuda.empty_cache()
    print(json.dumps(dict(tool="bench_eca_layout", ms_per_step=out, rounds=args.rounds, iters=args.iters, warmup=args.warmup)))


if __name__ == "__main__":
    main()
