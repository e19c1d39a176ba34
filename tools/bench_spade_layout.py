"""MaskSPADE through mask_spade_pyramid on channels_last features, in three forms measured in ONE build (one JSON line per row):

  A   channels_last x / gy through the channels-last kernels (MGASPADE_LAYOUT_NHWC); y and gx come back channels_last
  B   the same channels_last data the way the NCHW-only block took it: x.contiguous() and gy.contiguous() in, the NCHW kernels, y and gx
      converted back to channels_last as a channels_last neighbour would.  The NCHW kernels are the same code before and after the
      channels-last path was added, so this is the earlier path, not a second build of an older commit
  C   NCHW data through the NCHW kernels (reference point)

Shapes: bench_spade.py's cfg2 and cfg3 (batch 32, P3/P4/P5 of 640x640), fp32 and fp16 (fp16 features under torch.autocast, fp32
parameters), forward (torch.no_grad) and step (forward + backward to x, the mask and the six parameters).  Round r times `iters` calls of
each form with device events, the order alternating between rounds.  Per row: every round, the medians, `spread` = the largest
difference between two rounds of the same form, and for the step the bar: A is not slower than B by more than B's own spread.
A against C is reported, not barred.

    python tools/bench_spade_layout.py [--rounds 5] [--iters 20] [--norm in|bn] [--out bench_spade_layout.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_spade_layout.py --hip-only --rounds 1 --iters 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from bench_spade import CONFIGS, timed  # noqa: E402
from mga_yolo_amd import MaskSPADE, mask_spade_pyramid  # noqa: E402

CL = torch.channels_last


def make(cfg, dtype, dev, norm):
    B, lv = CONFIGS[cfg]
    g = torch.Generator().manual_seed(1234)
    levels = []
    for C, H, W in lv:
        torch.manual_seed(0)
        m = MaskSPADE(C, norm_type=norm).to(dev)
        x = torch.randn(B, C, H, W, generator=g).to(dev, dtype)
        mask = torch.randn(B, 1, H, W, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(B, C, H, W, generator=g).to(dev, dtype)
        levels.append(dict(m=m, x=x, x_cl=x.contiguous(memory_format=CL), mask=mask, gy=gy, gy_cl=gy.contiguous(memory_format=CL)))
    return levels


def forms(levels, dtype):
    amp = torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16)

    def running(m):
        return (m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if m.spade_config().bn else None

    def run(form, grad):
        def fn():
            xs, gys = [], []
            for d in levels:
                if form == "A":
                    x, gy = d["x_cl"], d["gy_cl"]
                elif form == "C":
                    x, gy = d["x"], d["gy"]
                else:
                    x, gy = d["x_cl"].contiguous(), (d["gy_cl"].contiguous() if grad else None)     # the copies the NCHW-only block made
                xs.append(x.detach().requires_grad_(grad))
                gys.append(gy)
            with amp, torch.set_grad_enabled(grad):
                ys = mask_spade_pyramid([(x, d["mask"], d["m"].spade_params(), d["m"].spade_config(), running(d["m"])) for x, d in zip(xs, levels)])
            gx = []
            if grad:
                wrt = xs + [d["mask"] for d in levels] + [p for d in levels for p in d["m"].parameters()]
                gx = torch.autograd.grad(ys, wrt, gys)[:len(xs)]
            if form == "B":                                                  # the channels_last neighbours convert y and gx back
                ys = [y.contiguous(memory_format=CL) for y in ys]
                gx = [t.contiguous(memory_format=CL) for t in gx]
            return ys, gx
        return fn
    return {"forward": {f: run(f, False) for f in "ABC"}, "step": {f: run(f, True) for f in "ABC"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--norm", default="in", choices=["in", "bn"])
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="run form A alone (for a kernel trace of the channels-last launches)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spade_layout.py measures on the GPU only"
    dev = torch.device("cuda:0")
    rows = []
    for cfg in a.configs.split(","):
        for dtype in (torch.float32, torch.float16):
            levels = make(cfg, dtype, dev, a.norm)
            for what, fns in forms(levels, dtype).items():
                names = ["A"] if a.hip_only else ["A", "B", "C"]
                for f in names:                               # warm up every shape of every form
                    for _ in range(3):
                        fns[f]()
                torch.cuda.synchronize()
                t = {f: [] for f in names}
                for r in range(a.rounds):
                    for f in (names if r % 2 == 0 else names[::-1]):
                        t[f].append(round(timed(fns[f], a.iters), 4))
                med = {f: statistics.median(v) for f, v in t.items()}
                spread = {f: round(max(v) - min(v), 4) for f, v in t.items()}
                row = dict(config=cfg, dtype=str(dtype).split(".")[-1], norm=a.norm, what=what, unit="ms", rounds=t, median=med, spread=spread)
                if not a.hip_only:
                    row.update(A_minus_B_ms=round(med["A"] - med["B"], 4), A_over_C=round(med["A"] / med["C"], 3))
                    if what == "step":
                        row["A_within_bar"] = bool(med["A"] - med["B"] <= spread["B"])
                rows.append(row)
                print(json.dumps(row), flush=True)
            del levels
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
