"""The image batch at training size on the device: ImagePlan's graph replay against the torch composition a user writes today.

    python tools/bench_image.py [--pairs 5] [--window 0.25] [--out profiles/image/bench_image.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_image.py --profile-run
    python tools/bench_image.py --kernel-trace <dir>/.../*_kernel_trace.csv [--out profiles/image/kernel_rows.json]

Rows: B = 32, 3 x 640 x 640 bytes to fp32 and fp16, contiguous and channels_last, without a resize and resized to 320 and to 960.
The composition is `.to(dtype) / 255` [`.contiguous(memory_format=torch.channels_last)`] [`F.interpolate(size, "bilinear")`] on the same
device bytes, timed eagerly and as a captured graph; the plan is timed as a captured graph.

Protocol: all three in one process, alternating, `--pairs` rounds after a warm-up; a round times each side over a window of at least
`--window` seconds of back-to-back replays between two device events.  A row reports each side's median over the rounds and its spread
(max - min over the rounds); `pays` says whether the plan beats the captured composition by more than the larger of the two spreads.

--profile-run makes five eager plan runs per row, in the rows' order, for a rocprofv3 kernel trace; --kernel-trace reads that trace back:
per row the kernel's median duration, the algorithmic bytes B*C*(H*W + H'*W'*w) over it, and that as a share of the 8 TB/s roofline."""
import argparse
import csv
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mga_yolo_amd import ImagePlan  # noqa: E402

B, C, H, W = 32, 3, 640, 640
ROOFLINE = 8e12
PROFILE_RUNS = 5


def rows():
    for size in (None, 320, 960):
        for dt in (torch.float32, torch.float16):
            for cl in (False, True):
                yield dict(dtype=dt, channels_last=cl, size=size)


def label(r):
    return f"{str(r['dtype']).split('.')[-1]} {'channels_last' if r['channels_last'] else 'contiguous'} {r['size'] or 'no resize'}"


def algorithmic_bytes(r):
    out = (r["size"] or H) * (r["size"] or W)
    return B * C * (H * W + out * (4 if r["dtype"] == torch.float32 else 2))


def composition(src, r):
    x = src.to(r["dtype"]) / 255
    if r["channels_last"]:
        x = x.contiguous(memory_format=torch.channels_last)
    if r["size"]:
        x = F.interpolate(x, size=(r["size"], r["size"]), mode="bilinear", align_corners=False)
    return x


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def window_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def bench(args):
    src = torch.randint(0, 256, (B, C, H, W), dtype=torch.uint8, device="cuda")
    out_rows = []
    for r in rows():
        plan = ImagePlan.create(B, C, H, W, dtype=r["dtype"], channels_last=r["channels_last"], size=r["size"])
        plan.src.copy_(src)
        g_plan, _ = capture(plan.run)
        g_comp, kept = capture(lambda: composition(src, r))
        g_plan.replay()
        g_comp.replay()
        torch.cuda.synchronize()
        if r["size"] is None:
            assert torch.equal(plan.out, kept) and plan.out.stride() == kept.stride(), label(r)
        sides = dict(plan_graph=g_plan.replay, torch_graph=g_comp.replay, torch_eager=lambda: composition(src, r))
        reps = {k: max(3, int(args.window * 1e3 / max(window_ms(fn, 10), 1e-3)) + 1) for k, fn in sides.items()}     # (also the warm-up)
        ms = {k: [] for k in sides}
        for _ in range(args.pairs):
            for k, fn in sides.items():
                ms[k].append(window_ms(fn, reps[k]))
        row = dict(row=label(r), algorithmic_MB=round(algorithmic_bytes(r) / 1e6, 1))
        for k in sides:
            row[k + "_ms"], row[k + "_spread_ms"] = round(statistics.median(ms[k]), 4), round(max(ms[k]) - min(ms[k]), 4)
            row[k + "_rounds_ms"], row[k + "_replays_per_window"] = [round(v, 4) for v in ms[k]], reps[k]
        gain = row["torch_graph_ms"] - row["plan_graph_ms"]
        row["speedup_vs_torch_graph"] = round(row["torch_graph_ms"] / row["plan_graph_ms"], 2)
        row["pays"] = bool(gain > max(row["plan_graph_spread_ms"], row["torch_graph_spread_ms"]))
        row["plan_TBps"] = round(algorithmic_bytes(r) / (row["plan_graph_ms"] * 1e-3) / 1e12, 2)
        out_rows.append(row)
        print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
        del plan, g_plan, g_comp, kept
        torch.cuda.empty_cache()
    doc = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, shape=[B, C, H, W], pairs=args.pairs, window_s=args.window,
               protocol="one process, sides alternating within a round, device events around a window of back-to-back replays; median over the "
                        "rounds, spread = max - min over a side's rounds; pays: torch_graph - plan_graph > the larger spread", rows=out_rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


def profile_run():
    src = torch.randint(0, 256, (B, C, H, W), dtype=torch.uint8, device="cuda")
    for r in rows():
        plan = ImagePlan.create(B, C, H, W, dtype=r["dtype"], channels_last=r["channels_last"], size=r["size"])
        plan.src.copy_(src)
        for _ in range(PROFILE_RUNS):
            plan.run()
        torch.cuda.synchronize()
        del plan
    return 0


def kernel_rows(args):
    with open(args.kernel_trace) as f:
        disp = [d for d in csv.DictReader(f) if "k_img_" in d["Kernel_Name"]]
    disp.sort(key=lambda d: int(d["Start_Timestamp"]))
    want = list(rows())
    assert len(disp) == PROFILE_RUNS * len(want), (len(disp), len(want))
    out_rows = []
    for i, r in enumerate(want):
        mine = disp[i * PROFILE_RUNS:(i + 1) * PROFILE_RUNS]
        names = {d["Kernel_Name"] for d in mine}
        assert len(names) == 1, names
        us = [(int(d["End_Timestamp"]) - int(d["Start_Timestamp"])) / 1e3 for d in mine]
        med = statistics.median(us)
        tbps = algorithmic_bytes(r) / (med * 1e-6) / 1e12
        row = dict(row=label(r), kernel=names.pop().replace("mgacbam::", "").split("(")[0], runs_us=[round(u, 1) for u in us], median_us=round(med, 1),
                   algorithmic_MB=round(algorithmic_bytes(r) / 1e6, 1), TBps=round(tbps, 2), share_of_8TBps=round(tbps * 1e12 / ROOFLINE, 3))
        out_rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(source="rocprofv3 --kernel-trace --stats of tools/bench_image.py --profile-run", shape=[B, C, H, W], rows=out_rows), f, indent=1)
        f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--kernel-trace")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.profile_run:
        return profile_run()
    if args.kernel_trace:
        args.out = args.out or os.path.join(ROOT, "profiles", "image", "kernel_rows.json")
        return kernel_rows(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "image", "bench_image.json")
    return bench(args)


if __name__ == "__main__":
    sys.exit(main())
