"""MaskSPADE on an MI355X: the HIP path (one mask_spade_pyramid call each way) beside the block's torch composition (spade_compose, the
reference's operator sequence) on the same GPU, same inputs.  Shapes: the P3/P4/P5 levels of bench.py's cfg2 and cfg3 (batch 32, 640x640),
fp32 and fp16 (fp16 = fp16 features under torch.autocast, fp32 parameters: the reference trainer's default numeric mode).

Forward time and step (forward + backward to x, mask and the six parameters) time come from INTERLEAVED pairs: round r times `iters`
calls of one side, then of the other, with device events; the order alternates between rounds.  Per row the output holds every round of
both sides, the medians, and `spread` = the largest difference between two rounds of the same side: a gain counts only beyond it.
Not the headline benchmark (bench.py is); prints one JSON line per row and writes them to --out.

    python tools/bench_spade.py [--rounds 5] [--iters 20] [--out bench_spade.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_spade.py --hip-only --rounds 1 --iters 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from mga_yolo_amd import MaskSPADE, mask_spade_pyramid  # noqa: E402
from mga_yolo_amd.functional import spade_compose  # noqa: E402

CONFIGS = {"cfg2": (32, [(64, 80, 80), (128, 40, 40), (256, 20, 20)]), "cfg3": (32, [(128, 80, 80), (256, 40, 40), (512, 20, 20)])}


def flops_fwd(B, lv, hidden=64):
    return sum(2 * B * H * W * (2 * C * hidden * 9 + hidden * 9) for C, H, W in lv)


def make(cfg, dtype, dev):
    B, lv = CONFIGS[cfg]
    g = torch.Generator().manual_seed(1234)
    levels = []
    for C, H, W in lv:
        torch.manual_seed(0)
        m = MaskSPADE(C).to(dev)
        x = torch.randn(B, C, H, W, generator=g).to(dev, dtype).requires_grad_(True)
        mask = torch.randn(B, 1, H, W, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(B, C, H, W, generator=g).to(dev, dtype)
        levels.append((m, x, mask, gy))
    return levels


def sides(levels, dtype):
    amp = torch.autocast("cuda", dtype=torch.float16, enabled=dtype == torch.float16)

    def hip_fwd():
        with amp:
            return mask_spade_pyramid([(x, mask, m.spade_params(), m.spade_config()) for m, x, mask, _ in levels])

    def torch_fwd():
        with amp:
            return [spade_compose(x, mask, m.spade_params(), m.spade_config()) for m, x, mask, _ in levels]

    def step(fwd):
        def run():
            ys = fwd()
            torch.autograd.backward(list(ys), [gy for *_, gy in levels])
            for m, x, mask, _ in levels:
                x.grad = mask.grad = None
                m.zero_grad(set_to_none=True)
        return run

    def nograd(fwd):
        def run():
            with torch.no_grad():
                fwd()
        return run
    return {"forward": (nograd(hip_fwd), nograd(torch_fwd)), "step": (step(hip_fwd), step(torch_fwd))}


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="time the HIP side alone (for a kernel trace of this block's launches)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spade.py measures on the GPU only"
    dev = torch.device("cuda:0")
    rows = []
    for cfg in CONFIGS:
        for dtype in (torch.float32, torch.float16):
            levels = make(cfg, dtype, dev)
            for what, (hip, ref) in sides(levels, dtype).items():
                both = (("hip", hip),) if a.hip_only else (("hip", hip), ("torch", ref))
                for _, fn in both:                        # warm up every shape of both sides
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                t = {name: [] for name, _ in both}
                for r in range(a.rounds):
                    order = both if r % 2 == 0 else both[::-1]
                    for name, fn in order:
                        t[name].append(round(timed(fn, a.iters), 4))
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = max(max(v) - min(v) for v in t.values())
                B, lv = CONFIGS[cfg]
                row = dict(config=cfg, dtype=str(dtype).split(".")[-1], what=what, unit="ms", rounds=t, median=med, spread=round(spread, 4))
                if not a.hip_only:
                    row.update(gain_ms=round(med["torch"] - med["hip"], 4), gain_beyond_spread=bool(med["torch"] - med["hip"] > spread))
                if what == "forward":
                    row["hip_forward_TFLOPs"] = round(flops_fwd(B, lv) / (med["hip"] * 1e-3) / 1e12, 2)
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
