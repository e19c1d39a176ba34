"""The multi-scale segmentation targets of a batch (mask_pyramid, include/mgatargets.h: one launch) beside the same pyramid composed from
torch operators on the device and beside this package's CPU composition on the host, in the same process.

    python tools/bench_targets.py [--rounds 5] [--steps 200] [--out profiles/targets/bench_targets.json]

Shapes: uint8 masks of 32 x 640 x 640 (13.1 MB read, 1.1 MB written at strides 8 / 16 / 32) and 8 x 1280 x 1280; avgpool and maxpool.
Per row, the timed things:
  fused_eager   mask_pyramid(mask, out=bufs): the public call, descriptor filled per call
  fused_call    a pre-filled descriptor launched from Python (what SlicePlan.forward does outside a graph)
  fused_graph   that launch captured in a graph of its own and replayed (what it costs inside the static step's graph)
  torch_eager   the torch composition on the device: (mask > 0).float(), one pad per stride that needs it, three pools -- written as a
                user would write it, into fresh tensors
  torch_graph   the same composition captured in a graph and replayed: torch's side without its launch overhead
  cpu           mask_pyramid on the CPU tensor (`--cpu-steps` per round; the copy of its three results to the device is NOT in it)
Protocol: everything is built, checked bit-equal and warmed first, then timed in alternating rounds of `steps` calls each, the clock read
after a device synchronise; a row reports each side's median over the rounds and its spread (max - min over the rounds), and whether the
difference of the medians of the fused and the torch side exceeds the larger spread.  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

CONFIGS = {"b32_640": (32, 640, 640), "b8_1280": (8, 1280, 1280)}
STRIDES = (8, 16, 32)


def torch_pyramid(mask, method):
    m = (mask > 0).to(torch.float32).unsqueeze(1)
    H, W = m.shape[-2:]
    pool = F.avg_pool2d if method == "avgpool" else F.max_pool2d
    out = []
    for s in STRIDES:
        p = F.pad(m, (0, -W % s, 0, -H % s)) if (H % s or W % s) else m
        out.append(pool(p, s))
    return out


def timed(fn, steps, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3 / steps


def graph_of(fn, dev):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return g, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "targets", "bench_targets.json"))
    a = ap.parse_args()
    assert a.rounds >= 5 and a.steps >= 20, "at least 5 rounds of at least 20 steps"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path"
    from mga_yolo_amd import mask_pyramid
    from mga_yolo_amd.functional import TargetPyramidCall
    dev = torch.device("cuda", 0)
    rows = []
    for cfg, (B, H, W) in CONFIGS.items():
        host = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) < 0.1).to(torch.uint8)
        mask = host.to(dev)
        for method in ("avgpool", "maxpool"):
            bufs = [torch.empty(B, 1, -(-H // s), -(-W // s), device=dev) for s in STRIDES]
            call = TargetPyramidCall(mask, bufs, STRIDES, method, False)
            fused_graph, _ = graph_of(call.run, dev)
            torch_graph, torch_out = graph_of(lambda: torch_pyramid(mask, method), dev)
            # the sides compute the same thing, bit for bit
            want = torch_pyramid(mask, method)
            cpu = mask_pyramid(host, STRIDES, method)
            for b in bufs:
                b.fill_(-1.0)
            fused_graph.replay(); torch_graph.replay()
            torch.cuda.synchronize(dev)
            for b, w, t, c in zip(bufs, want, torch_out, cpu):
                assert torch.equal(b, w) and torch.equal(t, w) and torch.equal(c, w.cpu())
            sides = dict(fused_eager=lambda: mask_pyramid(mask, STRIDES, method, out=bufs), fused_call=call.run, fused_graph=fused_graph.replay,
                         torch_eager=lambda: torch_pyramid(mask, method), torch_graph=torch_graph.replay)
            for fn in sides.values():
                timed(fn, a.warmup, dev)
            ms = {k: [] for k in list(sides) + ["cpu"]}
            for _ in range(a.rounds):                                # alternate the sides
                for k, fn in sides.items():
                    ms[k].append(timed(fn, a.steps, dev))
                t0 = time.perf_counter()
                for _ in range(a.cpu_steps):
                    mask_pyramid(host, STRIDES, method)
                ms["cpu"].append((time.perf_counter() - t0) * 1e3 / a.cpu_steps)
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            read, written = B * H * W, sum(b.numel() * 4 for b in bufs)
            row = dict(config=cfg, B=B, H=H, W=W, method=method, bytes_read=read, bytes_written=written, cpu_threads=torch.get_num_threads())
            for k in ms:
                row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 5), round(spread[k], 5), [round(v, 5) for v in ms[k]]
            for f, t in (("fused_eager", "torch_eager"), ("fused_graph", "torch_graph")):
                row[f"{f}_vs_{t}"] = round(med[t] / med[f], 2)
                row[f"{f}_vs_{t}_exceeds_spread"] = bool(abs(med[t] - med[f]) > max(spread[t], spread[f]))
            row["fused_graph_GBps"] = round((read + written) / (med["fused_graph"] * 1e-3) / 1e9, 1)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
            del sides, fused_graph, torch_graph, torch_out, call
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, cpu_steps=a.cpu_steps, warmup=a.warmup, strides=list(STRIDES),
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
