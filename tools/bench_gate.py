"""ProbMaskGater inside the static step, on an MI355X at BASELINE config 2 (bench.py's cfg2: batch 32, the P3/P4/P5 levels of YOLOv8n at
640x640).  Three measurements, in tools/bench_spade.py's protocol -- INTERLEAVED rounds (the order alternates between rounds), the median
per side, and `spread` = the largest difference between two rounds of one side; a difference counts only beyond it:

 (a) slice_ungated  the SlicePlan step with gate=None, this commit against its parent.  Two checkouts cannot share a process, so this row is
                    assembled from runs of `--part ungated` (which uses nothing the parent lacks, so the same file runs in the parent's
                    tree), started alternately: --ab-parent a.json c.json --ab-this b.json d.json.  Nothing that step runs changed, so
                    the two must be level within the spread.
 (b) slice_gated    the SlicePlan step with a gumbel gate on every level beside the ungated one, both replayed from their graphs in one
                    process.  The difference is the price of the gate's two launches; it is reported, not barred.
 (c) gate_alone     the three levels' gate alone, forward + backward through autograd: prob_mask_gate_pyramid (1 + 1 launches) beside the
                    existing per-level path (per level 2 torch.rand + prob_mask_gate, and its backward: 9 + 3 launches), eager calls,
                    10 x --steps of them per round.  Bar: the new path is faster by more than the larger of the two sides' spreads.

    python tools/bench_gate.py [--rounds 5] [--steps 200] [--out profiles/gate/bench_gate.json] [--ab-parent F.. --ab-this F..]
    python tools/bench_gate.py --part ungated --out F        # one side of (a); runs in either checkout
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402

WORKLOAD = "cfg2"


def make_plan(dev, gate=None):
    """bench.slice_step's plan and inputs; gate: None or a GateConfig per level"""
    from mga_yolo_amd import MGAMaskHead, MaskCBAM
    from mga_yolo_amd.slice import SlicePlan
    _, batch, lv = bench.WORKLOADS[WORKLOAD]
    shapes, hidden, cps, cfgs, hss = [], [], [], [], []
    for (C, H, W) in lv:
        torch.manual_seed(0)
        m = MaskCBAM(C)
        hid = max(8, ((C // 4) + 7) // 8 * 8)
        h = MGAMaskHead(C, hid)
        shapes.append((batch, C, H, W)); hidden.append(hid); cps.append(m.block_params()); cfgs.append(m.block_config()); hss.append(h.state_dict())
    kw = {} if gate is None else dict(gate=gate(len(shapes)), seed=1)
    plan = SlicePlan(shapes, hidden, cps, cfgs, hss, device=dev, **kw)
    g = torch.Generator(device="cpu").manual_seed(7)
    for l, (B, C, H, W) in enumerate(shapes):
        plan.x[l].copy_(torch.nn.functional.silu(torch.randn(B, C, H, W, generator=g)))
        plan.gy[l].copy_(torch.randn(B, C, H, W, generator=g))
        plan.targets[l].copy_((torch.rand(B, 1, H, W, generator=g) > 0.9).float())
    plan.det_loss.copy_(torch.tensor([1.0, 0.5, 1.5]))
    graph = plan.capture(plan.step)
    return plan, graph, shapes


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def interleaved(sides, rounds, iters):
    """sides: ((name, fn), ...) -> dict(rounds, median, spread).  Warm-up: one untimed round of every side, in the timed rounds' form (the
    first round of eager calls otherwise also measures the allocator and the clocks settling)."""
    for _, fn in sides:
        timed(fn, iters)
    t = {name: [] for name, _ in sides}
    for r in range(rounds):
        for name, fn in (sides if r % 2 == 0 else sides[::-1]):
            t[name].append(round(timed(fn, iters), 5))
    return dict(unit="ms", rounds=t, median={k: statistics.median(v) for k, v in t.items()},
                spread=round(max(max(v) - min(v) for v in t.values()), 5))


def gate_alone_sides(shapes, dev):
    from mga_yolo_amd import GateConfig, gate_state, prob_mask_gate, prob_mask_gate_pyramid
    g = torch.Generator().manual_seed(3)
    ps = [torch.randn(B, 1, H, W, generator=g).to(dev).requires_grad_(True) for B, _, H, W in shapes]
    gouts = [torch.randn(B, 1, H, W, generator=g).to(dev) for B, _, H, W in shapes]
    cfgs = [GateConfig("gumbel")] * len(ps)
    state = gate_state(1, 0, dev)

    def clear():
        for p in ps:
            p.grad = None

    def new():
        torch.autograd.backward(list(prob_mask_gate_pyramid(ps, state, cfgs)), gouts)
        clear()

    def old():
        outs = [prob_mask_gate(p, torch.rand(p.shape, device=dev), torch.rand(p.shape, device=dev)) for p in ps]
        torch.autograd.backward(outs, gouts)
        clear()
    return (("pyramid", new), ("per_level", old))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="graph replays / eager calls per round")
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=["all", "ungated"], default="all")
    ap.add_argument("--ab-parent", nargs="*", default=[], help="--part ungated outputs of the parent commit's tree")
    ap.add_argument("--ab-this", nargs="*", default=[], help="--part ungated outputs of this tree, started alternately with the parent's")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gate.py measures on the GPU only"
    dev = torch.device("cuda:0")
    rows = []
    plan, graph, shapes = make_plan(dev)
    if a.part == "ungated":
        row = dict(what="slice_ungated_one_side", config=WORKLOAD, **interleaved((("ungated", graph.replay),), a.rounds, a.steps))
        plan.check_handoff()
        rows.append(row)
    else:
        from mga_yolo_amd import GateConfig
        if a.ab_parent and a.ab_this:
            t = {"parent": [], "this": []}
            for side, files in (("parent", a.ab_parent), ("this", a.ab_this)):
                for f in files:
                    t[side] += json.load(open(f))[0]["rounds"]["ungated"]
            med = {k: statistics.median(v) for k, v in t.items()}
            spread = round(max(max(v) - min(v) for v in t.values()), 5)
            rows.append(dict(what="slice_ungated", config=WORKLOAD, unit="ms", rounds=t, median=med, spread=spread,
                             diff_ms=round(med["this"] - med["parent"], 5), level_within_spread=bool(abs(med["this"] - med["parent"]) <= spread)))
        gplan, ggraph, _ = make_plan(dev, gate=lambda n: [GateConfig("gumbel")] * n)
        row = dict(what="slice_gated", config=WORKLOAD, **interleaved((("ungated", graph.replay), ("gated", ggraph.replay)), a.rounds, a.steps),
                   launches=gplan.launches())
        row["gate_cost_ms"] = round(row["median"]["gated"] - row["median"]["ungated"], 5)
        plan.check_handoff(); gplan.check_handoff()
        rows.append(row)
        # eager calls are ~0.1 ms each: ten times the calls per round, so that a round is a few tenths of a second like the replayed ones
        row = dict(what="gate_alone", config=WORKLOAD, levels=[list(s) for s in shapes], calls_per_round=10 * a.steps,
                   **interleaved(gate_alone_sides(shapes, dev), a.rounds, 10 * a.steps))
        row["gain_ms"] = round(row["median"]["per_level"] - row["median"]["pyramid"], 5)
        row["gain_beyond_spread"] = bool(row["gain_ms"] > row["spread"])
        rows.append(row)
    for row in rows:
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
