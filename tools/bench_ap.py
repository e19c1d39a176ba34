"""Average precision per class on the device (include/ext/mgaap.h) beside the reference's procedure on the host, read-back included, and
beside the same procedure composed from torch operators on the device, in the same process.

    python tools/bench_ap.py [--rounds 5] [--steps 10] [--out profiles/ap/bench_ap.json]

Inputs: a run's accumulation of 2^17, 2^20 and 1.5 M detection rows with niou = 10, nc = 1 and nc = 80, half as many label rows as detections,
about a third of the rows true at the first threshold (tests/ap_cases.random_case: distinct confidences, at most nt true rows a class),
written into a DetMatchPlan's arena.  Per row, the timed things:
  ap_graph      DetApPlan.run captured in a graph and replayed
  ap_eager      DetApPlan.run, the launches issued one by one
  ap_results    run() + results(): the path a validator takes -- the launches, one read-back of the result block, the numpy finish
  host          DetMatchPlan.stats() + detap._host_ap: the read-back of every row and the reference's procedure in numpy on one core
  torch_device  the same procedure from torch operators on the device tensors (one sort, a loop over the classes with labels: cumsum, flip /
                cummax / flip, searchsorted interpolation), its (nc, niou + 3000) results read back
Protocol: tools/bench_confusion.py's -- everything is built, compared and warmed first (the device's curves equal to the host's, ap within
128 * 2^-53 * S; the torch composition's difference is reported, not asserted), then timed in alternating rounds of `steps` calls each (the
host side: `slow_steps`), the clock read after a device synchronise; a row reports each side's median over the rounds and its spread (max -
min over the rounds), and whether run() + results() beat stats() + host in EVERY round.  No figure is fixed in advance."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bench_confusion import capture  # noqa: E402
from bench_match import timed  # noqa: E402

NIOU = 10
SIZES = {"2^17": 1 << 17, "2^20": 1 << 20, "1.5M": 1500000}
CLASSES = (1, 80)


def _interp(x, xp, fp, left=None):
    """np.interp's index rule in torch ops (fp64)"""
    last = xp.numel() - 1
    j = torch.searchsorted(xp, x, right=True) - 1
    at = j.clamp(0, last)
    nxt = (at + 1).clamp(max=last)
    between = (fp[nxt] - fp[at]) / (xp[nxt] - xp[at]) * (x - xp[at]) + fp[at]
    out = torch.where((at == last) | (xp[at] == x), fp[at], between)
    return torch.where(j < 0, torch.full_like(out, fp[0].item() if left is None else left), out)


def torch_device(tp, conf, pred_cls, target_cls, nc, x101, x1000):
    """the reference's procedure from torch operators, on whatever device the tensors live; -> (ap, p_curve, r_curve, prec_values) dense, on the host"""
    order = torch.argsort(conf, descending=True, stable=True)
    tp, conf, pred_cls = tp[order], conf[order].double(), pred_cls[order]
    nt = torch.bincount(target_cls.long(), minlength=nc)
    niou = tp.shape[1]
    out = torch.zeros(nc, niou + 3000, dtype=torch.float64, device=tp.device)
    one, zero = torch.ones(1, dtype=torch.float64, device=tp.device), torch.zeros(1, dtype=torch.float64, device=tp.device)
    for c in torch.nonzero(nt).flatten().tolist():
        sel = pred_cls == c
        if not bool(sel.any()):
            continue
        tpc = tp[sel].double().cumsum(0)
        recall = tpc / (nt[c].double() + 1e-16)
        precision = tpc / torch.arange(1, tpc.shape[0] + 1, dtype=torch.float64, device=tp.device)[:, None]
        xp = -conf[sel]
        out[c, niou + 1000:niou + 2000] = _interp(-x1000, xp, recall[:, 0].contiguous(), left=0.0)
        out[c, niou:niou + 1000] = _interp(-x1000, xp, precision[:, 0].contiguous(), left=1.0)
        for t in range(niou):
            mrec = torch.cat((zero, recall[:, t], one))
            mpre = torch.cat((one, precision[:, t], zero)).flip(0).cummax(0).values.flip(0)
            y = _interp(x101, mrec, mpre)
            out[c, t] = ((x101[1:] - x101[:-1]) * (y[1:] + y[:-1]) / 2.0).sum()
            if t == 0:
                out[c, niou + 2000:] = _interp(x1000, mrec, mpre)
    h = out.cpu().numpy()
    return h[:, :niou], h[:, niou:niou + 1000], h[:, niou + 1000:niou + 2000], h[:, niou + 2000:]


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--rounds", type=int, default=5)
    ap_.add_argument("--steps", type=int, default=10)
    ap_.add_argument("--slow-steps", type=int, default=1)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--only", nargs="*", help="sizes, e.g. 2^17")
    ap_.add_argument("--out", default=os.path.join("profiles", "ap", "bench_ap.json"))
    a = ap_.parse_args()
    assert a.rounds >= 5, "at least 5 rounds"
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no other path for device tensors"
    import ap_cases as AC
    import ap_oracle as AO
    from mga_yolo_amd import DetApPlan, DetMatchPlan, _lib, detap
    dev = torch.device("cuda", 0)
    x101, x1000 = (torch.from_numpy(g).to(dev) for g in detap.grids())
    rows = []
    for size, n in SIZES.items():
        if a.only and size not in a.only:
            continue
        for nc in CLASSES:
            c = AC.random_case(np.random.default_rng([5, n, nc]), n, n // 2, nc, NIOU, labelled=nc)
            m = c["target_cls"].shape[0]
            match = DetMatchPlan.create(1, 1, n_cap=1, m_cap=1, imgsz=64, rows_cap=n, tgt_cap=m)
            plan = DetApPlan.create(match, nc=nc)
            rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state = plan._st.args[:7]
            rows_tp.copy_(torch.from_numpy(c["tp"].astype(np.uint8)))
            for dst, k in ((rows_conf, "conf"), (rows_cls, "pred_cls"), (tgt_cls, "target_cls")):
                dst.copy_(torch.from_numpy(c[k]))
            rows_img.copy_(torch.arange(n, dtype=torch.int32) // 300)
            tgt_img.copy_(torch.arange(m, dtype=torch.int32) // 150)
            state.copy_(torch.tensor([n, m, (n + 299) // 300, 0], dtype=torch.int32))
            graph = capture(dev, plan)

            def results():
                plan.run()
                return plan.results()

            def host():
                s = match.stats()
                return detap._host_ap(s["tp"], s["conf"], s["pred_cls"], s["target_cls"], nc=nc)

            def composed():
                return torch_device(rows_tp != 0, rows_conf, rows_cls, tgt_cls, nc, x101, x1000)
            graph.replay()
            torch.cuda.synchronize(dev)
            plan.check_status()
            by_graph = plan.result.cpu().numpy().copy()
            got, want = results(), host()
            assert by_graph.tobytes() == plan.result.cpu().numpy().tobytes(), "the replay's and the eager run's bytes"
            dense = detap._host_curves(c["tp"], c["conf"], c["pred_cls"], c["target_cls"], nc)
            ap_abs = AO.AP_ULPS * np.ones_like(want[5])                   # every term is non-negative and the sum at most 1: S <= 1
            for i, (g, w) in enumerate(zip(got, want)):
                assert (np.abs(g - w) <= ap_abs).all() if i == 5 else np.array_equal(g, w), f"output {i} of the device and the host differ"
            assert np.array_equal(plan._st.dense()["nt"], dense["nt"])
            t_ap, t_p, t_r, t_prec = composed()
            keep = dense["nt"] > 0
            torch_diff = float(max(np.abs(t_ap[keep] - got[5]).max(), np.abs(t_p[keep] - got[7]).max(), np.abs(t_r[keep] - got[8]).max()))
            sides = dict(ap_graph=(graph.replay, a.steps), ap_eager=(plan.run, a.steps), ap_results=(results, a.steps), host=(host, a.slow_steps),
                         torch_device=(composed, a.slow_steps))
            for k, (fn, steps) in sides.items():
                timed(fn, 1 if steps == a.slow_steps else a.warmup, dev)
            ms = {k: [] for k in sides}
            for _ in range(a.rounds):                                    # alternate the sides
                for k, (fn, steps) in sides.items():
                    ms[k].append(timed(fn, steps, dev))
            plan.check_status()
            med = {k: statistics.median(v) for k, v in ms.items()}
            passes = 4 + (0 if nc <= 1 else 1 if nc <= 256 else 2)
            row = dict(rows=size, n_rows=n, n_targets=m, nc=nc, niou=NIOU, true_at_t0=round(float(c["tp"][:, 0].mean()), 3),
                       launches=3 + 3 * passes + 7 * NIOU, ws_bytes=int(plan._st.ws.numel()), result_bytes=int(plan.result.numel()),
                       rows_read_back_by_host_bytes=int(match._arena.numel()), mAP50=round(float(got[5][:, 0].mean()), 6),
                       torch_device_max_abs_diff=torch_diff)
            for k in ms:
                row[k + "_ms"], row[k + "_spread_ms"], row[k + "_rounds_ms"] = round(med[k], 4), round(max(ms[k]) - min(ms[k]), 4), [round(v, 4) for v in ms[k]]
            row["results_beats_host_in_every_round"] = bool(all(r < h for r, h in zip(ms["ap_results"], ms["host"])))
            row["host_vs_ap_results"] = round(med["host"] / med["ap_results"], 1)
            row["torch_device_vs_ap_results"] = round(med["torch_device"] / med["ap_results"], 1)
            rows.append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_rounds_ms")}), flush=True)
            del graph, plan, match
            torch.cuda.empty_cache()
    out = dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, steps=a.steps, slow_steps=a.slow_steps, warmup=a.warmup,
               protocol="alternating rounds, median over rounds, spread = max - min over a side's rounds, clock read after a synchronise", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
