"""The rebuilt cases of tests/det_cases.py on the CPU: their features reproduce the recorded digest, the fp64 oracle meets the reference's
recorded fp64 run on them, the host path of mga_yolo_amd.detloss meets the bars, and every case holds what it was built for -- the picks
of an oversized box in every chunk of k_det_assign's visiting order, zero-metric picks that must survive the carry, more than 256 label
rows and partials, a foreground anchor on each of four levels."""
import json
import os

import numpy as np
import pytest
import torch

import det_cases as DC
import det_oracle as O

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module", params=list(DC.CASES))
def case(request):
    c = DC.load(request.param)
    c["oracle"] = O.oracle(c["feats"], *c["labels"], **c["kw"])
    return c


@pytest.mark.parametrize("name", list(DC.CASES))
def test_features_reproduce_the_recorded_digest(name):
    z = np.load(DC.path(name))
    feats = DC.build_feats(name, int(z["seed"]))
    assert DC.digest(feats) == str(z["sha256"])
    assert [tuple(f.shape) for f in feats] == [(DC.CASES[name]["B"], 64 + DC.CASES[name]["nc"], h, w) for h, w in DC.shapes(name)]
    assert all(f.dtype == torch.float32 for f in feats)
    assert os.path.getsize(DC.path(name)) < 300 * 1024 and not any(k.startswith(("feat", "g1", "gnu")) for k in z.files)


def test_bars_are_the_existing_ones_or_twice_the_reference_ratio():
    worst = json.load(open(os.path.join(O.GOLDEN, "det_ratios_shapes.json")))["worst"]
    assert DC.K == dict(loss=max(O.K["loss"], 2 * worst["loss"]), target_scores=max(O.K["target_scores"], 2 * worst["target_scores"]),
                        grad=max(O.K["grad"], 2 * worst["g1"], 2 * worst["gnu"]))
    for name in DC.CASES:                                        # the file's worst is the worst of the records themselves
        z = np.load(DC.path(name))
        for k, v in zip(z["ratio_names"], z["ratio_values"]):
            assert float(v) <= worst[str(k)]


def test_oracle_equals_the_reference_fp64_run(case):
    """Loss, items and target scores at 1e-9 of their terms; the gradients were held to the same at generation time (they are not stored)."""
    c, o = case, case["oracle"]
    O.check("loss", o["loss"], c["loss_f64"], o["terms"]["loss"], 1e-9 / O.K["loss"], O.K["loss"])
    O.check("items", o["items"], c["items_f64"], o["terms"]["loss"] / c["B"], 1e-9 / O.K["loss"], O.K["loss"])
    O.check("target_scores", o["target_scores"], c["target_scores_f64"], o["terms"]["target_scores"], 1e-9 / O.K["target_scores"], O.K["target_scores"])
    w = o["weight"] > 0
    assert torch.equal(o["fg"][w], torch.from_numpy(c["fg_mask_f64"])[w]) and bool(o["fg"][w].all())
    assert torch.equal(w, torch.from_numpy(c["target_scores_f64"]).sum(-1) > 0)


def test_host_path_against_the_record_and_the_oracle(case):
    from mga_yolo_amd import detection_loss
    c, o = case, case["oracle"]
    for up in ((1.0, 1.0, 1.0), DC.UPSTREAM):
        xs = [f.clone().requires_grad_(True) for f in c["feats"]]
        loss, items, asg = detection_loss(xs, *c["labels"], return_assignment=True, **c["kw"])
        O.check("loss", loss, c["loss_f64"], o["terms"]["loss"], EPS32, DC.K["loss"])
        O.check("items", items, c["items_f64"], o["terms"]["loss"] / c["B"], EPS32, DC.K["loss"])
        gs = torch.autograd.grad((loss * torch.tensor(up)).sum(), xs, allow_unused=True)
        for l, g in enumerate(gs):
            g = torch.zeros_like(xs[l]) if g is None else g
            O.check(f"g{up}[{l}]", g, O.grads(o, l, up), O.grad_terms(o["terms"], l, up), EPS32, DC.K["grad"])
    O.check("target_scores", asg["target_scores"], c["target_scores_f64"], o["terms"]["target_scores"], EPS32, DC.K["target_scores"])
    w = o["weight"] > 0
    assert torch.equal(asg["fg"][w], o["fg"][w]) and torch.equal(asg["target_gt"][w], o["target_gt"][w])
    assert torch.allclose(asg["target_bboxes"][w].double(), o["target_bboxes"][w], rtol=0, atol=1e-3)
    assert torch.equal(asg["weight"] > 0, w) and int(asg["status"]) == 0
    if c["name"] == "chunk_zero":                                # the project's own tie rule, at every anchor
        assert torch.equal(asg["fg"], o["fg"]) and torch.equal(asg["target_gt"], o["target_gt"])


def test_the_cases_hold_what_they_were_built_for(case):
    assert DC.built_for(case["name"], case["oracle"]) == []


def test_the_visiting_order_covers_the_anchors_inside_the_box():
    """visit_order is the statement of k_det_assign's rectangles the chunk properties rest on: every anchor the oracle found inside a box is
    in it, once, and an oversized box visits every anchor in anchor order."""
    for name in ("chunk2", "crowd", "lv4"):
        c = DC.load(name)
        o = O.oracle(c["feats"], *c["labels"], **c["kw"])
        for b, (rows, pos, met) in o["picks"].items():
            for g, r in enumerate(rows):
                order = DC.visit_order(name, r)
                assert len(set(order.tolist())) == order.size
                assert set(torch.nonzero(pos[g]).flatten().tolist()) <= set(order.tolist())
    assert np.array_equal(DC.visit_order("chunk2", 0), np.arange(DC.anchors("chunk2")))
    assert np.array_equal(DC.visit_order("chunk3", 0), np.arange(DC.anchors("chunk3"))) and DC.anchors("chunk3") == 6048
