"""The detection post-process on the host: tests/nms_oracle.py (numpy fp64) and detpost._host_postprocess (torch ops) against every stored
case of tests/nms_cases.py -- what the reference's own Detect._inference and non_max_suppression gave --, the answers known by construction,
the generator's guards recomputed -- for every max_nms override and every half rounding of a prediction the GPU tests use as well --, and
the wrong rules each failing the case built to catch it."""
import numpy as np
import pytest
import torch

import nms_cases as NC
import nms_oracle as O
from mga_yolo_amd import detect_postprocess, non_max_suppression
from mga_yolo_amd.detpost import _host_postprocess

NAMES = NC.NAMES
HALF = [torch.float16, torch.bfloat16]


def test_the_bar_is_twice_the_references_own_error_and_not_below_one():
    import json
    with open(O._RATIOS) as f:
        r = json.load(f)
    assert sorted(r["cases"]) == sorted(NC.PARITY) and r["worst"] == max(r["cases"].values())
    assert O.K == max(1.0, 2 * r["worst"])


def test_the_cases_without_parity_are_the_cuts_inside_equal_scores():
    """the reference cuts to max_nms behind an unstable argsort: which of the equal scores it keeps is not defined, so these two are held to
    their construction and the oracle"""
    assert sorted(set(NAMES) - set(NC.PARITY)) == ["cut_ties", "cut_ties_wide"] and all(n in NC.ANSWERS and n in NC.TIE_ORDER for n in NAMES if n not in NC.PARITY)


@pytest.mark.parametrize("name", NC.PARITY)
def test_oracle_keeps_what_the_reference_kept(name):
    c, o = NC.load(name), NC.oracle(name)
    assert o["count"].tolist() == [r.shape[0] for r in c["ref64"]] == [r.shape[0] for r in c["ref32"]]
    for b in range(c["B"]):
        n = int(o["count"][b])
        assert np.array_equal(o["keep"][b, :n], c["ref_keep"][b])
        for ref in (c["ref64"][b], c["ref32"][b]):
            assert np.array_equal(o["dets"][b, :n, 5], ref[:, 5])
        if n:
            # the reference's fp64 run: its scores are the oracle's but for a few fp64 roundings; its xywh2xyxy writes fp32 whatever it reads
            assert O.ratio(o["dets"][b, :n, 4], c["ref64"][b][:, 4], o["terms"][b, :n, 4]) < 1e-6
            assert O.ratio(o["dets"][b, :n, :4], c["ref64"][b][:, :4], o["terms"][b, :n, :4]) <= 0.5
            assert O.ratio(c["ref32"][b][:, :5], o["dets"][b, :n, :5], o["terms"][b, :n, :5]) <= O.K
            assert float(c["ratio"]) <= O.K / 2


@pytest.mark.parametrize("name", sorted(NC.ANSWERS))
def test_answers_known_by_construction(name):
    o = NC.oracle(name)
    keep, cls = NC.ANSWERS[name]
    for b in range(NC.CASES[name]["B"]):
        n = int(o["count"][b])
        assert o["keep"][b, :n].tolist() == keep[b] and o["dets"][b, :n, 5].astype(int).tolist() == cls[b]
    if name == "maxdet":
        assert (o["dets"][0, 5:] == 0).all() and o["dets"].shape[1] == 5


@pytest.mark.parametrize("name", NAMES)
def test_host_path_against_the_oracle(name):
    c, o = NC.load(name), NC.oracle(name)
    k = {x: v for x, v in c["kw"].items()}
    NC.check(f"host {name}", *detect_postprocess(c["feats"], **k), o)
    d64, n64, k64 = _host_postprocess([f.double() for f in c["feats"]], None, k["nc"], k["strides"], k["conf_thres"], k["iou_thres"], k["max_det"],
                                      k["max_nms"], k["multi_label"], k["agnostic"])
    NC.check(f"host fp64 {name}", d64, n64, k64, o, bar=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_pred_front_end_on_the_host(name):
    c = NC.load(name)
    k = dict(c["kw"])
    strides = k.pop("strides")
    pred = NC.ref_decode(c["feats"], strides, k["nc"])
    op = NC.oracle(name, front="pred")
    NC.check(f"host pred {name}", *detect_postprocess(pred, **k), op)
    assert np.array_equal(op["keep"], NC.oracle(name)["keep"]) and np.array_equal(op["count"], NC.oracle(name)["count"])
    if name not in NC.PARITY:
        return
    # the reference's call form, against the reference's own lists
    out, idx = non_max_suppression((pred, c["feats"]), **{x: v for x, v in k.items() if x != "nc"}, return_idxs=True)
    for b in range(c["B"]):
        assert out[b].shape == c["ref32"][b].shape and idx[b].tolist() == c["ref_keep"][b].tolist()
        n = out[b].shape[0]
        if n:
            assert O.ratio(out[b][:, :5].numpy(), c["ref64"][b][:, :5], op["terms"][b, :n, :5]) <= O.K + 0.5


@pytest.mark.parametrize("name", NAMES)
def test_the_generators_guards_hold(name):
    c = NC.load(name)
    for dt in (None, torch.float16, torch.bfloat16):
        assert O.guards(NC.oracle(name, dt)) == [], (name, dt)
    assert NC.built_for(name, c["feats"]) == []
    if name not in NC.TIE_ORDER:
        hi = O.oracle(feats=[f.numpy() for f in c["feats"]], lowest_first=False, **c["kw"])
        assert np.array_equal(hi["keep"], NC.oracle(name)["keep"]) and np.array_equal(hi["dets"], NC.oracle(name)["dets"])


@pytest.mark.parametrize("name", sorted(NC.MUTATIONS))
def test_each_wrong_rule_fails_the_case_built_for_it(name):
    """Keep what a suppressed box would have suppressed suppressed (chain), let classes suppress each other (classes), forget max_nms (maxnms),
    break ties by the highest index (ties; cut_ties and cut_ties_wide: at the max_nms cut): each changes the kept rows of its case."""
    c, o = NC.load(name), NC.oracle(name)
    wrong = O.oracle(feats=[f.numpy() for f in c["feats"]], **dict(c["kw"], **NC.MUTATIONS[name]))
    assert not np.array_equal(wrong["keep"], o["keep"])
    if name in NC.TIE_ORDER:                                      # the host path's other order differs as the oracle's does
        k = c["kw"]
        d, n, kp = _host_postprocess(c["feats"], None, k["nc"], k["strides"], k["conf_thres"], k["iou_thres"], k["max_det"], k["max_nms"],
                                     k["multi_label"], k["agnostic"], lowest_first=False)
        assert np.array_equal(kp.numpy(), wrong["keep"])


@pytest.mark.parametrize("max_nms", NC.SELECT_CUTS)
def test_select_at_every_cut_on_the_host(max_nms):
    """images 0 and 1 of `wide` cut at, around and far from kNmsLds and their own length: the guards hold under every override, the count is
    what the cut leaves, and the host path gives the oracle's answer"""
    feats, k, o = NC.select_case(max_nms)
    assert O.guards(o) == [] and o["n_cand"] == [NC.anchors("wide")] * 2
    for dt in HALF:
        assert O.guards(O.oracle(feats=[f.to(dt).float().numpy() for f in feats], **k)) == [], dt
    free = NC.select_case(NC.SELECT_CUTS[-1])[2]
    assert (o["count"] <= max_nms).all() and (free["count"] - o["count"] <= NC.anchors("wide") - max_nms).all() and o["count"].max() == min(max_nms, free["count"].max())
    NC.check(f"host select {max_nms}", *detect_postprocess(feats, **k), o)


@pytest.mark.parametrize("dtype", HALF, ids=["fp16", "bf16"])
@pytest.mark.parametrize("name,over", NC.PRED_HALF_CASES, ids=NC.PRED_HALF_IDS)
def test_pred_front_end_in_half_on_the_host(name, over, dtype):
    """a prediction rounded to fp16 / bf16: the guards hold on its upcast values and the host path gives the oracle's answer; in `wide` the
    scores tie by the hundreds and the tie order decides the answer, and under the cut some image's ranks max_nms and max_nms + 1 tie"""
    pred, k, o = NC.pred_half(name, dtype, **over)
    assert O.guards(o) == []
    NC.check(f"host pred {dtype} {name} {over}", *detect_postprocess(pred, **k), o)
    if name == "wide":
        sc = pred[:, 4].float().numpy()
        tied = [int((lambda n: n[n > 1].sum())(np.unique(sc[b], return_counts=True)[1])) for b in range(sc.shape[0])]
        assert min(tied) >= 300                                   # of an image's 1344 scores, those that share their value with another
        hi = NC.pred_half(name, dtype, lowest_first=False, **over)[2]
        assert O.guards(hi) == [] and not np.array_equal(hi["keep"], o["keep"])
    if over:
        ranked = -np.sort(-sc, 1)
        cut = ranked[:, k["max_nms"] - 1] == ranked[:, k["max_nms"]]
        assert cut.sum() >= 4 and (o["count"][cut] == k["max_nms"]).any() and o["count"].max() < k["max_det"]


def test_arguments_that_are_not_built_raise():
    pred = torch.zeros(1, 5, 8)
    for kw in (dict(classes=[0]), dict(labels=[torch.zeros(1, 5)]), dict(rotated=True), dict(end2end=True), dict(nc=3)):
        with pytest.raises(NotImplementedError):
            non_max_suppression(pred, **kw)
    with pytest.raises(NotImplementedError):
        non_max_suppression(torch.zeros(1, 300, 6))
    with pytest.raises(ValueError):
        detect_postprocess(pred, nc=1, conf_thres=1.5)
    assert [o.shape for o in non_max_suppression(pred)] == [(0, 6)]
