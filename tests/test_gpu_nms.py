"""The detection post-process on the device (include/mganms.h, csrc/nms.cuh) against tests/nms_oracle.py on every case of tests/nms_cases.py.
The kept set, its order, cls, keep and count are exact; coordinates and scores lie within K eps_fp32 terms, K = twice the largest ratio of
the reference's own fp32 run against its fp64 run over the cases (tests/golden/nms_ratios.json: 0.94, so K = 1.88), not below 1.  Half
features: the same bar against the oracle of the upcast values.  tests/nms_cases.py says which case runs which path of the kernels; the cases
with parity=False (the max_nms cut inside equal scores) are held to the oracle and their construction, not to the reference's lists."""
import numpy as np
import pytest
import torch

import nms_cases as NC
import nms_oracle as O

pytestmark = pytest.mark.gpu
NAMES = NC.NAMES
HALF = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])


def _run(name, dtype=torch.float32, **over):
    from mga_yolo_amd import detect_postprocess
    c = NC.load(name)
    feats = [f.cuda().to(dtype) for f in c["feats"]]
    return detect_postprocess(feats, **dict(c["kw"], **over))


@pytest.mark.parametrize("name", NAMES)
def test_every_case_fp32(name):
    NC.check(f"fp32 {name}", *_run(name), NC.oracle(name))


@pytest.mark.parametrize("name", sorted(NC.ANSWERS))
def test_answers_known_by_construction(name):
    _, count, keep = _run(name)
    want, _ = NC.ANSWERS[name]
    assert [keep[b, :int(count[b])].tolist() for b in range(len(want))] == want


@HALF
@pytest.mark.parametrize("name", NC.HALF_CASES)
def test_half_features_against_the_oracle_of_the_upcast_values(name, dtype):
    NC.check(f"{dtype} {name}", *_run(name, dtype), NC.oracle(name, dtype))


@pytest.mark.parametrize("name", NAMES)
def test_pred_front_end(name):
    """The same cases through `pred`, decoded as the reference's _inference does: within the bar of the oracle on that prediction, its scores
    copied bit for bit, and the same kept set as the maps front end."""
    from mga_yolo_amd import detect_postprocess
    c = NC.load(name)
    k = dict(c["kw"])
    strides = k.pop("strides")
    pred = NC.ref_decode(c["feats"], strides, k["nc"])
    dets, count, keep = detect_postprocess(pred.cuda(), **k)
    NC.check(f"pred {name}", dets, count, keep, NC.oracle(name, front="pred"))
    md, mc, mk = _run(name)
    assert torch.equal(count, mc) and torch.equal(keep, mk) and torch.equal(dets[..., 5], md[..., 5])
    dets, keep = dets.cpu(), keep.cpu().long()
    for b in range(c["B"]):
        n = int(count[b])
        assert torch.equal(dets[b, :n, 4], pred[b, 4 + dets[b, :n, 5].long(), keep[b, :n]])


@HALF
@pytest.mark.parametrize("name,over", NC.PRED_HALF_CASES, ids=NC.PRED_HALF_IDS)
def test_pred_front_end_in_half(name, over, dtype):
    """k_nms_cand<half> and <bf16> on a prediction rounded to that type: held to the oracle on the upcast prediction, the scores bit-equal
    to the upcast input.  In `wide` the scores tie by the hundreds, and the other tie order keeps other rows; under the cut at max_nms 700 the
    select in the workspace cuts inside equal scores (tests/test_nms_oracle.py asserts both of the inputs)."""
    from mga_yolo_amd import detect_postprocess
    pred, k, o = NC.pred_half(name, dtype, **over)
    dets, count, keep = detect_postprocess(pred.cuda(), **k)
    NC.check(f"pred {dtype} {name} {over}", dets, count, keep, o)
    dets, keep, up = dets.cpu(), keep.cpu().long(), pred.float()
    for b in range(pred.shape[0]):
        n = int(count[b])
        assert torch.equal(dets[b, :n, 4], up[b, 4 + dets[b, :n, 5].long(), keep[b, :n]])


@pytest.mark.parametrize("max_nms", NC.SELECT_CUTS)
def test_select_at_every_cut(max_nms):
    """nms_select on the workspace path: 1344 candidates an image cut at 1, around kNmsLds, and one short of their number (1344: no select)"""
    from mga_yolo_amd import detect_postprocess
    feats, k, o = NC.select_case(max_nms)
    NC.check(f"select {max_nms}", *detect_postprocess([f.cuda() for f in feats], **k), o)


@pytest.mark.parametrize("name", NC.PARITY)
def test_non_max_suppression_against_the_stored_reference_lists(name):
    from mga_yolo_amd import non_max_suppression
    c = NC.load(name)
    k = {x: v for x, v in c["kw"].items() if x not in ("nc", "strides")}
    pred = NC.ref_decode(c["feats"], c["kw"]["strides"], c["kw"]["nc"]).cuda()
    out, idx = non_max_suppression((pred, None), **k, return_idxs=True)
    assert isinstance(out, list) and len(out) == c["B"]
    terms = NC.oracle(name, front="pred")["terms"]
    for b in range(c["B"]):
        n = c["ref32"][b].shape[0]
        assert tuple(out[b].shape) == (n, 6) and idx[b].tolist() == c["ref_keep"][b].tolist()
        got = out[b].cpu().numpy()
        assert np.array_equal(got[:, 5], c["ref64"][b][:, 5])
        if n:
            # the reference's fp64 run writes its xyxy coordinates in fp32 (ops.empty_like): half an eps of the coordinate on top of the bar
            r = O.ratio(got[:, :5], c["ref64"][b][:, :5], terms[b, :n, :5])
            print(f"nms {name}[{b}]: {r:.3f}")
            assert r <= O.K + 0.5


def _plan(names, **over):
    from mga_yolo_amd import DetPostPlan
    c = NC.load(names[0])
    shapes = [(c["B"],) + tuple(f.shape[2:]) for f in c["feats"]]
    k = dict(c["kw"], **over)
    return DetPostPlan.create(shapes, k.pop("nc"), **k)


def _load(plan, name):
    for dst, f in zip(plan.feats, NC.load(name)["feats"]):
        dst.copy_(f)


def _quiet(name):
    """the case's features with every class logit at -20: no candidate anywhere"""
    feats = [f.clone() for f in NC.load(name)["feats"]]
    for f in feats:
        f[:, 64:] = -20.0
    return feats


SAME_SHAPE = ("basic", "empty_all", "empty", "basic")          # B 2, 64^2, nc 1, the default arguments


def test_plan_captured_once_replays_on_fresh_features():
    plan = _plan(SAME_SHAPE)
    _load(plan, "empty")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run()
    for name in SAME_SHAPE:
        _load(plan, name)
        graph.replay()
        torch.cuda.synchronize()
        plan.check_status()
        eager = _run(name)
        for got, want in zip((plan.dets, plan.count, plan.keep), eager):
            assert torch.equal(got, want), name
        NC.check(f"replay {name}", plan.dets, plan.count, plan.keep, NC.oracle(name))


def test_consecutive_calls_on_the_same_buffers_leave_nothing_stale():
    plan = _plan(SAME_SHAPE)
    for name in SAME_SHAPE:
        _load(plan, name)
        plan.run()
        plan.check_status()
        NC.check(f"call {name}", plan.dets, plan.count, plan.keep, NC.oracle(name))
    o = NC.oracle("empty_all")
    assert not o["dets"].any() and (o["keep"] == -1).all()


def test_overflow_poisons_its_image_and_no_other():
    o = NC.oracle("basic")
    b = int(np.argmax(o["n_cand"]))
    cap = o["n_cand"][b] - 1
    assert all(n <= cap for i, n in enumerate(o["n_cand"]) if i != b)
    plan = _plan(SAME_SHAPE, cand_cap=cap)
    _load(plan, "basic")
    plan.run()
    assert int(plan.status) == 1 and int(plan.count[b]) == -1
    assert torch.isnan(plan.dets[b]).all() and (plan.keep[b] == -1).all()
    with pytest.raises(RuntimeError):
        plan.check_status()
    for i in range(2):
        if i != b:
            n = int(o["count"][i])
            assert int(plan.count[i]) == n and np.array_equal(plan.keep[i].cpu().numpy(), o["keep"][i])
            assert O.ratio(plan.dets[i].cpu().numpy()[:, :5], o["dets"][i][:, :5], o["terms"][i][:, :5]) <= O.K
    _load(plan, "empty")                                         # the next call on the same buffers: the list that overflowed starts empty
    plan.run()
    plan.check_status()
    NC.check("after the overflow", plan.dets, plan.count, plan.keep, NC.oracle("empty"))


def _is_empty(plan):
    return not plan.dets.any() and not plan.count.any() and bool((plan.keep == -1).all())


def test_plan_replayed_across_the_paths():
    """one plan of ml_wide's shape captured once and replayed on a list past kNmsLds (the workspace), an empty one, and the long one again on
    the same buffers: each replay byte-equal to the eager call, the empty one all zeros and -1"""
    from mga_yolo_amd import detect_postprocess
    c, o = NC.load("ml_wide"), NC.oracle("ml_wide")
    assert all(n > NC.LDS for n in o["n_cand"])
    plan = _plan(("ml_wide",))
    quiet = _quiet("ml_wide")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run()
    for what, feats in (("long", c["feats"]), ("empty", quiet), ("long again", c["feats"])):
        for dst, f in zip(plan.feats, feats):
            dst.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        plan.check_status()
        eager = detect_postprocess([f.cuda() for f in feats], **c["kw"])
        for got, want in zip((plan.dets, plan.count, plan.keep), eager):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8)), what
        if what == "empty":
            assert _is_empty(plan)
        else:
            NC.check(f"replay {what}", plan.dets, plan.count, plan.keep, o)


def test_multi_label_overflow_inside_an_anchor_s_classes():
    """cand_cap one short of the fuller image's candidates: the list is crossed by the last class of an anchor that has 44 or more, that
    image is poisoned and no other; the next call on the same buffers is clean; at cand_cap = the candidates nothing overflows"""
    o = NC.oracle("ml_wide")
    b = int(np.argmax(o["n_cand"]))
    cap = o["n_cand"][b] - 1
    assert all(n <= cap for i, n in enumerate(o["n_cand"]) if i != b)
    plan = _plan(("ml_wide",), cand_cap=cap)
    _load(plan, "ml_wide")
    plan.run()
    assert int(plan.status) == 1 and int(plan.count[b]) == -1
    assert torch.isnan(plan.dets[b]).all() and (plan.keep[b] == -1).all()
    with pytest.raises(RuntimeError):
        plan.check_status()
    for i in range(2):
        if i != b:
            assert int(plan.count[i]) == int(o["count"][i]) and np.array_equal(plan.keep[i].cpu().numpy(), o["keep"][i])
            assert np.array_equal(plan.dets[i, :, 5].cpu().numpy(), o["dets"][i][:, 5])
            assert O.ratio(plan.dets[i].cpu().numpy()[:, :5], o["dets"][i][:, :5], o["terms"][i][:, :5]) <= O.K
    for dst, f in zip(plan.feats, _quiet("ml_wide")):           # the next call on the same buffers: the list that overflowed starts empty
        dst.copy_(f)
    plan.run()
    plan.check_status()
    assert _is_empty(plan)
    plan = _plan(("ml_wide",), cand_cap=max(o["n_cand"]))
    _load(plan, "ml_wide")
    plan.run()
    plan.check_status()
    NC.check("cand_cap at the candidates", plan.dets, plan.count, plan.keep, o)
