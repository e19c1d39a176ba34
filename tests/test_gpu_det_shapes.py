"""The detection criterion on the device past the sizes of the six stored cases (tests/det_cases.py): boxes over two and three chunks of
k_det_assign with picks in every chunk, zero-metric picks that must survive the carry, 300 interleaved label rows at several m_cap (the second
256-row pass, up to 4096 entries in k_det_resolve), 260 partials in k_det_final, 1 / 2 / 4 levels, topk 1 and 16, classes outside
0 .. nc - 1.  Element-wise against the fp64 oracle and the reference's recorded fp64 run at the bars of det_cases.K."""
import numpy as np
import pytest
import torch

import det_cases as DC
import det_oracle as O
from test_gpu_det import EPS, UP1, _fresh, _run

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def cases():
    """name -> the loaded case with its fp64 oracle, computed once and never written to."""
    memo = {}

    def get(name):
        if name not in memo:
            c = DC.load(name)
            c["oracle"] = O.oracle(c["feats"], *c["labels"], **c["kw"])
            memo[name] = c
        return memo[name]
    return get


def _check_assignment(asg, o, want_scores):
    O.check("target_scores", asg["target_scores"], want_scores, o["terms"]["target_scores"], EPS[F32], DC.K["target_scores"])
    w = o["weight"] > 0
    assert torch.equal(asg["fg"].cpu()[w], o["fg"][w]) and bool(o["fg"][w].all())
    assert torch.equal(asg["target_gt"].cpu()[w], o["target_gt"][w])
    assert torch.allclose(asg["target_bboxes"].cpu()[w].double(), o["target_bboxes"][w], rtol=0, atol=1e-3)
    assert torch.equal(asg["weight"].cpu() > 0, w) and int(asg["status"]) == 0


def _check_against(o, c, loss, items, gs, up, eps_g, want_loss=None, want_items=None):
    B = c["B"]
    O.check("loss", loss, o["loss"] if want_loss is None else want_loss, o["terms"]["loss"], EPS[F32], DC.K["loss"])
    O.check("items", items, o["items"] if want_items is None else want_items, o["terms"]["loss"] / B, EPS[F32], DC.K["loss"])
    for l, g in enumerate(gs):
        O.check(f"g{tuple(up)}[{l}]", g, O.grads(o, l, up), O.grad_terms(o["terms"], l, up), eps_g, DC.K["grad"])


@pytest.mark.parametrize("name", list(DC.CASES))
def test_fp32_against_the_record_and_the_oracle(built_lib, cases, name):
    """Loss, items and target scores against the reference's recorded fp64 run, the gradients against the oracle (held equal to the
    reference's on these inputs when the record was made), every element of every image."""
    c = cases(name)
    o = c["oracle"]
    for up in (UP1, DC.UPSTREAM):
        loss, items, asg, gs = _run(c["feats"], c["labels"], c["kw"], up)
        _check_against(o, c, loss, items, gs, up, EPS[F32], c["loss_f64"], c["items_f64"])
    _check_assignment(asg, o, c["target_scores_f64"])
    w = o["weight"] > 0
    assert torch.equal(asg["fg"].cpu()[w], torch.from_numpy(c["fg_mask_f64"])[w])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("name", DC.HALF_CASES)
def test_half_features_against_the_oracle_on_the_upcast_values(built_lib, cases, name, dtype):
    c = cases(name)
    feats = [f.to(dtype).float() for f in c["feats"]]
    o = O.oracle(feats, *c["labels"], **c["kw"])
    loss, items, asg, gs = _run(feats, c["labels"], c["kw"], DC.UPSTREAM, dtype=dtype)
    assert all(g.dtype == dtype for g in gs) and loss.dtype == F32
    _check_against(o, c, loss, items, gs, DC.UPSTREAM, EPS[dtype])
    _check_assignment(asg, o, o["target_scores"])


def test_zero_metric_picks_survive_the_carry(built_lib, cases):
    """chunk_zero: the foreground mask and the assigned row at EVERY anchor, those of weight 0 included: the zero-metric picks are the lowest
    anchor indices, taken in chunk 0 and carried past the positive picks of chunk 1."""
    c = cases("chunk_zero")
    o = c["oracle"]
    _, _, asg, _ = _run(c["feats"], c["labels"], c["kw"], UP1)
    assert torch.equal(asg["fg"].cpu(), o["fg"]) and torch.equal(asg["target_gt"].cpu(), o["target_gt"])
    assert int((o["fg"] & (o["weight"] == 0)).sum()) > 0 and int((o["weight"] > 0).sum()) > 0


def _same_bits(a, b, assignment=True):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
    if assignment:
        for k in ("fg", "target_gt", "target_scores", "target_bboxes", "weight"):
            assert torch.equal(a[2][k], b[2][k]), k


def test_crowd_at_several_m_cap(built_lib, cases):
    c = cases("crowd")
    o = c["oracle"]
    runs = [_run(c["feats"], c["labels"], c["kw"], DC.UPSTREAM, m_cap=m) for m in (None, 128, 256)]
    for loss, items, asg, gs in runs:
        assert int(asg["status"]) == 0
        _check_against(o, c, loss, items, gs, DC.UPSTREAM, EPS[F32], c["loss_f64"], c["items_f64"])
        _check_assignment(asg, o, c["target_scores_f64"])
        for k in ("fg", "target_gt", "target_scores", "target_bboxes", "weight"):
            assert torch.equal(asg[k], runs[0][2][k]), k
    most = int(np.bincount(c["labels"][0].numpy().astype(np.int64)).max())
    loss, items, asg, gs = _run(c["feats"], c["labels"], c["kw"], DC.UPSTREAM, m_cap=most - 1)
    assert int(asg["status"]) == 1
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(items).all()) and all(bool(torch.isnan(g).all()) for g in gs)


def test_plan_replays_crowd_with_other_label_counts(built_lib, cases):
    """One capture at n_cap = 320, m_cap = 128, replayed with 300, 200, 0, 257 and 300 live rows: each replay is the eager call on the first
    n rows, bit for bit; the rows past n stay in the buffers."""
    from mga_yolo_amd import DetLossPlan
    c = cases("crowd")
    bidx, cls, bb = c["labels"]
    kw = c["kw"]
    up = torch.tensor(DC.UPSTREAM, dtype=F32).cuda()
    plan = DetLossPlan.create([(f.shape[0], f.shape[2], f.shape[3]) for f in c["feats"]], kw["nc"], n_cap=320, m_cap=128, dtype=F32, g_out=up,
                              strides=kw["strides"], gains=kw["gains"], topk=kw["topk"])
    plan.set_labels(bidx.cuda(), cls.cuda(), bb.cuda())

    def step():
        plan.forward(); plan.backward()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    seen = []
    for t, n in enumerate((300, 200, 0, 257, 300)):
        feats = c["feats"] if t in (0, 4) else _fresh(c, 60 + t)
        for dst, f in zip(plan.feats, feats):
            dst.copy_(f)
        plan.n.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        plan.check_status()
        want = _run(feats, (bidx[:n], cls[:n], bb[:n]), kw, DC.UPSTREAM, m_cap=128)
        assert torch.equal(plan.out, want[0]) and torch.equal(plan.items, want[1]), n
        assert all(torch.equal(x, y) for x, y in zip(plan.g_feats, want[3])), n
        assert torch.equal(plan.assign_gt.long(), want[2]["target_gt"]) and torch.equal(plan.assign_score, want[2]["weight"]), n
        seen.append(plan.out.clone())
    assert torch.equal(seen[0], seen[4]) and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[3])
    assert float(seen[2][0]) == 0.0 and float(seen[2][2]) == 0.0 and float(seen[2][1]) > 0.0
    assert torch.equal(plan.batch_idx[:300].cpu(), bidx)         # the stale rows were there to be read


def test_classes_outside_the_range_are_clamped(built_lib):
    c = O.load_case("b2_64_nc3")
    bidx, cls, bb = c["labels"]
    nc = c["kw"]["nc"]
    wild, tame = cls.clone(), cls.clone()
    wild[3], wild[0] = nc + 3, -2                                # stored: class 0 and class nc - 1
    tame[3], tame[0] = nc - 1, 0
    assert not torch.equal(tame, cls)                            # the clamped labels are another input than the stored one
    a = _run(c["feats"], (bidx, wild, bb), c["kw"], tuple(c["upstream"]))
    b = _run(c["feats"], (bidx, tame, bb), c["kw"], tuple(c["upstream"]))
    _same_bits(a, b)
    assert bool(torch.isfinite(a[0]).all()) and int(a[2]["status"]) == 0
    plain = _run(c["feats"], c["labels"], c["kw"], tuple(c["upstream"]))
    assert not torch.equal(plain[0], a[0])


@pytest.mark.parametrize("name", ["chunk3", "crowd"])
def test_two_runs_give_the_same_bits(built_lib, cases, name):
    c = cases(name)
    _same_bits(_run(c["feats"], c["labels"], c["kw"], DC.UPSTREAM), _run(c["feats"], c["labels"], c["kw"], DC.UPSTREAM))
