"""The detection matching on the device (include/ext/mgamatch.h, csrc/match.cuh) against tests/match_oracle.py on every case of
tests/match_cases.py.  tp and best_gt are exactly the oracle's (which, on the cases of MC.PARITY, is the reference validator's own stored
answer); best_iou lies within K eps_fp32 term of the fp64 oracle, K = twice the largest ratio of the reference's own fp32 box_iou over the cases
(tests/golden/match_ratios.json: 0.61, so K = 1.22), not below 1.  Then the plan: fed by a DetPostPlan inside one captured graph, its status
words, and its accumulation.  tests/match_cases.py says which case runs which path of the kernels."""
import json
import os

import numpy as np
import pytest
import torch

import match_cases as MC
import match_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
RATIOS = json.load(open(os.path.join(GOLDEN, "match_ratios.json")))
K = max(2 * RATIOS["worst"], 1.0)
_ORACLES = {}


def _case(name):
    """the case, its record and its oracle: computed once, shared, left unchanged"""
    if name not in _ORACLES:
        c, z = MC.load(name)
        _ORACLES[name] = (c, z, MC.oracle(name, c))
    return _ORACLES[name]


def _check(what, tp, best_iou, best_gt, o):
    tp, best_iou, best_gt = tp.cpu().numpy(), best_iou.cpu().numpy(), best_gt.cpu().numpy()
    r = O.ratio(best_iou, o["best_iou"], o["term"])
    print(f"{what}: true {int(tp.sum())}, best_iou ratio {r:.3f} (bar {K:.3f})")
    assert np.array_equal(tp != 0, o["tp"]), what
    assert np.array_equal(best_gt, o["best_gt"]), what
    assert r <= K, what


@pytest.mark.parametrize("name", MC.NAMES)
def test_every_case_through_match_detections(name):
    from mga_yolo_amd import match_detections
    c, z, o = _case(name)
    tp, best_iou, best_gt = match_detections(*MC.tensors(MC.live(c), "cuda"), imgsz=c["hw"], iouv=c["iouv"], single_cls=c["single_cls"])
    assert tp.dtype == torch.bool and best_iou.dtype == torch.float32 and best_gt.dtype == torch.int32
    _check(name, tp, best_iou, best_gt, o)
    if name in MC.PARITY:                                          # and bit for bit the reference's own fp32 box_iou: the same operations in the same order
        assert np.array_equal(tp.cpu().numpy(), z["ref_tp"])
        assert np.array_equal(best_iou.cpu().numpy(), z["ref_best_iou_f32"])
    if name in MC.ANSWERS:
        k = len(MC.ANSWERS[name]["tp"])
        assert tp[0, :k].tolist() == MC.ANSWERS[name]["tp"] and best_gt[0, :k].tolist() == MC.ANSWERS[name]["best_gt"]


def _plan(c, acc=True, m_cap=None, rows_cap=None, tgt_cap=None, garbage=True):
    """a plan on a case's own tensors: every label row in the static buffers, the n word at the case's"""
    from mga_yolo_amd import DetMatchPlan
    dets, count, bi, cl, bx = MC.tensors(c if garbage else MC.live(c), "cuda")
    B, D = dets.shape[:2]
    n_live = int((bi[:c["n"]] < B).sum()) if c["n"] is not None else int(((bi >= 0) & (bi < B)).sum())
    total = int(count.clamp(0, D).sum())
    plan = DetMatchPlan.create(B, D, n_cap=bi.numel(), m_cap=m_cap or c["m_cap"], imgsz=c["hw"], iouv=c["iouv"], single_cls=c["single_cls"],
                               rows_cap=(rows_cap if rows_cap is not None else 2 * total + 1) if acc else None,
                               tgt_cap=(tgt_cap if tgt_cap is not None else 2 * n_live + 1) if acc else None, dets=dets, count=count)
    plan.set_labels(bi, cl, bx)
    if c["n"] is not None and garbage:
        plan.n.fill_(c["n"])
    return plan, total, n_live


def test_the_n_word_hides_the_rows_behind_it():
    c, _, o = _case("nword")
    assert c["n"] < len(c["batch_idx"])
    plan, total, n_live = _plan(c)
    plan.run()
    plan.check_status()
    _check("nword through the plan", plan.tp, plan.best_iou, plan.best_gt, o)
    assert plan.state.tolist() == [total, n_live, len(c["count"]), 0]
    plan, _, _ = _plan(c, acc=False, m_cap=8)
    plan.n.fill_(len(c["batch_idx"]))                              # with the word at n_cap the rows behind it take part, and change the answer
    plan.run()
    every = O.oracle(c["dets"], c["count"], c["batch_idx"], c["cls"], c["bboxes"], c["hw"], c["iouv"])
    assert not np.array_equal(every["best_gt"], o["best_gt"])
    _check("nword, every row", plan.tp, plan.best_iou, plan.best_gt, every)
    plan.n.fill_(10 ** 6)                                          # clamped to n_cap
    plan.run()
    _check("nword, the word past n_cap", plan.tp, plan.best_iou, plan.best_gt, every)
    plan.n.fill_(-3)                                               # clamped to 0: no labels
    plan.run()
    assert not plan.tp.any() and (plan.best_gt == -1).all() and not plan.best_iou.any()


def _feats(B, nc, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h in (8, 4):
        f = 0.5 * torch.randn(B, 64 + nc, h, h, generator=g)
        f[:, 64:] = -4 + 4.5 * torch.rand(B, nc, h, h, generator=g)
        out.append(f)
    return out


def test_plan_behind_a_post_process_in_one_captured_graph():
    """forward's maps -> DetPostPlan.run -> DetMatchPlan.run as one captured chain on a two-level 64 x 64 input; three replays with fresh
    features and 5, 0 and 9 label rows.  The labels are jittered copies of rows the post-process keeps, so there is something to match.
    stats() against the host path on the rows the device's post-process wrote."""
    from mga_yolo_amd import DetMatchPlan, DetPostPlan
    from mga_yolo_amd.detmatch import host_stats
    B, nc, D = 3, 2, 24
    post = DetPostPlan.create([(B, 8, 8), (B, 4, 4)], nc, strides=(8, 16), conf_thres=0.3, iou_thres=0.5, max_det=D, multi_label=True)
    match = DetMatchPlan.create(B, D, n_cap=16, m_cap=8, imgsz=64, rows_cap=3 * B * D, tgt_cap=32, dets=post.dets, count=post.count)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        post.run(); match.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        post.run(); match.run()
    match.reset()
    batches, rs = [], np.random.RandomState(3)
    for r, n_lab in enumerate((5, 0, 9)):
        for dst, src in zip(post.feats, _feats(B, nc, 50 + r)):
            dst.copy_(src)
        post.run()                                                 # eagerly, to draw this replay's labels from its rows
        dets, count = post.dets.cpu(), post.count.cpu()
        assert int(count.min()) > 0
        bi = torch.from_numpy(rs.randint(0, B, n_lab).astype(np.float32))
        rows = [dets[int(b), rs.randint(int(count[int(b)]))] for b in bi]
        bx = torch.stack([torch.stack(((q[0] + q[2]) / 2, (q[1] + q[3]) / 2, (q[2] - q[0]) * (1 + 0.2 * rs.uniform(-1, 1)), q[3] - q[1])) / 64
                          for q in rows]) if n_lab else torch.zeros(0, 4)
        cl = torch.stack([q[5] for q in rows]).reshape(-1, 1) if n_lab else torch.zeros(0, 1)
        match.set_labels(bi.cuda(), cl.cuda(), bx.cuda())
        graph.replay()
        torch.cuda.synchronize()
        post.check_status(); match.check_status()
        assert torch.equal(post.dets.cpu(), dets) and torch.equal(post.count.cpu(), count)
        batches.append((dets, count, bi, cl, bx))
    got, want = match.stats(), host_stats(batches, imgsz=64)
    assert got["seen"] == want["seen"] == 3 * B == match.seen
    assert want["tp"].any() and not want["tp"].all() and want["tp"].shape[0] == sum(int(b[1].sum()) for b in batches)
    for k in ("tp", "conf", "pred_cls", "target_cls", "target_img"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def test_status_1_an_image_over_m_cap():
    c, _, o = _case("basic")
    per = np.bincount(c["batch_idx"][c["batch_idx"] < 3].astype(int), minlength=3)
    over = per > 2
    assert over.any() and not over.all()
    plan, total, n_live = _plan(c, m_cap=2)
    plan.run()
    assert plan.status.item() == 1 and plan.state.tolist() == [0, 0, 0, 0]                # nothing appended for the whole call
    with pytest.raises(RuntimeError, match="m_cap"):
        plan.check_status()
    tp, iou, gt = plan.tp.cpu().numpy(), plan.best_iou.cpu().numpy(), plan.best_gt.cpu().numpy()
    for b in range(3):
        if over[b]:
            assert not tp[b].any() and np.isnan(iou[b]).all() and (gt[b] == -1).all()
        else:                                                      # the other images are answered
            assert np.array_equal(tp[b] != 0, o["tp"][b]) and np.array_equal(gt[b], o["best_gt"][b])


def test_the_n_word_inside_the_second_staging_chunk():
    """`chunks` through a plan of five label workgroups with the word on the chunk boundary, one behind it and six behind it: the answer and
    the accumulated rows are those of the rows before the word"""
    from mga_yolo_amd.detmatch import host_stats
    c, _, _ = _case("chunks")
    assert len(c["batch_idx"]) > 4 * 256 and c["n"] is None
    plan, total, _ = _plan(c)
    B = len(c["count"])
    for n in MC.N_WORDS:
        cut = dict(c, n=n)
        plan.reset()
        plan.n.fill_(n)
        plan.run()
        plan.check_status()
        _check(f"chunks, n = {n}", plan.tp, plan.best_iou, plan.best_gt, MC.oracle("chunks", cut))
        n_live = int((c["batch_idx"][:n] < B).sum())
        assert plan.state.tolist() == [total, n_live, B, 0]
        got, want = plan.stats(), host_stats([MC.tensors(MC.live(cut))], imgsz=c["hw"], iouv=c["iouv"])
        assert got["seen"] == want["seen"] == B and got["target_cls"].shape == (n_live,)
        for k in ("tp", "conf", "pred_cls", "target_cls", "target_img"):
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (n, k)


def test_status_1_decided_by_rows_of_the_second_staging_chunk():
    c, _, o = _case("chunks")
    B = len(c["count"])
    per = np.bincount(c["batch_idx"][c["batch_idx"] < B].astype(int), minlength=B)
    b = int(np.argmax(per))
    m_cap = int(per[b]) - 1
    assert (np.delete(per, b) <= m_cap).all() and int((c["batch_idx"][:MC.STAGE] == b).sum()) <= m_cap    # the first chunk alone fits
    plan, _, _ = _plan(c, m_cap=m_cap)
    plan.run()
    assert plan.status.item() == 1 and plan.state.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="m_cap"):
        plan.check_status()
    tp, iou, gt = plan.tp.cpu().numpy(), plan.best_iou.cpu().numpy(), plan.best_gt.cpu().numpy()
    for i in range(B):
        if i == b:
            assert not tp[i].any() and np.isnan(iou[i]).all() and (gt[i] == -1).all()
        else:
            assert np.array_equal(tp[i] != 0, o["tp"][i]) and np.array_equal(gt[i], o["best_gt"][i])
            assert O.ratio(iou[i], o["best_iou"][i], o["term"][i]) <= K


def test_status_2_rows_cap_one_short_appends_nothing():
    c, _, o = _case("basic")
    _, total, n_live = _plan(c, acc=False)
    for rows_cap, tgt_cap in ((2 * total - 1, 2 * n_live), (2 * total, 2 * n_live - 1)):
        plan, _, _ = _plan(c, rows_cap=rows_cap, tgt_cap=tgt_cap)
        plan.run()
        plan.check_status()
        before, state = plan._arena.clone(), plan.state.tolist()
        assert state == [total, n_live, 3, 0]
        plan.run()                                                 # the second batch does not fit
        assert plan.status.item() == 2
        with pytest.raises(RuntimeError, match="rows_cap"):
            plan.check_status()
        assert torch.equal(plan._arena, before) and plan.state.tolist() == state
        _check("status 2", plan.tp, plan.best_iou, plan.best_gt, o)                       # tp is written all the same
    plan, _, _ = _plan(c, rows_cap=2 * total, tgt_cap=2 * n_live)                         # exactly enough for two
    plan.run(); plan.run()
    assert plan.status.item() == 0 and plan.state.tolist() == [2 * total, 2 * n_live, 6, 0]
    s = plan.stats()
    assert s["tp"].shape == (2 * total, 10) and np.array_equal(s["tp"][:total], s["tp"][total:]) and s["target_cls"].shape == (2 * n_live,)


@pytest.mark.parametrize("name", ["basic", "wide", "labels256", "chunks", "dets600"])
def test_two_runs_give_the_same_bytes(name):
    c, _, _ = _case(name)
    outs = []
    for _ in range(2):
        plan, _, _ = _plan(c)
        plan.run()
        outs.append([t.clone() for t in (plan.tp, plan.best_iou, plan.best_gt, plan.status, plan._arena)])
        plan.run()                                                 # and a second batch behind the first
        outs[-1].append(plan._arena.clone())
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs))


def test_an_iou_on_the_threshold_counts():
    """50 / (100 + 50 - 50 + 1e-7) is 0.5 exactly in fp32: `>=` holds, and no product is contracted into the sums"""
    from mga_yolo_amd import match_detections
    dets = torch.tensor([[[0., 0., 10., 5., 0.9, 0.]]], device="cuda")
    tp, best, gt = match_detections(dets, torch.tensor([1], dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda"),
                                    torch.zeros(1, 1, device="cuda"), torch.tensor([[5 / 64, 5 / 64, 10 / 64, 10 / 64]], device="cuda"),
                                    imgsz=64, iouv=[0.5, 0.55])
    assert tp.tolist() == [[[True, False]]] and best.item() == 0.5 and gt.item() == 0


def test_count_and_labels_on_the_host_are_moved_to_the_detections_device():
    from mga_yolo_amd import match_detections
    c, _, o = _case("basic")
    dets, count, bi, cl, bx = MC.tensors(c)
    _check("host count", *match_detections(dets.cuda(), count, bi, cl, bx, imgsz=c["hw"], iouv=c["iouv"]), o)
    _check("int64 count", *match_detections(dets.cuda(), count.long().cuda(), bi.cuda(), cl, bx.cuda(), imgsz=c["hw"], iouv=c["iouv"]), o)


def test_a_plan_without_accumulation_says_so():
    c, _, _ = _case("steal")
    plan, _, _ = _plan(c, acc=False)
    for ask in (plan.reset, plan.stats, lambda: plan.seen):
        with pytest.raises(RuntimeError, match="no accumulation"):
            ask()


def _validator(c, original=None):
    """a stand-in validator class with detmatch.update_metrics bound as install(match=True) binds it, and the case as its loop takes it"""
    import types
    from mga_yolo_amd import detmatch
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])

    class V:
        update_metrics = detmatch.update_metrics
        seen = 0

        def _prepare_pred(self, pred):
            return pred

        def _process_batch(self, preds, batch):
            raise AssertionError("the replacement never calls it")
        _prepare_batch = match_predictions = _process_batch
    v = V()
    v.iouv = torch.from_numpy(np.asarray(c["iouv"])).cuda()
    v.args = types.SimpleNamespace(single_cls=False, plots=False, visualize=False, save_json=False, save_txt=False)
    v.metrics = types.SimpleNamespace(stats=stats, update_stats=lambda s: [stats[k].append(x) for k, x in s.items()])
    if original is not None:
        detmatch._ORIGINALS[V] = original
    dets, count, bi, cl, bx = MC.tensors(MC.live(c), "cuda")
    B, D = dets.shape[:2]
    preds = [dict(bboxes=dets[b, :max(int(count[b]), 0), :4].clone(), conf=dets[b, :max(int(count[b]), 0), 4].clone(),
                  cls=dets[b, :max(int(count[b]), 0), 5].clone()) for b in range(B)]
    return v, preds, dict(batch_idx=bi, cls=cl, bboxes=bx, img=torch.empty(B, 0, *c["hw"], device="cuda"))


@pytest.mark.parametrize("name", ["basic", "empty"])
def test_replacement_update_metrics_on_the_device_leaves_the_reference_s_lists(name):
    c, z, _ = _case(name)
    v, preds, batch = _validator(c)
    v.update_metrics(preds, batch)
    assert v.seen == len(preds)
    for key, lst in v.metrics.stats.items():
        for b, got in enumerate(lst):
            want = z[f"stats_{key}_{b}"]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (key, b)


def test_replacement_update_metrics_hands_an_image_over_256_labels_to_the_reference_s():
    c, _, _ = _case("steal")
    calls = []
    v, preds, batch = _validator(c, original=lambda self, preds, batch: calls.append(len(preds)))
    v.update_metrics(preds, batch)                                 # one label row: the replacement's own
    assert not calls and v.seen == 1
    crowd = dict(batch, batch_idx=torch.zeros(257, device="cuda"), cls=torch.zeros(257, 1, device="cuda"),
                 bboxes=batch["bboxes"][:1].repeat(257, 1))
    v.update_metrics(preds, crowd)
    assert calls == [1] and v.seen == 1                            # nothing was counted before the hand-over
    w, preds, batch = _validator(c)                                # bound by hand, no method to hand over to: a refusal
    with pytest.raises(NotImplementedError, match="256"):
        w.update_metrics(preds, dict(crowd))
