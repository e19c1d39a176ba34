"""The confusion matrix on the device (include/ext/mgaconfusion.h, csrc/confusion.cuh) against tests/confusion_oracle.py on every case of
tests/confusion_cases.py.  Under the cases' guards every comparison is exact equality of integers, on every element of det_out, lab_out
and cm (the oracle, on the cases of CC.PARITY, is the reference's own stored per-image answer).  Then the plan: the n word, its status
words, its accumulation, the captured chain behind a post-process and a matching, and the replacement update_metrics with the switch on.
tests/confusion_cases.py says which case runs which path of the kernels."""
import types

import numpy as np
import pytest
import torch

import confusion_cases as CC
import confusion_oracle as CO

pytestmark = pytest.mark.gpu
_ORACLES = {}


def _case(name):
    """the case, its record and its oracle: computed once, shared, left unchanged"""
    if name not in _ORACLES:
        c, z = CC.load(name)
        _ORACLES[name] = (c, z, CC.oracle(name, c))
    return _ORACLES[name]


def _oracle(c, **kw):
    return CO.oracle(c["dets"], c["count"], c["batch_idx"], c["cls"], c["bboxes"], c["hw"], c["nc"], CC.conf_thres(c), c["iou_thres"],
                     single_cls=c["single_cls"], n=c["n"], round32=c["construct"], **kw)


def _check(what, cm, det_out, lab_out, o, n=None):
    cm, det_out, lab_out = cm.cpu().numpy(), det_out.cpu().numpy(), lab_out.cpu().numpy()
    print(f"{what}: {int(cm.sum())} counts, {int((det_out >= 0).sum())} counted detections")
    assert np.array_equal(det_out, o["det_out"]), what
    assert np.array_equal(lab_out, o["lab_out"][:n]), what
    assert np.array_equal(cm, o["cm"]), what


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_case_through_confusion_matrix(name):
    from mga_yolo_amd import confusion_matrix
    c, z, o = _case(name)
    lv = CC.live(c)
    cm, det_out, lab_out = confusion_matrix(*CC.tensors(lv, "cuda"), nc=c["nc"], imgsz=c["hw"], conf=c["conf"], iou_thres=c["iou_thres"],
                                            single_cls=c["single_cls"])
    assert cm.dtype == torch.int64 and det_out.dtype == torch.int32 and lab_out.dtype == torch.int32 and cm.shape == (c["nc"] + 1, c["nc"] + 1)
    _check(name, cm, det_out, lab_out, o, n=len(lv["batch_idx"]))
    if name in CC.PARITY:
        assert np.array_equal(cm.cpu().numpy(), z["ref_per_image"].sum(0))
    if name in CC.ANSWERS:
        a = CC.ANSWERS[name]
        rows = np.nonzero(c["batch_idx"] == 0)[0]
        assert np.array_equal(cm.cpu().numpy(), CC.answer_matrix(name))
        assert det_out[0].tolist() == a["det_out"] and lab_out.cpu()[rows].tolist() == a["lab_out"]


def _plan(c, m_cap=None, accumulate=True, single_cls=None, garbage=True):
    """a plan on a case's own tensors: every label row in the static buffers, the n word at the case's"""
    from mga_yolo_amd import ConfusionPlan
    dets, count, bi, cl, bx = CC.tensors(c if garbage else CC.live(c), "cuda")
    B, D = dets.shape[:2]
    plan = ConfusionPlan.create(B, D, nc=c["nc"], n_cap=bi.numel(), m_cap=m_cap or c["m_cap"], imgsz=c["hw"], conf=c["conf"],
                                iou_thres=c["iou_thres"], single_cls=c["single_cls"] if single_cls is None else single_cls,
                                accumulate=accumulate, dets=dets, count=count)
    plan.set_labels(bi, cl, bx)
    if c["n"] is not None and garbage:
        plan.n.fill_(c["n"])
    return plan


def test_the_n_word_hides_the_rows_behind_it():
    c, _, o = _case("nword")
    assert c["n"] < len(c["batch_idx"])
    plan = _plan(c)
    plan.run()
    plan.check_status()
    _check("nword through the plan", plan.cm, plan.det_out, plan.lab_out, o)
    assert (plan.lab_out[c["n"]:] == -1).all() and torch.equal(plan.matrix(), plan.cm.cpu().long())
    every = _oracle(dict(c, n=None))
    assert not np.array_equal(every["cm"], o["cm"])                # with the word at n_cap the rows behind it take part, and change the answer
    plan = _plan(c, m_cap=8)
    plan.n.fill_(10 ** 6)                                          # clamped to n_cap
    plan.run()
    _check("nword, the word past n_cap", plan.cm, plan.det_out, plan.lab_out, every)
    plan.n.fill_(-3)                                               # clamped to 0: no labels, every counted detection a false positive
    plan.run()
    none = _oracle(dict(c, n=0))
    _check("nword, no labels", plan.cm, plan.det_out, plan.lab_out, none)
    assert (plan.lab_out == -1).all() and not plan.cm[c["nc"]].any()


def test_the_n_word_inside_the_second_staging_chunk():
    c, _, _ = _case("chunks")
    assert len(c["batch_idx"]) > CC.STAGE + 6 and c["n"] is None
    plan = _plan(c)
    total = np.zeros_like(_case("chunks")[2]["cm"])
    for n in CC.N_WORDS:
        plan.n.fill_(n)
        plan.run()
        plan.check_status()
        o = _oracle(dict(c, n=n))
        _check(f"chunks, n = {n}", plan.cm, plan.det_out, plan.lab_out, o)
        total += o["cm"]
    assert np.array_equal(plan.matrix().numpy(), total)


def _status_leaves_nothing(plan, status, match):
    before = plan.acc.clone()
    plan.run()
    assert plan.status.item() == status and not plan.cm.any() and torch.equal(plan.acc, before)
    with pytest.raises(RuntimeError, match=match):
        plan.check_status()


def test_status_1_an_image_over_m_cap():
    c, _, o = _case("basic")
    per = np.bincount(c["batch_idx"][c["batch_idx"] < 3].astype(int), minlength=3)
    over = per > 2
    assert over.any() and not over.all()
    good = _plan(c)
    good.run()                                                     # something in acc that a refused call must leave
    plan = _plan(c, m_cap=2)
    plan.acc.copy_(good.acc)
    assert plan.acc.any()
    _status_leaves_nothing(plan, 1, "m_cap")
    det_out, lab_out = plan.det_out.cpu().numpy(), plan.lab_out.cpu().numpy()
    for b in range(3):
        rows = np.nonzero(c["batch_idx"] == b)[0]
        if over[b]:
            assert (det_out[b] == -1).all() and (lab_out[rows] == -1).all()
        else:                                                      # the other images are answered
            assert np.array_equal(det_out[b], o["det_out"][b]) and np.array_equal(lab_out[rows], o["lab_out"][rows])


def test_status_1_decided_by_rows_of_the_second_staging_chunk():
    c, _, o = _case("chunks")
    B = len(c["count"])
    per = np.bincount(c["batch_idx"][c["batch_idx"] < B].astype(int), minlength=B)
    b = int(np.argmax(per))
    m_cap = int(per[b]) - 1
    assert (np.delete(per, b) <= m_cap).all() and int((c["batch_idx"][:CC.STAGE] == b).sum()) <= m_cap    # the first chunk alone fits
    plan = _plan(c, m_cap=m_cap)
    plan.acc.fill_(7)
    _status_leaves_nothing(plan, 1, "m_cap")
    det_out, lab_out = plan.det_out.cpu().numpy(), plan.lab_out.cpu().numpy()
    for i in range(B):
        rows = np.nonzero(c["batch_idx"] == i)[0]
        if i == b:
            assert (det_out[i] == -1).all() and (lab_out[rows] == -1).all()
        else:
            assert np.array_equal(det_out[i], o["det_out"][i]) and np.array_equal(lab_out[rows], o["lab_out"][rows])


@pytest.mark.parametrize("where", ["label", "detection"])
def test_status_3_a_class_outside_the_matrix(where):
    c, _, o = _case("basic")
    c = dict(c, dets=c["dets"].copy(), cls=c["cls"].copy())
    if where == "label":
        r = int(np.nonzero(c["batch_idx"] == 1)[0][0])
        c["cls"][r] = c["nc"]                                      # a live label row of an image
    else:
        d = int(np.nonzero(c["dets"][2, :int(c["count"][2]), 4] > 0.25)[0][0])
        c["dets"][2, d, 5] = -1.0                                  # a counted detection
    plan = _plan(c)
    plan.acc.fill_(5)
    _status_leaves_nothing(plan, 3, "class")
    single = _plan(c, single_cls=True)                             # the same inputs with every class taken as 0
    single.run()
    single.check_status()
    _check(f"bad {where} class under single_cls", single.cm, single.det_out, single.lab_out, _oracle(dict(c, single_cls=True)))
    if where == "detection":                                       # a class outside the matrix on a row that is not counted is nobody's business
        c["dets"][2, d, 4] = 0.1
        plan = _plan(c)
        plan.run()
        plan.check_status()
        _check("bad class, not counted", plan.cm, plan.det_out, plan.lab_out, _oracle(c))
    both = _plan(c if where == "label" else dict(c, cls=np.full_like(c["cls"], np.nan)), m_cap=2)
    both.run()
    assert both.status.item() == 1                                 # 1 takes precedence over 3


def _three_batches(c):
    """`basic`, `basic` with its images in reverse order, and `basic` without the label rows at even places"""
    B = len(c["count"])
    rev = dict(c, dets=c["dets"][::-1].copy(), count=c["count"][::-1].copy(),
               batch_idx=np.where(c["batch_idx"] < B, B - 1 - c["batch_idx"], c["batch_idx"]).astype(np.float32))
    odd = dict(c, batch_idx=c["batch_idx"][1::2].copy(), cls=c["cls"][1::2].copy(), bboxes=c["bboxes"][1::2].copy())
    return [c, rev, odd]


def test_plan_accumulates_three_batches_and_resets():
    from mga_yolo_amd import ConfusionPlan
    c, _, _ = _case("basic")
    batches = _three_batches(c)
    B, D = c["dets"].shape[:2]
    runs = []
    for _ in range(2):
        plan = ConfusionPlan.create(B, D, nc=c["nc"], n_cap=len(c["batch_idx"]) + 3, m_cap=8, imgsz=c["hw"], conf=c["conf"])
        snaps, want = [], np.zeros((c["nc"] + 1, c["nc"] + 1), np.int64)
        for k in batches:
            dets, count, bi, cl, bx = CC.tensors(k, "cuda")
            plan.dets.copy_(dets); plan.count.copy_(count)
            plan.set_labels(bi, cl, bx)
            plan.run()
            plan.check_status()
            o = _oracle(k)
            assert not [g for g in o["guards"]]
            n = len(k["batch_idx"])
            _check("a batch of three", plan.cm, plan.det_out, plan.lab_out[:n], o)
            assert (plan.lab_out[n:] == -1).all()
            want += o["cm"]
            snaps += [t.clone() for t in (plan.cm, plan.acc, plan.det_out, plan.lab_out)]
        assert plan.acc.dtype == torch.int64 and np.array_equal(plan.matrix().numpy(), want) and want.sum() > batches[0]["nc"]
        runs.append(snaps)
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*runs))      # two runs: the same bytes
    plan.reset()
    assert not plan.matrix().any()
    plan.run()
    assert np.array_equal(plan.matrix().numpy(), _oracle(batches[-1])["cm"])
    bare = ConfusionPlan.create(B, D, nc=c["nc"], n_cap=4, m_cap=4, imgsz=c["hw"], accumulate=False)
    for ask in (bare.reset, bare.matrix):
        with pytest.raises(RuntimeError, match="no accumulation"):
            ask()


@pytest.mark.parametrize("name", ["labels256", "chunks", "dets600"])
def test_two_runs_give_the_same_bytes(name):
    c, _, _ = _case(name)
    outs = []
    for _ in range(2):
        plan = _plan(c)
        plan.run(); plan.run()
        outs.append([t.clone() for t in (plan.cm, plan.acc, plan.det_out, plan.lab_out, plan.status)])
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs))
    assert torch.equal(outs[0][1], 2 * outs[0][0].long())


def _feats(B, nc, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h in (8, 4):
        f = 0.5 * torch.randn(B, 64 + nc, h, h, generator=g)
        f[:, 64:] = -4 + 4.5 * torch.rand(B, nc, h, h, generator=g)
        out.append(f)
    return out


def test_the_chain_post_match_confusion_in_one_captured_graph():
    """forward's maps -> DetPostPlan.run -> DetMatchPlan.run -> ConfusionPlan.run as one captured chain on a two-level 64 x 64 input; three
    replays with fresh features and 5, 0 and 9 label rows set once through the matching plan.  The labels are jittered copies of rows the
    post-process keeps, every third of another class.  Each replay's matrix against the oracle on the rows the device's post-process wrote."""
    from mga_yolo_amd import ConfusionPlan, DetMatchPlan, DetPostPlan
    B, nc, D = 3, 2, 24
    post = DetPostPlan.create([(B, 8, 8), (B, 4, 4)], nc, strides=(8, 16), conf_thres=0.3, iou_thres=0.5, max_det=D)
    match = DetMatchPlan.create(B, D, n_cap=16, m_cap=8, imgsz=64, dets=post.dets, count=post.count)
    cm = ConfusionPlan.create(B, D, nc=nc, m_cap=8, imgsz=64, conf=0.001, dets=post.dets, count=post.count, labels=match)
    assert cm.batch_idx is match.batch_idx and cm.cls is match.cls and cm.bboxes is match.bboxes and cm.n is match.n
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        post.run(); match.run(); cm.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        post.run(); match.run(); cm.run()
    cm.reset()
    total, rs = np.zeros((nc + 1, nc + 1), np.int64), np.random.RandomState(3)
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
        cl = torch.stack([(q[5] + (i % 3 == 2)) % nc for i, q in enumerate(rows)]).reshape(-1, 1) if n_lab else torch.zeros(0, 1)
        cm.set_labels(bi.cuda(), cl.cuda(), bx.cuda())             # the matching plan's: one call serves both
        match.run()
        tp = match.tp.clone()                                      # the matching alone, before the chain
        graph.replay()
        torch.cuda.synchronize()
        post.check_status(); match.check_status(); cm.check_status()
        assert torch.equal(post.dets.cpu(), dets) and torch.equal(post.count.cpu(), count) and torch.equal(match.tp, tp)
        o = CO.oracle(dets.numpy(), count.numpy(), bi.numpy(), cl.numpy(), bx.numpy(), (64, 64), nc, 0.25, 0.45)
        assert not o["guards"], o["guards"]
        _check(f"replay {r}", cm.cm, cm.det_out, cm.lab_out[:n_lab], o)
        assert (cm.lab_out[n_lab:] == -1).all()
        total += o["cm"]
    assert np.array_equal(cm.matrix().numpy(), total) and np.trace(total[:nc, :nc]) and total[:nc, nc].sum()


def _validator(c, nc=None, matches=None):
    """a stand-in validator class with detmatch.update_metrics bound as install(match=True) binds it, plots on, a ConfusionMatrix stand-in
    whose process_batch counts its calls, and the case as the validator's loop takes it"""
    from mga_yolo_amd import detmatch
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])
    calls = []

    class V:
        update_metrics = detmatch.update_metrics
        seen = 0

        def _prepare_pred(self, pred):
            return pred

        def _prepare_batch(self, si, batch):
            return dict(si=si)

        def _process_batch(self, preds, batch):
            raise AssertionError("the replacement never calls it")
        match_predictions = _process_batch
    v = V()
    v.iouv = torch.linspace(0.5, 0.95, 10).cuda()
    v.args = types.SimpleNamespace(single_cls=False, plots=True, visualize=False, save_json=False, save_txt=False, conf=c["conf"])
    v.metrics = types.SimpleNamespace(stats=stats, update_stats=lambda s: [stats[k].append(x) for k, x in s.items()])
    nc = nc or c["nc"]
    v.confusion_matrix = types.SimpleNamespace(nc=nc, task="detect", matches=matches, matrix=np.zeros((nc + 1, nc + 1)),
                                               process_batch=lambda predn, pbatch, conf: calls.append(pbatch["si"]))
    dets, count, bi, cl, bx = CC.tensors(CC.live(c), "cuda")
    B = dets.shape[0]
    preds = [dict(bboxes=dets[b, :max(int(count[b]), 0), :4].clone(), conf=dets[b, :max(int(count[b]), 0), 4].clone(),
                  cls=dets[b, :max(int(count[b]), 0), 5].clone()) for b in range(B)]
    return v, calls, preds, dict(batch_idx=bi, cls=cl, bboxes=bx, img=torch.empty(B, 0, *c["hw"], device="cuda"))


def _same_lists(a, b):
    return all(len(a[k]) == len(b[k]) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in a)


@pytest.mark.parametrize("name", ["basic", "empty"])
def test_replacement_update_metrics_with_the_switch_on(name):
    from mga_yolo_amd import detmatch, install, uninstall
    c, z, _ = _case(name)
    B = len(c["count"])
    off, calls_off, preds, batch = _validator(c)
    off.update_metrics(preds, batch)                               # the switch off: the per-image calls, the matrix untouched
    assert calls_off == list(range(B)) and not off.confusion_matrix.matrix.any()
    try:
        install(match=True, confusion=True)
        assert detmatch._CONFUSION_ON
        on, calls, preds, batch = _validator(c)
        on.update_metrics(preds, batch)
        on.update_metrics(preds, batch)                            # a second batch is added to the first
        assert not calls and on.seen == 2 * B
        assert np.array_equal(on.confusion_matrix.matrix, 2 * z["ref_per_image"].sum(0)) and on.confusion_matrix.matrix.dtype == np.float64
        half = {k: v[:len(v) // 2] for k, v in on.metrics.stats.items()}
        assert _same_lists(half, off.metrics.stats) and off.metrics.stats["tp"]
        for kw in (dict(matches={}), dict(nc=120)):                # visualize, and more classes than the device holds: the per-image call
            v, calls, preds, batch = _validator(c, **kw)
            v.update_metrics(preds, batch)
            assert calls == list(range(B)) and not v.confusion_matrix.matrix.any() and _same_lists(v.metrics.stats, off.metrics.stats)
        v, calls, preds, batch = _validator(c)                     # a label class outside the matrix: status 3, the per-image calls take the batch
        batch["cls"] = torch.full_like(batch["cls"], c["nc"])
        v.update_metrics(preds, batch)
        assert calls == list(range(B)) and not v.confusion_matrix.matrix.any() and v.seen == B
        v, calls, preds, batch = _validator(c)
        v.args.plots = False                                       # no plots: neither
        v.update_metrics(preds, batch)
        assert not calls and not v.confusion_matrix.matrix.any()
    finally:
        uninstall()
    assert not detmatch._CONFUSION_ON
