"""The confusion matrix without a GPU: the oracle's two statements against each other, against the reference's stored per-image matrices
and against the answers by construction; every wrong rule against the case built for it; the torch statement (`_host_confusion`) against the
oracle element by element; reference_conf; and the install switch on a stub validator."""
import types

import numpy as np
import pytest
import torch

import confusion_cases as CC
import confusion_oracle as CO

_LOADED = {}


def _case(name):
    """the case, its record and its oracle: computed once, shared, left unchanged"""
    if name not in _LOADED:
        c, z = CC.load(name)
        _LOADED[name] = (c, z, CC.oracle(name, c))
    return _LOADED[name]


@pytest.mark.parametrize("name", CC.NAMES)
def test_rule_equals_procedure_and_the_guards_hold(name):
    c, _, o = _case(name)
    guards = [g for g in o["guards"] if not (name in CC.TWINS and "two largest" in g)]
    assert not guards and not CC.built_for(name, c, o)
    if name in CC.PARITY:                                          # on equal IoUs the procedure's order is an unstable sort's
        p = CC.oracle(name, c, use_procedure=True)
        for k in ("cm", "per_image", "det_out", "lab_out"):
            assert np.array_equal(p[k], o[k]), k
    assert o["cm"].sum() == (o["lab_out"] >= 0).sum() + (o["det_out"] == c["nc"]).sum()


@pytest.mark.parametrize("name", CC.PARITY)
def test_oracle_equals_the_reference_s_per_image_matrices(name):
    c, z, o = _case(name)
    assert z["ref_per_image"].shape == o["per_image"].shape and np.array_equal(z["ref_per_image"], o["per_image"])


@pytest.mark.parametrize("name", list(CC.ANSWERS))
def test_oracle_equals_the_answer_by_construction(name):
    c, _, o = _case(name)
    a = CC.ANSWERS[name]
    rows = np.nonzero(c["batch_idx"] == 0)[0]
    assert np.array_equal(o["cm"], CC.answer_matrix(name))
    assert o["det_out"][0].tolist() == a["det_out"] and o["lab_out"][rows].tolist() == a["lab_out"]
    assert (np.delete(o["lab_out"], rows) == -1).all()


@pytest.mark.parametrize("name", list(CC.BUILT_AGAINST))
def test_every_wrong_rule_fails_the_case_built_against_it(name):
    c, _, o = _case(name)
    w = CC.oracle(name, c, wrong=CC.BUILT_AGAINST[name])
    assert not np.array_equal(w["cm"], o["cm"])
    assert sorted(CC.BUILT_AGAINST.values()) == sorted(CO.WRONG)   # and every wrong rule has its case


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("name", CC.NAMES)
def test_host_statement_equals_the_oracle(name, dtype):
    from mga_yolo_amd import confusion_matrix
    c, _, o = _case(name)
    dets, count, bi, cl, bx = CC.tensors(CC.live(c))
    cm, det_out, lab_out = confusion_matrix(dets.to(dtype), count, bi, cl, bx, nc=c["nc"], imgsz=c["hw"], conf=c["conf"], iou_thres=c["iou_thres"],
                                            single_cls=c["single_cls"])
    n = len(CC.live(c)["batch_idx"])
    assert cm.dtype == torch.int64 and det_out.dtype == torch.int32 and lab_out.dtype == torch.int32
    assert np.array_equal(det_out.numpy(), o["det_out"]) and np.array_equal(lab_out.numpy(), o["lab_out"][:n])
    assert np.array_equal(cm.numpy(), o["cm"])


def test_host_statement_refuses_a_class_outside_the_matrix():
    from mga_yolo_amd import confusion_matrix
    c, _, _ = _case("basic")
    dets, count, bi, cl, bx = CC.tensors(c)
    with pytest.raises(ValueError, match="class"):
        confusion_matrix(dets, count, bi, torch.full_like(cl, c["nc"]), bx, nc=c["nc"], imgsz=c["hw"])
    confusion_matrix(dets, count, bi, torch.full_like(cl, c["nc"]), bx, nc=c["nc"], imgsz=c["hw"], single_cls=True)
    for bad in (dict(iou_thres=1.0), dict(iou_thres=-0.1), dict(conf=float("inf")), dict(iou_thres=float("nan"))):
        with pytest.raises(ValueError):
            confusion_matrix(dets, count, bi, cl, bx, nc=c["nc"], imgsz=c["hw"], **bad)


def test_reference_conf():
    from mga_yolo_amd import reference_conf
    assert reference_conf(None) == 0.25 and reference_conf(0.001) == 0.25 and reference_conf(0.25) == 0.25
    assert reference_conf(0.01) == 0.01 and reference_conf(0.5) == 0.5 and reference_conf(0.0) == 0.0
    assert all(CC.conf_thres(CC.build(n, 100)) == reference_conf(CC.build(n, 100)["conf"]) for n in ("basic", "nword", "empty"))


def _stub(c, calls):
    """a stub validator on host tensors with detmatch.update_metrics bound, plots on, and a counting ConfusionMatrix stand-in"""
    from mga_yolo_amd import detmatch
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])

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
    v.iouv = torch.linspace(0.5, 0.95, 10)
    v.args = types.SimpleNamespace(single_cls=False, plots=True, visualize=False, save_json=False, save_txt=False, conf=c["conf"])
    v.metrics = types.SimpleNamespace(stats=stats, update_stats=lambda s: [stats[k].append(x) for k, x in s.items()])
    v.confusion_matrix = types.SimpleNamespace(nc=c["nc"], task="detect", matches=None, matrix=np.zeros((c["nc"] + 1, c["nc"] + 1)),
                                               process_batch=lambda predn, pbatch, conf: calls.append((pbatch["si"], conf)))
    dets, count, bi, cl, bx = CC.tensors(CC.live(c))
    B = dets.shape[0]
    preds = [dict(bboxes=dets[b, :max(int(count[b]), 0), :4].clone(), conf=dets[b, :max(int(count[b]), 0), 4].clone(),
                  cls=dets[b, :max(int(count[b]), 0), 5].clone()) for b in range(B)]
    return v, preds, dict(batch_idx=bi, cls=cl, bboxes=bx, img=torch.empty(B, 0, *c["hw"]))


def test_install_switch_and_the_host_path_keeps_the_per_image_calls():
    from mga_yolo_amd import detmatch, install, uninstall
    c, _, _ = _case("basic")
    assert detmatch._CONFUSION_ON is False
    with pytest.raises(ValueError, match="match=True"):
        install(confusion=True)
    assert detmatch._CONFUSION_ON is False
    try:
        install(match=True, confusion=True)
        assert detmatch._CONFUSION_ON is True
        install(match=True, confusion=True)                        # twice: one undo record
        calls = []
        v, preds, batch = _stub(c, calls)
        v.update_metrics(preds, batch)                             # host tensors: the reference's per-image path, switch or not
        assert calls == [(b, c["conf"]) for b in range(len(preds))] and not v.confusion_matrix.matrix.any() and v.seen == len(preds)
    finally:
        uninstall()
    assert detmatch._CONFUSION_ON is False
    install(match=True)                                            # without confusion= the switch stays off
    try:
        assert detmatch._CONFUSION_ON is False
    finally:
        uninstall()
