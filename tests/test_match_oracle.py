"""The detection matching without a GPU: tests/match_oracle.py against the stored answers of the reference's validator (tests/golden/match_*.npz,
tools/gen_golden_match.py), its two statements of the matching against each other, the host path (detmatch._host_match) against the oracle, the
four wrong rules against the cases built for them, and the replacement update_metrics against the lists the reference's own left."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import match_cases as MC
import match_oracle as O
from conftest import GOLDEN

RATIOS = json.load(open(os.path.join(GOLDEN, "match_ratios.json")))
K = max(2 * RATIOS["worst"], 1.0)                                  # the bar of the GPU tests; the host path is held to it as well


@pytest.fixture(scope="module")
def loaded():
    """every case, its record and its oracle, computed once"""
    out = {}
    for name in MC.NAMES:
        c, z = MC.load(name)
        out[name] = (c, z, MC.oracle(name, c))
    return out


@pytest.mark.parametrize("name", MC.NAMES)
def test_oracle_against_the_golden(loaded, name):
    c, z, o = loaded[name]
    why = [g for g in o["guards"] if not (name in MC.TWINS and "two largest" in g)]
    assert not why and not MC.built_for(name, c, o), why
    if name in MC.PARITY:
        assert np.array_equal(o["tp"], z["ref_tp"])
        assert np.array_equal(MC.oracle(name, c, use_procedure=True)["tp"], z["ref_tp"])
    r = O.ratio(z["ref_best_iou_f32"], o["best_iou"], o["term"])
    assert r == pytest.approx(float(z["ratio"])) and r <= RATIOS["worst"] == max(RATIOS["cases"].values())
    if name in MC.ANSWERS:
        a = MC.ANSWERS[name]
        k = len(a["tp"])
        assert o["tp"][0, :k].tolist() == a["tp"] and o["best_gt"][0, :k].tolist() == a["best_gt"]


def test_the_rule_is_the_procedure_on_random_matrices():
    """3000 label x detection matrices, a third of their entries 0 (another class), no two equal otherwise"""
    rs = np.random.RandomState(7)
    thrs = [float(t) for t in MC.IOUV10]
    true = 0
    for _ in range(3000):
        L, D = rs.randint(1, 7), rs.randint(1, 10)
        iou = rs.permutation(np.linspace(0.3, 0.99, L * D) + rs.uniform(0, 1e-3)).reshape(L, D) * (rs.uniform(size=(L, D)) > 0.33)
        tp, _, _ = O.rule(iou, thrs)
        for t, thr in enumerate(thrs):
            assert np.array_equal(tp[:, t], O.procedure(iou, thr)), (iou, thr)
        true += int(tp.sum())
    assert true > 30000


@pytest.mark.parametrize("name", MC.NAMES)
def test_host_path_against_the_oracle(loaded, name):
    from mga_yolo_amd import match_detections
    c, z, o = loaded[name]
    lc = MC.live(c)
    tp, best_iou, best_gt = match_detections(*MC.tensors(lc), imgsz=c["hw"], iouv=c["iouv"], single_cls=c["single_cls"])
    assert tp.dtype == torch.bool and tuple(tp.shape) == c["dets"].shape[:2] + (len(c["iouv"]),)
    assert np.array_equal(tp.numpy(), o["tp"]) and np.array_equal(best_gt.numpy(), o["best_gt"])
    assert O.ratio(best_iou.numpy(), o["best_iou"], o["term"]) <= K
    if name in MC.PARITY:                                          # the same fp32 operations in the same order as the reference's box_iou
        assert np.array_equal(best_iou.numpy(), z["ref_best_iou_f32"])


@pytest.mark.parametrize("n", MC.N_WORDS)
def test_chunks_under_an_n_word_in_its_second_chunk(loaded, n):
    """the inputs of the GPU plan test: the guards hold with the rows behind the word cut off, the word changes the answer, and the host
    path on the rows before it gives the oracle's"""
    from mga_yolo_amd import match_detections
    c, _, every = loaded["chunks"]
    cut = dict(c, n=n)
    o = MC.oracle("chunks", cut)
    assert not o["guards"] and o["best_gt"].max() < n and not np.array_equal(o["best_gt"], every["best_gt"])
    tp, best_iou, best_gt = match_detections(*MC.tensors(MC.live(cut)), imgsz=c["hw"], iouv=c["iouv"])
    assert np.array_equal(tp.numpy(), o["tp"]) and np.array_equal(best_gt.numpy(), o["best_gt"])
    assert O.ratio(best_iou.numpy(), o["best_iou"], o["term"]) <= K


@pytest.mark.parametrize("name,wrong", sorted(MC.BUILT_AGAINST.items()))
def test_a_wrong_rule_fails_the_case_built_for_it(loaded, name, wrong):
    c, _, o = loaded[name]
    assert not np.array_equal(MC.oracle(name, c, wrong=wrong)["tp"], o["tp"])
    assert o["tp"][0, :len(MC.ANSWERS[name]["tp"])].tolist() == MC.ANSWERS[name]["tp"]


def test_strictly_greater_fails_an_iou_on_the_threshold():
    """`>` instead of `>=`: a label of 10 x 10 and a detection that is its lower half have IoU 50 / (100 + 50 - 50 + 1e-7) = 0.5 exactly in fp32
    (no case of the goldens can hold this: the fp64 oracle's 0.4999999995 lies on the other side).  The rule level, then the host path."""
    iou = np.array([[0.5, 0.75]])
    tp, _, _ = O.rule(iou, [0.5, 0.75])
    wrong, _, _ = O.rule(iou, [0.5, 0.75], wrong="strictly_greater")
    assert tp.tolist() == [[True, False], [False, True]] and wrong.tolist() == [[False, False], [True, False]]
    from mga_yolo_amd import match_detections
    dets = torch.tensor([[[0., 0., 10., 5., 0.9, 0.]]])
    tp, best, gt = match_detections(dets, torch.tensor([1], dtype=torch.int32), torch.zeros(1), torch.zeros(1, 1),
                                    torch.tensor([[5 / 64, 5 / 64, 10 / 64, 10 / 64]]), imgsz=64, iouv=[0.5, 0.55])
    assert tp.tolist() == [[[True, False]]] and best.item() == 0.5 and gt.item() == 0


def test_call_forms_and_refused_arguments():
    from mga_yolo_amd import match_detections
    c, _ = MC.load("basic")
    d, n, bi, cl, bx = MC.tensors(c)
    a = match_detections(d, n, bi, cl, bx, imgsz=c["hw"])
    b = match_detections(d, n, bi, cl.reshape(-1), bx, imgsz=c["hw"], iouv=torch.linspace(0.5, 0.95, 10))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    sq = match_detections(d, n, bi, cl, bx, imgsz=128)
    assert all(torch.equal(x, y) for x, y in zip(sq, match_detections(d, n, bi, cl, bx, imgsz=(128, 128))))
    for bad in ([0.5, 0.5], [0.6, 0.5], [0.0, 0.5], [0.5, 1.5], [], [0.01 * i for i in range(1, 18)]):
        with pytest.raises(ValueError):
            match_detections(d, n, bi, cl, bx, imgsz=c["hw"], iouv=bad)
    with pytest.raises(ValueError):
        match_detections(d[..., :5], n, bi, cl, bx, imgsz=c["hw"])


def _stand_in(iouv, single_cls):
    stats = dict(tp=[], conf=[], pred_cls=[], target_cls=[], target_img=[])

    def prepare_pred(pred):
        if single_cls:
            pred["cls"] *= 0
        return pred
    return types.SimpleNamespace(iouv=torch.from_numpy(np.asarray(iouv)), niou=len(iouv), seen=0, _prepare_pred=prepare_pred,
                                 args=types.SimpleNamespace(single_cls=single_cls, plots=False, visualize=False, save_json=False, save_txt=False),
                                 metrics=types.SimpleNamespace(stats=stats, update_stats=lambda s: [stats[k].append(v) for k, v in s.items()]))


@pytest.mark.parametrize("name", MC.PARITY)
def test_replacement_update_metrics_leaves_the_reference_s_lists(loaded, name):
    from mga_yolo_amd import detmatch
    c, z, _ = loaded[name]
    lc = MC.live(c)
    dets, count, bi, cl, bx = MC.tensors(lc)
    B, D = dets.shape[:2]
    preds = []
    for b in range(B):
        k = min(max(int(count[b]), 0), D)
        preds.append(dict(bboxes=dets[b, :k, :4].clone(), conf=dets[b, :k, 4].clone(), cls=dets[b, :k, 5].clone()))
    batch = dict(batch_idx=bi, cls=cl * 0 if c["single_cls"] else cl, bboxes=bx, img=torch.empty(B, 0, *c["hw"]))
    s = _stand_in(c["iouv"], c["single_cls"])
    detmatch.update_metrics(s, preds, batch)
    assert s.seen == B
    for key, lst in s.metrics.stats.items():
        assert len(lst) == B
        for b, got in enumerate(lst):
            want = z[f"stats_{key}_{b}"]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (key, b)


@pytest.fixture
def stub_val():
    """Stand-ins for the two module objects the reference makes of ultralytics/models/yolo/detect/val.py"""
    names = ("ultralytics.models.yolo.detect.val", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.val")
    if any(n in sys.modules for n in names):
        pytest.skip("the reference itself is importable here: the stub would shadow it")
    made = []
    for n in names:
        parts = n.split(".")
        for i in range(1, len(parts) + 1):
            p = ".".join(parts[:i])
            if p not in sys.modules:
                sys.modules[p] = types.ModuleType(p)
                made.append(p)

        class DetectionValidator:
            def update_metrics(self, preds, batch):
                return "reference"

            def _process_batch(self, preds, batch):
                return {}

            def _prepare_batch(self, si, batch):
                return {}

            def match_predictions(self, pred_classes, true_classes, iou):
                return None
        sys.modules[n].DetectionValidator = DetectionValidator
    yield [sys.modules[n].DetectionValidator for n in names]
    for p in made:
        sys.modules.pop(p, None)


def test_install_match_is_opt_in_and_uninstall_restores(stub_val):
    import mga_yolo_amd
    from mga_yolo_amd import detmatch
    classes = stub_val
    originals = [c.__dict__["update_metrics"] for c in classes]

    class Sub(classes[1]):                                         # MGAValidator's place: it reaches the replacement through super()
        def update_metrics(self, preds, batch):
            return super().update_metrics
    try:
        mga_yolo_amd.install()
        mga_yolo_amd.install(nms=True)
        assert [c.__dict__["update_metrics"] for c in classes] == originals
        patched = mga_yolo_amd.install(match=True)
        assert all(c.__dict__["update_metrics"] is detmatch.update_metrics for c in classes)
        assert {"ultralytics.models.yolo.detect.val", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.val"} <= set(patched)
        assert Sub().update_metrics(None, None).__func__ is detmatch.update_metrics

        # a validator with a _process_batch, _prepare_batch or match_predictions of its own (masks, keypoints, rotated boxes) gets the
        # reference's method, the one install() replaced, not the axis-aligned matching
        for method in ("_process_batch", "_prepare_batch", "match_predictions"):
            for base in classes:
                Other = type("Other", (base,), {method: lambda self, *a: None})
                assert Other().update_metrics([], {}) == "reference", method
        Plain = type("Plain", (classes[0],), {"_prepare_pred": lambda self, p: p})     # nothing the replacement stands in for: it runs (no images)
        assert Plain().update_metrics([], {}) is None
        mga_yolo_amd.install(match=True)                           # a second call rebinds nothing and records nothing to undo twice
    finally:
        mga_yolo_amd.uninstall()
    assert [c.__dict__["update_metrics"] for c in classes] == originals


def test_update_metrics_bound_by_hand_refuses_what_it_does_not_cover():
    """without install() there is no method to hand a segmentation, pose or OBB validator to: a clear refusal, not wrong metrics"""
    from mga_yolo_amd import detmatch

    class Base:
        update_metrics = detmatch.update_metrics

        def _process_batch(self, preds, batch):
            return {}

        def _prepare_batch(self, si, batch):
            return {}

        def match_predictions(self, *a):
            return None

    class Obb(Base):
        def _process_batch(self, preds, batch):
            return {}
    with pytest.raises(NotImplementedError, match="_process_batch"):
        Obb().update_metrics([], {})


def test_assemble_stats_orders_image_after_image():
    from mga_yolo_amd.detmatch import assemble_stats
    s = assemble_stats(np.array([[1], [0], [1]], np.uint8), np.array([.9, .8, .7], np.float32), np.array([1, 2, 3], np.float32),
                       np.array([0, 0, 1], np.int32), np.array([4, 2, 2, 7], np.float32), np.array([1, 0, 1, 0], np.int32), 3)
    assert s["tp"].tolist() == [[True], [False], [True]] and s["tp"].dtype == bool and s["seen"] == 3
    assert s["target_cls"].tolist() == [2, 7, 4, 2] and s["target_img"].tolist() == [2, 7, 2, 4]
