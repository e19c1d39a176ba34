"""Average precision without a GPU: the oracle's two statements (tests/ap_oracle.py) against each other, against the reference's recorded
outputs (tests/golden/ap_*.npz) and against the answers known by hand; mga_yolo_amd.detap's host path against the oracle; the 12-tuple's
shapes and dtypes, the degenerate cases included; install(ap=True) / uninstall() on a stub of the reference's ultralytics.utils.metrics."""
import sys
import types
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import ap_cases as AC
import ap_oracle as AO
from mga_yolo_amd import detap


@pytest.fixture(scope="module")
def answers():
    """every case's inputs, the literal procedure's tuple and the rule's dense arrays, computed once"""
    out = {}
    for name in AC.CASES:
        c = AC.build(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            lit, lit_abs = AO.procedure(c["tp"], c["conf"], c["pred_cls"], c["target_cls"])
        out[name] = dict(case=c, lit=lit, lit_abs=lit_abs, rule=AO.rule(c["tp"], c["conf"], c["pred_cls"], c["target_cls"], c["nc"]))
    return out


def test_the_cases_hold_what_they_were_built_for():
    built = {n: AC.build(n) for n in AC.CASES}
    for name in AC.PARITY:
        assert AC.distinct_within_class(built[name]), name            # the reference alone decides these
    for name in AC.TIES:
        assert not AC.distinct_within_class(built[name]), name
    assert {built[n]["nc"] for n in AC.SEEDED} == {1, 3, 80, 300} and {built[n]["tp"].shape[1] for n in AC.CASES} >= {1, 10, 16}
    junk = built["seed_nc80_junk"]["pred_cls"]
    assert (junk == 2.5).any() and (junk == 80).any() and (junk == -1).any()
    assert (built["seed_nc300_t16"]["target_cls"] > 255).any()        # the second class digit
    z = built["signed_zeros"]["conf"]
    assert np.signbit(z).any() and (z == 0).sum() == 4 and not np.signbit(z[z == 0]).all()
    d = built["one_and_denormal"]["conf"]
    assert d.max() == 1.0 and 0 < d.min() < np.finfo(np.float32).tiny
    for name in AC.CASES:
        a, b = built[name], AC.build(name)
        assert all(np.array_equal(a[k], b[k]) for k in ("tp", "conf", "pred_cls", "target_cls")), name      # rebuilt from the seed


@pytest.mark.parametrize("name", AC.CASES)
def test_the_procedure_and_the_rule_agree(answers, name):
    a = answers[name]
    AO.compare(*(a["case"][k] for k in ("tp", "conf", "pred_cls", "target_cls")), a["case"]["nc"])
    got = detap._finish(a["rule"])
    AO.assert_tuple(got, a["lit"], a["lit_abs"], name)
    c = AO.compact(a["rule"])
    assert np.array_equal(c["classes"], np.unique(a["case"]["target_cls"]).astype(int))
    assert np.array_equal(c["ap_abs"], a["lit_abs"])


@pytest.mark.parametrize("name", AC.PARITY)
def test_the_oracle_equals_the_reference_s_recorded_outputs(answers, name):
    inputs, ref = AC.load_golden(name)
    c = answers[name]["case"]
    assert all(np.array_equal(inputs[k], c[k]) for k in inputs), "the record's inputs are the case's"
    AO.assert_tuple(answers[name]["lit"], ref, answers[name]["lit_abs"], name + ": procedure")
    AO.assert_tuple(detap._finish(answers[name]["rule"]), ref, answers[name]["lit_abs"], name + ": rule")
    for g, r in zip(detap._host_ap(c["tp"], c["conf"], c["pred_cls"], c["target_cls"], nc=c["nc"]), ref):
        assert np.asarray(g).dtype == r.dtype and np.asarray(g).shape == r.shape, name


@pytest.mark.parametrize("name", sorted(AC.ANSWERS))
def test_the_answers_known_by_hand(answers, name):
    ap = answers[name]["rule"]["ap"][0]
    assert np.abs(ap - AC.ANSWERS[name]).max() <= 1e-12, (name, ap)
    if name == "ties":                                               # accumulation order decides; the other order has another answer
        c = answers[name]["case"]
        other = AO.rule(c["tp"][::-1], c["conf"][::-1], c["pred_cls"][::-1], c["target_cls"], c["nc"])["ap"][0]
        assert np.abs(other - AC.TIES_OTHER_ORDER).max() <= 1e-12 and abs(AC.TIES_OTHER_ORDER - AC.ANSWERS[name]) > 0.2


def test_signed_zeros_tie_and_keep_their_order(answers):
    c = answers["signed_zeros"]["case"]
    plus = AO.rule(c["tp"], np.abs(c["conf"]), c["pred_cls"], c["target_cls"], c["nc"])
    for k in ("ap", "p_curve", "r_curve", "prec_values"):
        assert np.array_equal(plus[k], answers["signed_zeros"]["rule"][k]), k


def test_np_interp_takes_the_last_of_repeated_abscissae():
    xp, fp = [0, .5, .5, 1, 1], [1, .8, .6, .3, 0]
    assert np.interp(0.5, xp, fp) == 0.6 == AO.interp_rule([0.5], xp, fp)[0] == detap._interp(np.array([0.5]), np.array(xp), np.array(fp))[0]
    assert np.interp(1.0, xp, fp) == 0 == AO.interp_rule([1.0], xp, fp)[0] == detap._interp(np.array([1.0]), np.array(xp), np.array(fp))[0]
    x = np.linspace(0, 1, 1000)
    assert np.array_equal(np.interp(x, xp, fp), AO.interp_rule(x, xp, fp))
    assert np.array_equal(np.interp(-x, [-.7, -.7, -.2], [.1, .4, .9], left=1), AO.interp_rule(-x, [-.7, -.7, -.2], [.1, .4, .9], left=1.0))


@pytest.mark.parametrize("name", AC.CASES)
def test_host_ap_equals_the_oracle(answers, name):
    a = answers[name]
    c = a["case"]
    dense = detap._host_curves(c["tp"], c["conf"], c["pred_cls"], c["target_cls"], c["nc"])
    AO.assert_dense(dense, a["rule"], name)
    want = detap._finish(a["rule"])
    for kind in (np.asarray, torch.from_numpy):
        got = detap.ap_per_class(*(kind(c[k]) for k in ("tp", "conf", "pred_cls", "target_cls")), nc=c["nc"])
        AO.assert_tuple(got, want, AO.compact(a["rule"])["ap_abs"], name)
    sized = detap.ap_per_class(c["tp"], c["conf"], c["pred_cls"], c["target_cls"])                       # nc from the targets
    AO.assert_tuple(sized, want, AO.compact(a["rule"])["ap_abs"], name + ": nc=None")


def test_the_tuple_s_shapes_and_dtypes():
    for name, k in (("seed_nc3_t10", 3), ("labels_no_dets", 2), ("no_targets", 0), ("no_detections", 2)):
        c = AC.build(name)
        niou = c["tp"].shape[1]
        tp, fp, p, r, f1, ap, classes, p_curve, r_curve, f1_curve, x, prec_values = detap.ap_per_class(
            c["tp"], c["conf"], c["pred_cls"], c["target_cls"], nc=c["nc"])
        assert [a.shape for a in (tp, fp, p, r, f1, classes)] == [(k,)] * 6, name
        assert ap.shape == (k, niou) and p_curve.shape == r_curve.shape == f1_curve.shape == (k, 1000) and x.shape == (1000,), name
        assert all(a.dtype == np.float64 for a in (tp, fp, p, r, f1, ap, p_curve, r_curve, f1_curve, x, prec_values)), name
        assert classes.dtype == np.dtype(int), name
    assert prec_values.shape == (1, 1000) and not prec_values.any()                                      # no class has detections and labels
    one = detap.ap_per_class(*(AC.build("labels_no_dets")[k] for k in ("tp", "conf", "pred_cls", "target_cls")), nc=3)
    assert one[11].shape == (1, 1000) and not one[5][1].any() and not one[7][1].any()                    # class 1: labels, no detections


def test_what_the_host_path_refuses():
    c = AC.build("seed_nc3_t10")
    args = [c[k] for k in ("tp", "conf", "pred_cls", "target_cls")]
    with pytest.raises(ValueError, match="target class"):
        detap.ap_per_class(*args, nc=2)
    with pytest.raises(ValueError, match="target class"):
        detap.ap_per_class(*args[:3], np.float32([0, 1.5]), nc=3)
    conf = c["conf"].copy()
    conf[5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        detap.ap_per_class(args[0], conf, *args[2:], nc=3)
    with pytest.raises(ValueError, match="niou"):
        detap.ap_per_class(args[0][:, 0], *args[1:], nc=3)


@pytest.fixture
def stub_metrics():
    calls = []

    def ref_ap(*a, **k):
        return "reference"
    names = ("ultralytics.utils.metrics", "mga_yolo.external.ultralytics.ultralytics.utils.metrics")
    made = {}
    for name in ("ultralytics", "ultralytics.utils") + names:
        if name not in sys.modules:
            made[name] = sys.modules[name] = types.ModuleType(name)
    if not made.keys() >= set(names):
        for name in made:
            del sys.modules[name]
        pytest.skip("the reference itself is importable here: the stub would shadow it")
    for i, name in enumerate(names):
        made[name].ap_per_class = ref_ap
        made[name].plot_pr_curve = lambda *a, _i=i, **k: calls.append((_i, "pr", a, k))
        made[name].plot_mc_curve = lambda *a, _i=i, **k: calls.append((_i, "mc", a, k))
    yield [sys.modules[n] for n in names], ref_ap, calls
    for name in made:
        sys.modules.pop(name, None)


def test_install_ap_is_opt_in_and_uninstall_restores(stub_metrics):
    import mga_yolo_amd
    mods, ref_ap, calls = stub_metrics
    c = AC.build("seed_nc3_t10")
    args = [c[k] for k in ("tp", "conf", "pred_cls", "target_cls")]
    try:
        mga_yolo_amd.install()                                      # the default leaves the metrics alone
        assert all(m.ap_per_class is ref_ap for m in mods)
        patched = mga_yolo_amd.install(ap=True)
        assert {m.__name__ for m in mods} <= set(patched)
        fns = [m.ap_per_class for m in mods]
        assert all(f is not ref_ap and f.__name__ == "ap_per_class" for f in fns) and fns[0] is not fns[1]
        mga_yolo_amd.install(ap=True)                               # a second call rebinds nothing
        assert [m.ap_per_class for m in mods] == fns
        if not torch.cuda.is_available():                           # (with a GPU the replacement runs there: tests/test_gpu_ap.py)
            import inspect
            assert list(inspect.signature(fns[0]).parameters) == ["tp", "conf", "pred_cls", "target_cls", "plot", "on_plot", "save_dir",
                                                                  "names", "eps", "prefix"]
            want = detap._host_ap(*args)
            got = fns[1](*args, plot=True, save_dir=Path("out"), names={0: "a", 2: "c", 7: "z"}, prefix="B")
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            assert [(i, kind) for i, kind, _, _ in calls] == [(1, "pr"), (1, "mc"), (1, "mc"), (1, "mc")]       # the module's own, looked up when called
            shown = {i: n for i, n in enumerate(["a", None, "c"]) if n}
            assert calls[0][2][3] == Path("out") / "BPR_curve.png" and calls[0][2][4] == shown and calls[0][2][2] is got[5]
            assert [k["ylabel"] for _, _, _, k in calls[1:]] == ["F1", "Precision", "Recall"]
            assert [a[2].name for _, _, a, _ in calls[1:]] == ["BF1_curve.png", "BP_curve.png", "BR_curve.png"]
            assert fns[0](*args) is not None and len(calls) == 4    # plot=False draws nothing
    finally:
        mga_yolo_amd.uninstall()
    assert all(m.ap_per_class is ref_ap for m in mods)
