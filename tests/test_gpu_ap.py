"""Average precision on the device (include/ext/mgaap.h) against the oracle's rule (tests/ap_oracle.py): every case of tests/ap_cases.py
through `ap_per_class` and through `DetApPlan`; row counts at the edges of a wave, of the sort's tile and of the one-workgroup scan's trip;
junk behind the live rows; a real DetMatchPlan's accumulation, eagerly and as one captured chain; the status words; equal bytes on every
run.  The bars are the issue's: integers and the interpolated curves EQUAL, ap within 128 * 2^-53 * (the sum of its absolute terms)."""
import numpy as np
import pytest
import torch

import ap_cases as AC
import ap_oracle as AO
from mga_yolo_amd import _lib, detap

pytestmark = pytest.mark.gpu
K = _lib.AP_TILE
KEYS = ("tp", "conf", "pred_cls", "target_cls")


@pytest.fixture(scope="module")
def rules():
    """the oracle's dense answer of every case, computed once"""
    out = {}
    for name in AC.CASES:
        c = AC.build(name)
        out[name] = (c, AO.rule(*(c[k] for k in KEYS), c["nc"]))
    return out


def _filled(c, rows_cap=None, tgt_cap=None, junk=True):
    """A DetMatchPlan whose accumulation holds the case's rows -- written into its arena, behind them NaN confidences and class junk -- and
    the DetApPlan that reads it in place"""
    from mga_yolo_amd import DetApPlan, DetMatchPlan
    n, m, niou = c["tp"].shape[0], c["target_cls"].shape[0], c["tp"].shape[1]
    match = DetMatchPlan.create(1, 1, n_cap=1, m_cap=1, imgsz=64, iouv=np.linspace(0.2, 0.95, niou) if niou > 1 else [0.5],
                                rows_cap=rows_cap or 2 * n + 3, tgt_cap=tgt_cap or 2 * m + 3)
    plan = DetApPlan.create(match, nc=c["nc"])
    rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state = plan._st.args[:7]
    assert rows_tp.data_ptr() >= match._arena.data_ptr() and state.data_ptr() == match.state.data_ptr()     # in place
    if junk:
        rows_tp.fill_(1); rows_conf.fill_(float("nan")); rows_cls.fill_(1e9); tgt_cls.fill_(float("nan"))
    rows_tp[:n] = torch.from_numpy(c["tp"].astype(np.uint8)).cuda()
    rows_conf[:n], rows_cls[:n], tgt_cls[:m] = (torch.from_numpy(c[k]).cuda() for k in ("conf", "pred_cls", "target_cls"))
    state.copy_(torch.tensor([n, m, 7, 0], dtype=torch.int32))
    return match, plan


def _dense(plan):
    plan.run()
    torch.cuda.synchronize()
    plan.check_status()
    return plan._st.dense()


@pytest.mark.parametrize("name", AC.CASES)
def test_every_case_through_ap_per_class_and_through_the_plan(rules, name):
    c, want = rules[name]
    got = detap.ap_per_class(*(torch.from_numpy(c[k]).cuda() for k in KEYS), nc=c["nc"])
    AO.assert_tuple(got, detap._finish(want), AO.compact(want)["ap_abs"], name + " through ap_per_class")
    match, plan = _filled(c)
    before = match._arena.clone()
    AO.assert_dense(_dense(plan), want, name + " through DetApPlan")
    assert torch.equal(match._arena, before)                                      # the accumulation and state are read, never written
    AO.assert_tuple(plan.results(), detap._finish(want), AO.compact(want)["ap_abs"], name + " results()")
    assert len(plan.box_results()) == 10 and np.array_equal(plan.nt_per_class, want["nt"])
    if name in AC.ANSWERS:
        assert np.abs(plan._st.dense()["ap"][0] - AC.ANSWERS[name]).max() <= 1e-12


EDGES = [0, 1, 63, 64, 65, K - 1, K, K + 1, 2 * K + 1]


@pytest.mark.parametrize("n", EDGES)
def test_row_counts_at_the_edges_of_a_wave_and_of_the_tile(n):
    c = AC.random_case(np.random.default_rng([7, n]), n, 400, 3, 2) if n else AC.build("no_detections")
    AO.assert_dense(_dense(_filled(c, rows_cap=max(n, 1))[1]), AO.rule(*(c[k] for k in KEYS), c["nc"]), f"{n} rows, rows_cap = n")
    AO.assert_dense(_dense(_filled(c, rows_cap=3 * K + 5)[1]), AO.rule(*(c[k] for k in KEYS), c["nc"]), f"{n} rows, rows_cap well above")


def test_a_class_boundary_on_a_tile_boundary():
    rng = np.random.default_rng(11)
    c = AC.random_case(rng, 2 * K + 100, 900, 3, 3, labelled=3)
    c["pred_cls"][:] = np.repeat(np.float32([1, 0, 2, 1]), [K // 2, K, 100, K // 2])[rng.permutation(2 * K + 100)]   # class 0: exactly one tile
    c = AC._capped(c)
    want = AO.rule(*(c[k] for k in KEYS), c["nc"])
    assert want["n_det"].tolist() == [K, K, 100]
    AO.assert_dense(_dense(_filled(c)[1]), want, "class boundaries at K and 2K")


@pytest.mark.parametrize("nc", [1, 80])
def test_more_than_256_tiles(nc):
    """the one-workgroup scans of the digit table, the tile sums and the tile envelopes take several trips"""
    n = 256 * K + 777
    c = AC.random_case(np.random.default_rng([13, nc]), n, 90000, nc, 2)
    AO.assert_dense(_dense(_filled(c, rows_cap=n + 5, tgt_cap=90001)[1]), AO.rule(*(c[k] for k in KEYS), nc), f"{n} rows, nc {nc}")


def _feats(B, nc, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for h in (8, 4):
        f = 0.5 * torch.randn(B, 64 + nc, h, h, generator=g)
        f[:, 64:] = -4 + 4.5 * torch.rand(B, nc, h, h, generator=g)
        out.append(f)
    return out


def _labels_from(post, rs, B, n_lab):
    """labels that are jittered copies of rows the post-process kept, so there is something to match"""
    dets, count = post.dets.cpu(), post.count.cpu()
    bi = torch.from_numpy(rs.randint(0, B, n_lab).astype(np.float32))
    rows = [dets[int(b), rs.randint(int(count[int(b)]))] for b in bi]
    bx = torch.stack([torch.stack(((q[0] + q[2]) / 2, (q[1] + q[3]) / 2, (q[2] - q[0]) * (1 + 0.2 * rs.uniform(-1, 1)), q[3] - q[1])) / 64 for q in rows])
    cl = torch.stack([q[5] for q in rows]).reshape(-1, 1)
    return bi.cuda(), cl.cuda(), bx.cuda()


def _chain(captured):
    from mga_yolo_amd import DetApPlan, DetMatchPlan, DetPostPlan
    B, nc, D = 3, 2, 24
    post = DetPostPlan.create([(B, 8, 8), (B, 4, 4)], nc, strides=(8, 16), conf_thres=0.3, iou_thres=0.5, max_det=D, multi_label=True)
    match = DetMatchPlan.create(B, D, n_cap=16, m_cap=8, imgsz=64, rows_cap=3 * B * D, tgt_cap=32, dets=post.dets, count=post.count)
    ap = DetApPlan.create(match, nc=nc)
    step = lambda: (post.run(), match.run(), ap.run())
    if captured:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        step = graph.replay
    blocks = []
    for _ in range(2 if captured else 1):
        match.reset()
        rs = np.random.RandomState(3)
        for r, n_lab in enumerate((5, 4, 9)):
            for dst, src in zip(post.feats, _feats(B, nc, 50 + r)):
                dst.copy_(src)
            post.run()                                                            # eagerly, to draw this batch's labels from its rows
            match.set_labels(*_labels_from(post, rs, B, n_lab))
            step()
            torch.cuda.synchronize()
            post.check_status(); match.check_status(); ap.check_status()
        blocks.append(ap.result.cpu().numpy().copy())
    s = match.stats()
    assert s["tp"].any() and not s["tp"].all() and s["target_cls"].size == 18
    want = AO.rule(s["tp"], s["conf"], s["pred_cls"], s["target_cls"], nc)
    AO.assert_dense(ap._st.dense(), want, "three accumulated batches")
    AO.assert_tuple(ap.results(), detap._host_ap(s["tp"], s["conf"], s["pred_cls"], s["target_cls"], nc=nc), AO.compact(want)["ap_abs"],
                    "results() against _host_ap on match.stats()")
    return blocks


def test_three_batches_accumulated_by_a_real_matching_plan():
    _chain(captured=False)


def test_the_same_as_one_captured_chain_replayed_twice_with_equal_bits():
    first, second = _chain(captured=True)
    assert first.tobytes() == second.tobytes()


def test_status_3_status_4_and_3_before_4(rules):
    c, _ = rules["seed_nc3_t10"]
    for what, conf_nan, bad_target, status in (("a NaN confidence", True, None, 4), ("a target class of nc", False, 3.0, 3),
                                               ("a target class of 1.5", False, 1.5, 3), ("a NaN target class", False, float("nan"), 3),
                                               ("both", True, -1.0, 3)):
        match, plan = _filled(c)
        if conf_nan:
            plan._st.args[1][17] = float("nan")
        if bad_target is not None:
            plan._st.args[4][5] = bad_target
        before = match._arena.clone()
        plan.run()
        torch.cuda.synchronize()
        assert int(plan.status) == status, what
        with pytest.raises(RuntimeError, match="target class" if status == 3 else "NaN"):
            plan.check_status()
        d = plan._st.dense()
        assert all(np.isnan(d[k]).all() for k in ("ap", "p_curve", "r_curve", "prec_values")) and (d["nt"] == -1).all() and (d["n_det"] == -1).all(), what
        assert torch.equal(match._arena.view(torch.uint8), before.view(torch.uint8)), what      # the accumulation and state are untouched
        with pytest.raises(RuntimeError, match="non-zero status"):
            plan.results()
    with pytest.raises(RuntimeError, match="NaN"):
        bad = c["conf"].copy()
        bad[3] = np.nan
        detap.ap_per_class(torch.from_numpy(c["tp"]).cuda(), torch.from_numpy(bad).cuda(), *(torch.from_numpy(c[k]).cuda() for k in KEYS[2:]), nc=3)


@pytest.mark.parametrize("name", ["seed_nc80_junk", "seed_nc300_t16", "ties"])
def test_two_runs_give_the_same_bytes(rules, name):
    _, plan = _filled(rules[name][0])
    plan.run()
    first = (plan.result.cpu().numpy().copy(), int(plan.status))
    plan.result.fill_(0xAB)
    plan._st.ws.fill_(0xCD)                                                        # the workspace needs no initialisation
    plan.run()
    assert (plan.result.cpu().numpy().tobytes(), int(plan.status)) == (first[0].tobytes(), first[1])


def test_the_installed_replacement_runs_on_the_device(rules):
    import sys
    import types
    c, want = rules["seed_nc3_t10"]
    name = "ultralytics.utils.metrics"
    if name in sys.modules:
        pytest.skip("the reference itself is importable here: the stub would shadow it")
    made = [n for n in ("ultralytics", "ultralytics.utils", name) if n not in sys.modules]
    for n in made:
        sys.modules[n] = types.ModuleType(n)
    sys.modules[name].ap_per_class = lambda *a, **k: "reference"
    import mga_yolo_amd
    try:
        mga_yolo_amd.install(ap=True)
        got = sys.modules[name].ap_per_class(*(c[k] for k in KEYS))
        AO.assert_tuple(got, detap._finish(want), AO.compact(want)["ap_abs"], "the replacement")
    finally:
        mga_yolo_amd.uninstall()
        for n in made:
            sys.modules.pop(n, None)
