"""The Detect maps read in place as torch.channels_last (include/ext/mgamaps.h: the NHWC instantiations of k_det_assign, k_det_resolve,
k_det_loss, k_det_bwd and k_nms_cand) against the NCHW device run of the same values: THE SAME BITS in every output, in fp32, fp16 and bf16.
Every stored case of the criterion and of the post-process; shapes the layout can break (row pitches of 65, 67, 69 and 144 elements, a 1 x 1
level, a workgroup that straddles an image and a level, B * A at and one past a multiple of the workgroup); levels carved out of larger buffers
at odd element offsets between sentinels; the poisoned call; no copy on the way in or out; both plans in one captured graph."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_cases as DC
import det_oracle as O
import nms_cases as NC
from test_gpu_det import EPS, UP1
from test_gpu_det import _check_assignment as _check_assignment_stored
from test_gpu_det_shapes import _check_against, _check_assignment

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=["fp32", "fp16", "bf16"])
CL = torch.channels_last
_INT = {F32: torch.int32, F16: torch.int16, BF16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64, torch.bool: torch.bool}


def _same(a, b):
    """torch.equal on the bit patterns: a NaN equals the same NaN"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(_INT[a.dtype]), b.contiguous().view(_INT[b.dtype]))


def _cl(t):
    return t.contiguous(memory_format=CL)


# ---- the criterion ----------------------------------------------------------------------------------------------------------------------
def _det(feats, labels, kw, up, dtype=F32, cl=False, **more):
    from mga_yolo_amd import detection_loss
    xs = [f.to(dtype).cuda() for f in feats]
    xs = [(_cl(x) if cl else x).requires_grad_(True) for x in xs]
    loss, items, asg = detection_loss(xs, *(t.cuda() for t in labels), return_assignment=True, **kw, **more)
    gs = torch.autograd.grad((loss * torch.tensor(up, dtype=F32, device="cuda")).sum(), xs)
    torch.cuda.synchronize()
    return loss, items, asg, gs


def _assert_same_run(a, b, what):
    """out, items, the assignment (assign_gt, assign_score and what is derived from them), status and every gradient element"""
    assert _same(a[0], b[0]) and _same(a[1], b[1]), what
    for k in ("target_gt", "weight", "fg", "target_scores", "target_bboxes", "status"):
        assert _same(a[2][k], b[2][k]), (what, k)
    for l, (x, y) in enumerate(zip(a[3], b[3])):
        assert _same(x, y), (what, "gradient", l)


_MEMO = {}


def _case(name):
    """A stored case of tests/det_oracle.py or tests/det_cases.py, loaded once and never written to."""
    if name not in _MEMO:
        c = O.load_case(name) if name in O.CASES else DC.load(name)
        c["upstream"] = tuple(float(u) for u in c["upstream"])
        _MEMO[name] = c
    return _MEMO[name]


STORED = list(O.CASES) + list(DC.CASES)


@DTYPES
@pytest.mark.parametrize("name", STORED)
def test_criterion_on_every_stored_case_equals_the_nchw_run(built_lib, name, dtype):
    c = _case(name)
    for up in (UP1, c["upstream"]):
        want = _det(c["feats"], c["labels"], c["kw"], up, dtype)
        got = _det(c["feats"], c["labels"], c["kw"], up, dtype, cl=True)
        _assert_same_run(got, want, (name, up))
        assert all(g.dtype == dtype and g.is_contiguous(memory_format=CL) for g in got[3])
    assert int(got[2]["status"]) == 0


@pytest.mark.parametrize("name", STORED)
def test_criterion_fp32_against_the_fp64_oracle(built_lib, name):
    """The channels_last run itself at the bars of tests/test_gpu_det.py (its cases) and tests/test_gpu_det_shapes.py (theirs)"""
    c = _case(name)
    o = O.oracle(c["feats"], *c["labels"], **c["kw"])
    for key, up in (("g1", UP1), ("gnu", c["upstream"])):
        loss, items, asg, gs = _det(c["feats"], c["labels"], c["kw"], up, cl=True)
        if name in O.CASES:
            O.check("loss", loss, c["loss_f64"], o["terms"]["loss"], EPS[F32], O.K["loss"])
            O.check("items", items, c["items_f64"], o["terms"]["loss"] / int(c["B"]), EPS[F32], O.K["loss"])
            for l, g in enumerate(gs):
                O.check(f"{key}[{l}]", g, c[f"{key}_{l}_f64"], O.grad_terms(o["terms"], l, up), EPS[F32], O.K["grad"])
        else:
            _check_against(o, c, loss, items, gs, up, EPS[F32], c["loss_f64"], c["items_f64"])
    if name in O.CASES:
        _check_assignment_stored(asg, o, c["target_scores_f64"], EPS[F32])
    else:
        _check_assignment(asg, o, c["target_scores_f64"])


# ---- the post-process -------------------------------------------------------------------------------------------------------------------
def _post(feats, kw, dtype=F32, cl=False, **over):
    from mga_yolo_amd import detect_postprocess
    xs = [f.cuda().to(dtype) for f in feats]
    out = detect_postprocess([_cl(x) for x in xs] if cl else xs, **dict(kw, **over))
    torch.cuda.synchronize()
    return out


VARIANTS = [dict(multi_label=m, agnostic=a, conf_thres=conf) for m in (False, True) for a in (False, True) for conf in (0.25, 0.001)]


def _assert_same_post(feats, kw, dtype, what):
    for over in VARIANTS:
        want, got = _post(feats, kw, dtype, **over), _post(feats, kw, dtype, cl=True, **over)
        for k, x, y in zip(("dets", "count", "keep"), got, want):
            assert _same(x, y), (what, over, k)


@DTYPES
@pytest.mark.parametrize("name", NC.NAMES)
def test_post_process_on_every_case_equals_the_nchw_run(name, dtype):
    c = NC.load(name)
    _assert_same_post(c["feats"], c["kw"], dtype, name)
    dets, count, keep = _post(c["feats"], c["kw"], dtype, cl=True)          # the case's own arguments: the stored answer's
    if dtype == F32:
        NC.check(f"channels_last {name}", dets, count, keep, NC.oracle(name))


# ---- shapes the layout can break -----------------------------------------------------------------------------------------------------------
# name: (seed, B, (H, W) of the image, strides, nc).  A = the levels' cells; kBlock = 256 anchors of (B, A) a workgroup
SHAPES = {
    "nc1_pitch65": (101, 2, (64, 64), (8, 16, 32), 1),
    "nc3_pitch67": (102, 2, (64, 64), (8, 16, 32), 3),
    "nc5_pitch69": (103, 2, (64, 64), (8, 16, 32), 5),
    "nc80_pitch144": (104, 3, (128, 128), (8, 16, 32), 80),              # three rounds through LDS a workgroup, B * A = 1008
    "top_1x1": (105, 3, (32, 32), (8, 16, 32), 3),                       # levels 4 x 4, 2 x 2, 1 x 1: B * A = 63, nine segments in one workgroup
    "ragged_96x64": (106, 3, (96, 64), (8, 16, 32), 5),                  # B * A = 378: the second workgroup starts inside image 0's level 1
    "ba_256": (107, 1, (128, 128), (8,), 2),                             # B * A = 256: exactly one workgroup
    "ba_512": (108, 2, (128, 128), (8,), 1),
    "ba_257": (109, 1, (128, 128), (8, 128), 2),                         # one more: a second workgroup of one anchor, the 1 x 1 level's
}


def _shape_case(name):
    if name not in _MEMO:
        seed, B, (H, W), strides, nc = SHAPES[name]
        g = torch.Generator().manual_seed(seed)
        feats = [1.5 * torch.randn(B, 64 + nc, H // s, W // s, generator=g) for s in strides]
        rows = []
        for b in range(B):
            for _ in range(3):
                cx, cy = torch.rand(2, generator=g).tolist()
                w, h = (0.15 + 0.5 * torch.rand(2, generator=g)).tolist()
                rows.append((float(b), float(torch.randint(0, nc, (1,), generator=g)), cx, cy, w, h))
        r = torch.tensor(rows, dtype=F32)
        _MEMO[name] = dict(feats=feats, labels=(r[:, 0].clone(), r[:, 1].clone(), r[:, 2:].clone()),
                           kw=dict(nc=nc, strides=strides, gains=DC.GAINS, topk=10), A=sum((H // s) * (W // s) for s in strides), B=B)
    return _MEMO[name]


def test_the_shapes_are_what_they_are_named_for():
    ba = {n: _shape_case(n)["B"] * _shape_case(n)["A"] for n in SHAPES}
    assert ba["ragged_96x64"] == 378 and ba["ba_256"] == 256 and ba["ba_512"] == 512 and ba["ba_257"] == 257 and ba["top_1x1"] == 63
    assert tuple(_shape_case("top_1x1")["feats"][2].shape[2:]) == (1, 1) and tuple(_shape_case("ba_257")["feats"][1].shape[2:]) == (1, 1)
    assert [64 + SHAPES[n][4] for n in list(SHAPES)[:4]] == [65, 67, 69, 144]


@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_criterion_on_the_added_shapes(built_lib, name, dtype):
    c = _shape_case(name)
    for up in (UP1, DC.UPSTREAM):
        want = _det(c["feats"], c["labels"], c["kw"], up, dtype)
        got = _det(c["feats"], c["labels"], c["kw"], up, dtype, cl=True)
        _assert_same_run(got, want, (name, up))
        assert all(g.is_contiguous(memory_format=CL) for g in got[3])
    assert int(want[2]["fg"].sum()) > 0 and bool(torch.isfinite(want[0]).all())


@DTYPES
@pytest.mark.parametrize("name", list(SHAPES))
def test_post_process_on_the_added_shapes(name, dtype):
    c = _shape_case(name)
    kw = dict(NC.DEFAULTS, nc=c["kw"]["nc"], strides=c["kw"]["strides"])
    _assert_same_post(c["feats"], kw, dtype, name)
    assert int(_post(c["feats"], kw, dtype, cl=True)[1].sum()) > 0


# ---- bounds: levels inside larger buffers ---------------------------------------------------------------------------------------------------
GUARD, FILL = 37, -7.0                                           # elements before and after a level; their value (exact in every element type)


def _carved(values, off, fill=FILL):
    """(buffer, NHWC view): `values` (B, C, H, W) laid out channels_last from element `off` of a buffer of GUARD + n + GUARD sentinels"""
    B, Cc, H, W = values.shape
    n = values.numel()
    buf = torch.full((off + n + GUARD,), fill, dtype=values.dtype, device=values.device)
    view = buf[off:off + n].view(B, H, W, Cc).permute(0, 3, 1, 2)
    view.copy_(values)
    return buf, view


def _guards_intact(buf, off, n, fill=FILL):
    return bool((buf[:off] == fill).all()) and bool((buf[off + n:] == fill).all())


@DTYPES
@pytest.mark.parametrize("name", ["nc1_pitch65", "nc80_pitch144", "top_1x1", "ragged_96x64", "ba_257"])
def test_no_byte_outside_a_level_is_written_and_every_gradient_is(built_lib, name, dtype):
    """Every level and every gradient level starts at an odd element of its buffer (3, 5, 7, ...: never 16-byte aligned in fp32, 2 bytes
    off a 4-byte boundary in half precision).  After forward, backward and the post-process the sentinels around all of them stand, no NaN
    the gradient buffers were filled with survives, and the results are the NCHW run's."""
    from mga_yolo_amd import detloss, detect_postprocess, _lib
    c = _shape_case(name)
    kw = c["kw"]
    want = _det(c["feats"], c["labels"], kw, DC.UPSTREAM, dtype)
    vals = [f.to(dtype).cuda() for f in c["feats"]]
    offs = [3 + 2 * l for l in range(len(vals))]
    fb, fv = zip(*(_carved(v, o) for v, o in zip(vals, offs)))
    gb, gv = zip(*(_carved(torch.full_like(v, float("nan")), o + 2) for v, o in zip(vals, offs)))
    assert all(v.is_contiguous(memory_format=CL) and v.data_ptr() % 16 != 0 for v in fv + gv)
    b_, c_, x_ = (t.cuda() for t in c["labels"])
    up = torch.tensor(DC.UPSTREAM, dtype=F32, device="cuda")
    m_cap = int(torch.bincount(b_.long()).max())
    st = detloss._DetState(list(fv), kw["strides"], kw["nc"], kw["topk"], m_cap, kw["gains"], b_, c_, x_, None, g_feats=list(gv), upstream=up,
                           flags=_lib.MAPS_LAYOUT_NHWC)
    st.forward(vals[0].device)
    st.backward(vals[0].device)
    torch.cuda.synchronize()
    for l, v in enumerate(vals):
        assert _guards_intact(fb[l], offs[l], v.numel()) and _guards_intact(gb[l], offs[l] + 2, v.numel()), l
        assert _same(fv[l], v), l                                # the maps themselves are only read
        assert not bool(torch.isnan(want[3][l]).any()) and not bool(torch.isnan(gv[l]).any()), l
        assert _same(gv[l], want[3][l]), l
    assert _same(st.out, want[0]) and _same(st.items, want[1]) and int(st.status) == 0
    assert _same(st.assign_gt.long(), want[2]["target_gt"]) and _same(st.assign_score, want[2]["weight"])
    pk = dict(NC.DEFAULTS, nc=kw["nc"], strides=kw["strides"], conf_thres=0.001, multi_label=True)
    got = detect_postprocess(list(fv), **pk)
    torch.cuda.synchronize()
    for x, y in zip(got, _post(c["feats"], pk, dtype)):
        assert _same(x, y)
    assert all(_guards_intact(fb[l], offs[l], v.numel()) for l, v in enumerate(vals))


# ---- the poisoned call ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_more_rows_than_m_cap_poisons_the_call_in_either_layout(built_lib, dtype):
    c = _case("b2_64_nc1")                                       # image 0 has two boxes: m_cap + 1 rows at m_cap = 1
    runs = [_det(c["feats"], c["labels"], c["kw"], UP1, dtype, cl=cl, m_cap=1) for cl in (False, True)]
    for loss, items, asg, gs in runs:
        assert int(asg["status"]) == 1
        assert bool(torch.isnan(loss).all()) and bool(torch.isnan(items).all()) and all(bool(torch.isnan(g).all()) for g in gs)
    _assert_same_run(runs[1], runs[0], "poisoned")
    clean = _det(c["feats"], c["labels"], c["kw"], UP1, dtype, cl=True, m_cap=2)
    assert int(clean[2]["status"]) == 0 and bool(torch.isfinite(clean[0]).all())


# ---- no copy ---------------------------------------------------------------------------------------------------------------------------------
def test_channels_last_maps_are_read_and_their_gradients_written_in_place(built_lib, monkeypatch):
    from mga_yolo_amd import _lib, detect_postprocess, detection_loss, detloss, detpost
    seen = []

    def spy(real):
        def call(name, dev, desc, *rest):
            D = desc._obj
            seen.append((name, rest, [D.feats[l] for l in range(4)], [D.g_feats[l] for l in range(4)] if hasattr(D, "g_feats") else None))
            return real(name, dev, desc, *rest)
        return call
    monkeypatch.setattr(detloss, "call", spy(detloss.call))
    monkeypatch.setattr(detpost, "call", spy(detpost.call))
    c = _shape_case("nc3_pitch67")
    xs = [_cl(f.cuda()).requires_grad_(True) for f in c["feats"]]
    loss, _ = detection_loss(xs, *(t.cuda() for t in c["labels"]), **c["kw"])
    gs = torch.autograd.grad(loss.sum(), xs)
    detect_postprocess([x.detach() for x in xs], nc=c["kw"]["nc"], strides=c["kw"]["strides"])
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == ["mgamaps_det_forward", "mgamaps_det_backward", "mgamaps_nms_run"]
    ptrs = [x.data_ptr() for x in xs] + [None]
    for name, rest, feats, g_feats in seen:
        assert rest == (_lib.MAPS_LAYOUT_NHWC,) and feats == ptrs, name
    assert seen[1][3] == [g.data_ptr() for g in gs] + [None]
    assert all(g.is_contiguous(memory_format=CL) and not g.is_contiguous() and g.stride() == x.stride() for g, x in zip(gs, xs))
    # NCHW maps, and levels of two layouts (the copy path), go with flags = 0
    del seen[:]
    mixed = [xs[0].detach(), c["feats"][1].cuda(), xs[2].detach()]
    detect_postprocess(mixed, nc=c["kw"]["nc"], strides=c["kw"]["strides"])
    detect_postprocess([f.cuda() for f in c["feats"]], nc=c["kw"]["nc"], strides=c["kw"]["strides"])
    assert [s[1] for s in seen] == [(0,), (0,)] and seen[0][2][0] != mixed[0].data_ptr() and seen[0][2][1] == mixed[1].data_ptr()


# ---- the plans -------------------------------------------------------------------------------------------------------------------------------
def test_both_plans_channels_last_in_one_captured_graph(built_lib):
    from mga_yolo_amd import DetLossPlan, DetPostPlan
    c = _shape_case("ragged_96x64")
    kw = c["kw"]
    bidx, cls, bb = (t.cuda() for t in c["labels"])
    shapes = [(f.shape[0], f.shape[2], f.shape[3]) for f in c["feats"]]
    up = torch.tensor(DC.UPSTREAM, dtype=F32).cuda()
    pk = dict(strides=kw["strides"], conf_thres=0.25, multi_label=True)
    plans = {}
    for cl in (True, False):
        loss = DetLossPlan.create(shapes, kw["nc"], n_cap=12, m_cap=4, dtype=F32, g_out=up, strides=kw["strides"], gains=kw["gains"], topk=kw["topk"],
                                  channels_last=cl)
        post = DetPostPlan.create(shapes, kw["nc"], feats=loss.feats, channels_last=cl, **pk)
        loss.set_labels(bidx, cls, bb)
        plans[cl] = (loss, post)
        assert all(f.is_contiguous(memory_format=CL) == cl or f.shape[2:] == (1, 1) for f in loss.feats + loss.g_feats)
        with pytest.raises(ValueError):
            DetPostPlan.create(shapes, kw["nc"], feats=loss.feats, channels_last=not cl, **pk)
    loss, post = plans[True]

    def step():
        loss.forward(); loss.backward(); post.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    outs = []
    for t, n in enumerate((9, 5)):
        g = torch.Generator().manual_seed(300 + t)
        feats = [f + 0.05 * torch.randn(f.shape, generator=g) for f in c["feats"]]
        for pl, _ in plans.values():
            for dst, f in zip(pl.feats, feats):
                dst.copy_(f)
            pl.n.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        loss.check_status(); post.check_status()
        nl, npost = plans[False]
        nl.forward(); nl.backward(); npost.run()
        torch.cuda.synchronize()
        eager = _det(feats, tuple(x[:n].cpu() for x in (bidx, cls, bb)), kw, DC.UPSTREAM, cl=True, m_cap=4)
        assert _same(loss.out, eager[0]) and _same(loss.items, eager[1]) and _same(loss.out, nl.out) and _same(loss.items, nl.items), n
        for l in range(len(feats)):
            assert _same(loss.g_feats[l], eager[3][l]) and _same(loss.g_feats[l], nl.g_feats[l]), (n, l)
        assert _same(loss.assign_gt, nl.assign_gt) and _same(loss.assign_score, nl.assign_score), n
        ep = _post(feats, dict(NC.DEFAULTS, nc=kw["nc"], **pk), cl=True)
        for x, y, z in zip((post.dets, post.count, post.keep), ep, (npost.dets, npost.count, npost.keep)):
            assert _same(x, y) and _same(x, z), n
        outs.append(loss.out.clone())
    assert not _same(outs[0], outs[1]) and int(post.count.sum()) > 0
