"""CPU-side checks of the detection criterion (include/mgadet.h; the header against the binding is tests/test_abi_headers.py's): the size
query, every refusal -- each returned, with its message, before anything is launched (there is no GPU here) -- and the host path of
mga_yolo_amd.detloss against the reference's stored results and the fp64 oracle, under both tie orders."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import det_oracle as O
from abi_header import FAKE as P, a16

EPS32 = float(np.finfo(np.float32).eps)

# B = 2, 64 x 64 image, m_cap = 4: 84 anchors, 8 slots, one workgroup of partials
WS_BYTES = 2 * a16(8 * 4) + 3 * a16(8 * 16 * 4) + 2 * a16(2 * 4) + a16(3 * 4) + a16(4 * 4)


def _desc(_lib, **over):
    D = _lib.DetDesc()
    for l, (h, s) in enumerate(((8, 8), (4, 16), (2, 32))):
        D.feats[l], D.g_feats[l], D.H[l], D.W[l], D.stride[l] = P + 0x10000 * (l + 1), P + 0x10000 * (l + 5), h, h, s
    D.n_levels, D.B, D.nc, D.reg_max, D.dtype, D.topk, D.n_cap, D.m_cap = 3, 2, 3, 16, _lib.F32, 10, 6, 4
    D.gains[0], D.gains[1], D.gains[2] = 7.5, 0.5, 1.5
    for i, name in enumerate(("batch_idx", "cls", "bboxes", "n", "assign_gt", "assign_score", "out", "items", "status", "upstream")):
        setattr(D, name, P + 0x100000 + 0x1000 * i)
    D.ws, D.ws_bytes = P + 0x200000, WS_BYTES
    for k, v in over.items():
        m = re.fullmatch(r"(feats|g_feats|H|W|stride)(\d)", k)
        if m:
            getattr(D, m.group(1))[int(m.group(2))] = v
        else:
            setattr(D, k, v)
    return D


CASES = [  # (what, overrides, code of mgadet_forward, code of mgadet_backward)
    ("n_levels 0", dict(n_levels=0), -5, -5), ("n_levels 5", dict(n_levels=5), -5, -5),
    ("unknown dtype", dict(dtype=3), -3, -3), ("negative dtype", dict(dtype=-1), -3, -3),
    ("reg_max 8", dict(reg_max=8), -7, -7), ("reg_max 1", dict(reg_max=1), -7, -7),
    ("topk 17", dict(topk=17), -7, -7), ("topk 0", dict(topk=0), -7, -7),
    ("m_cap 0", dict(m_cap=0), -7, -7), ("m_cap 257", dict(m_cap=257), -7, -7),
    ("reserved set", dict(reserved=1), -7, -7),
    ("descending strides", dict(stride1=4), -7, -7), ("repeated stride", dict(stride2=16), -7, -7), ("stride 0", dict(stride0=0), -7, -7),
    ("B 0", dict(B=0), -2, -2), ("nc 0", dict(nc=0), -2, -2), ("H 0", dict(H1=0), -2, -2), ("n_cap < 0", dict(n_cap=-1), -2, -2),
    ("B * A = 2^31", dict(B=1 << 17, H0=128, W0=128), -2, -2),
    ("feats NULL", dict(feats1=None), -1, -1), ("g_feats NULL", dict(g_feats2=None), None, -1),
    ("labels NULL", dict(cls=None), -1, -1), ("out NULL", dict(out=None), -1, -1), ("status NULL", dict(status=None), -1, -1),
    ("assign NULL", dict(assign_gt=None), -1, -1), ("ws NULL", dict(ws=None), -1, -1), ("upstream NULL", dict(upstream=None), None, -1),
    ("fp32 feats misaligned", dict(feats0=P + 0x10002), -4, -4), ("fp16 feats misaligned", dict(dtype=1, feats2=P + 0x30001), -4, -4),
    ("labels misaligned", dict(bboxes=P + 0x102002), -4, -4), ("n misaligned", dict(n=P + 0x103001), -4, -4),
    ("ws misaligned", dict(ws=P + 0x200008), -4, -4), ("g_feats misaligned", dict(g_feats0=P + 0x50002), None, -4),
    ("ws too small", dict(ws_bytes=WS_BYTES - 1), -6, -6),
]


@pytest.mark.parametrize("what,over,fwd,bwd", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, over, fwd, bwd):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    D = _desc(_lib, **over)
    for fn, want in ((lib.mgadet_forward, fwd), (lib.mgadet_backward, bwd)):
        if want is None:
            continue                                         # the call would get past its checks and launch: not on this machine
        assert fn(C.byref(D), None) == want, what
        assert lib.mgacbam_last_error(), what
    assert {_lib.E_ARG, _lib.E_SIZE, _lib.E_ALIGN, _lib.E_NULL, _lib.E_SHAPE, _lib.E_DTYPE, _lib.E_LEVELS} == {-7, -6, -4, -1, -2, -3, -5}


def test_size_query(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    assert lib.mgadet_ws_bytes(C.byref(_desc(_lib))) == WS_BYTES == _lib.det_ws_bytes(_desc(_lib))
    assert lib.mgadet_ws_bytes(C.byref(_desc(_lib, ws=None, ws_bytes=0, feats0=None))) == WS_BYTES       # buffers do not enter the size
    # more anchors -> more partials; more slots -> more candidates
    assert lib.mgadet_ws_bytes(C.byref(_desc(_lib, H0=80, W0=80))) > WS_BYTES
    assert lib.mgadet_ws_bytes(C.byref(_desc(_lib, m_cap=8))) > WS_BYTES
    for over in (dict(reg_max=8), dict(topk=17), dict(n_levels=0), dict(dtype=7), dict(m_cap=300), dict(stride1=8), dict(B=0)):
        assert lib.mgadet_ws_bytes(C.byref(_desc(_lib, **over))) == 0 and lib.mgacbam_last_error(), over
        with pytest.raises(RuntimeError):
            _lib.det_ws_bytes(_desc(_lib, **over))
    assert lib.mgadet_ws_bytes(None) == 0


# ---- the host path ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=O.CASES)
def case(request):
    c = O.load_case(request.param)
    c["name"] = request.param
    c["oracle"] = O.oracle(c["feats"], *c["labels"], **c["kw"])
    return c


def _weight_positive(c):
    return torch.from_numpy(c["target_scores_f64"]).sum(-1) > 0


def test_oracle_equals_the_reference_fp64_run(case):
    """The fp64 oracle against the reference's own fp64 run: rounding apart (1e-9 relative to each quantity's terms) they are one function."""
    c, o = case, case["oracle"]
    eps = 1e-9 / O.K["loss"]
    O.check("loss", o["loss"], c["loss_f64"], o["terms"]["loss"], eps, O.K["loss"])
    O.check("items", o["items"], c["items_f64"], o["terms"]["loss"] / int(c["B"]), eps, O.K["loss"])
    O.check("target_scores", o["target_scores"], c["target_scores_f64"], o["terms"]["target_scores"], 1e-9 / O.K["target_scores"], O.K["target_scores"])
    for key in ("g1", "gnu"):
        up = (1.0, 1.0, 1.0) if key == "g1" else c["upstream"]
        for l in range(3):
            O.check(f"{key}[{l}]", O.grads(o, l, up), c[f"{key}_{l}_f64"], O.grad_terms(o["terms"], l, up), 1e-9 / O.K["grad"], O.K["grad"])
    w = _weight_positive(c)
    assert torch.equal(o["fg"][w], torch.from_numpy(c["fg_mask_f64"])[w]) and bool(o["fg"][w].all())
    assert torch.allclose(o["target_bboxes"][w], torch.from_numpy(c["target_bboxes_f64"])[w], rtol=0, atol=1e-9)
    assert torch.equal(o["weight"] > 0, w)


def test_host_path_against_the_goldens(case):
    """mga_yolo_amd.detection_loss on host tensors (fp32 torch ops) against the reference's fp64 run, at the GPU tests' bars."""
    from mga_yolo_amd import detection_loss
    c, o = case, case["oracle"]
    for key in ("g1", "gnu"):
        up = torch.ones(3) if key == "g1" else torch.from_numpy(c["upstream"]).float()
        xs = [f.clone().requires_grad_(True) for f in c["feats"]]
        loss, items, asg = detection_loss(xs, *c["labels"], return_assignment=True, **c["kw"])
        O.check("loss", loss, c["loss_f64"], o["terms"]["loss"], EPS32, O.K["loss"])
        O.check("items", items, c["items_f64"], o["terms"]["loss"] / int(c["B"]), EPS32, O.K["loss"])
        assert not items.requires_grad
        gs = torch.autograd.grad((loss * up).sum(), xs, allow_unused=True)
        for l, g in enumerate(gs):
            g = torch.zeros_like(xs[l]) if g is None else g
            O.check(f"{key}[{l}]", g, c[f"{key}_{l}_f64"], O.grad_terms(o["terms"], l, up), EPS32, O.K["grad"])
    O.check("target_scores", asg["target_scores"], c["target_scores_f64"], o["terms"]["target_scores"], EPS32, O.K["target_scores"])
    w = _weight_positive(c)
    assert torch.equal(asg["fg"][w], torch.from_numpy(c["fg_mask_f64"])[w])
    assert torch.equal(asg["target_gt"][w], o["target_gt"][w])
    assert torch.allclose(asg["target_bboxes"][w].double(), torch.from_numpy(c["target_bboxes_f64"])[w], rtol=0, atol=1e-3)
    assert int(asg["status"]) == 0


def test_tie_order_does_not_reach_the_loss_or_the_gradients(case):
    """Ties of the metric broken to the HIGHEST anchor index instead: the foreground mask may differ, nothing weighted does."""
    c, lo = case, case["oracle"]
    hi = O.oracle(c["feats"], *c["labels"], lowest_first=False, **c["kw"])
    assert torch.equal(hi["loss"], lo["loss"]) and torch.equal(hi["target_scores"], lo["target_scores"])
    for i in range(3):
        for l in range(3):
            assert torch.equal(hi["comp_grads"][i][l], lo["comp_grads"][i][l])
    w = lo["weight"] > 0
    assert torch.equal(hi["fg"][w], lo["fg"][w]) and torch.equal(hi["target_gt"][w], lo["target_gt"][w])


def test_the_cases_hold_what_they_were_built_for():
    """The committed cases exercise the paths they name: a contested anchor, a top-k cut, the DFL clamp, exact edges, zero-weight positives."""
    o = {n: O.oracle(O.load_case(n)["feats"], *O.load_case(n)["labels"], **O.load_case(n)["kw"]) for n in ("b3_96x64_nc5", "b2_128_nc2", "b2_64_nc3")}
    big = O.load_case("b2_128_nc2")
    assert int(o["b2_128_nc2"]["fg"].sum()) > 0 and float(big["loss_f64"][2]) > 0
    assert int(O.load_case("empty")["batch_idx"].size) == 0 and not O.load_case("empty")["fg_mask_f64"].any()
    zero = O.load_case("b2_64_nc3")
    assert (np.abs(zero["bboxes"]).sum(1) == 0).any()                                      # the all-zero label row
    assert not (o["b2_64_nc3"]["target_gt"] == 1).any() and not (o["b2_64_nc3"]["target_gt"] == 2).any()   # it, and the box without a centre
    assert not (o["b3_96x64_nc5"]["target_gt"][1] >= 0).any()                                 # the image without a box
    # exact ties of the metric: positives of weight 0, two of them handed to slot 0 whose box does not hold them; the reference's own
    # order of equal metrics gives another foreground mask, at anchors of weight 0 only
    ties = O.load_case("ties")
    t = O.oracle(ties["feats"], *ties["labels"], **ties["kw"])
    zero = t["fg"] & (t["weight"] == 0)
    assert int(zero.sum()) >= 2 and (t["target_gt"][zero] == 0).any()
    other = torch.from_numpy(ties["fg_mask_f64"]) != t["fg"]
    assert bool(other.any()) and not bool((other & (t["weight"] > 0)).any())


def test_v8_detection_loss_takes_the_reference_call_forms():
    from mga_yolo_amd import V8DetectionLoss, detection_loss
    c = O.load_case("b2_64_nc3")
    crit = V8DetectionLoss(c["kw"]["nc"], c["kw"]["strides"], c["kw"]["gains"], topk=c["kw"]["topk"])
    batch = dict(batch_idx=c["labels"][0], cls=c["labels"][1].view(-1, 1), bboxes=c["labels"][2])
    a = crit(c["feats"], batch)
    b = crit((torch.zeros(1), c["feats"]), batch)
    want = detection_loss(c["feats"], *c["labels"], **c["kw"])
    for got in (a, b):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[0].shape == (3,)
    with pytest.raises(ValueError):
        detection_loss([f[:, :-1] for f in c["feats"]], *c["labels"], **c["kw"])
