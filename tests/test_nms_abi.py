"""include/mganms.h without a GPU: every refusal before a launch, the size query, and install(nms=True) / uninstall() on a stub of the
reference's ultralytics.utils.ops.  The header against the binding is tests/test_abi_headers.py's."""
import ctypes as C
import re
import sys
import types

import pytest

from abi_header import FAKE as P, a16

# B = 2, 64 x 64 image: 84 anchors, cand_cap = 84: the counters, the keys, the boxes
WS_BYTES = a16(2 * 4) + a16(2 * 84 * 8) + a16(2 * 84 * 16)


def _desc(_lib, from_pred=False, **over):
    D = _lib.NmsDesc()
    if from_pred:
        D.pred, D.n_levels, D.A = P + 0x50000, 0, 84
    else:
        for l, (h, s) in enumerate(((8, 8), (4, 16), (2, 32))):
            D.feats[l], D.H[l], D.W[l], D.stride[l] = P + 0x10000 * (l + 1), h, h, s
        D.n_levels, D.A = 3, 0
    D.B, D.nc, D.dtype, D.max_det, D.max_nms, D.flags = 2, 3, _lib.F32, 300, 30000, 0
    D.conf_thres, D.iou_thres, D.cand_cap, D.reserved = 0.25, 0.45, 84, 0
    for i, name in enumerate(("dets", "count", "keep", "status")):
        setattr(D, name, P + 0x100000 + 0x1000 * i)
    D.ws, D.ws_bytes = P + 0x200000, WS_BYTES
    for k, v in over.items():
        m = re.fullmatch(r"(feats|H|W|stride)(\d)", k)
        if m:
            getattr(D, m.group(1))[int(m.group(2))] = v
        else:
            setattr(D, k, v)
    return D


CASES = [  # (what, from pred, overrides, code)
    ("n_levels -1", False, dict(n_levels=-1), -5), ("n_levels 5", False, dict(n_levels=5), -5),
    ("unknown dtype", False, dict(dtype=3), -3), ("negative dtype", True, dict(dtype=-1), -3),
    ("feats and pred", False, dict(pred=P + 0x50000), -7), ("pred and a feature map", True, dict(feats1=P), -7),
    ("conf > 1", False, dict(conf_thres=1.5), -7), ("conf < 0", False, dict(conf_thres=-0.1), -7), ("conf NaN", False, dict(conf_thres=float("nan")), -7),
    ("iou > 1", True, dict(iou_thres=1.01), -7), ("iou NaN", False, dict(iou_thres=float("nan")), -7),
    ("max_det 0", False, dict(max_det=0), -7), ("max_nms 0", False, dict(max_nms=0), -7), ("cand_cap 0", False, dict(cand_cap=0), -7),
    ("unknown flag", False, dict(flags=4), -7), ("reserved set", False, dict(reserved=1), -7),
    ("descending strides", False, dict(stride1=4), -7), ("repeated stride", False, dict(stride2=16), -7), ("stride 0", False, dict(stride0=0), -7),
    ("B 0", False, dict(B=0), -2), ("nc 0", True, dict(nc=0), -2), ("H 0", False, dict(H1=0), -2), ("A < 0", True, dict(A=-1), -2),
    ("pred without A", True, dict(A=0), -2), ("A not the levels' sum", False, dict(A=85), -2),
    ("B * A = 2^31", False, dict(B=1 << 17, H0=128, W0=128), -2), ("A * nc = 2^31", True, dict(A=1 << 20, nc=1 << 11), -2),
    ("feats NULL", False, dict(feats1=None), -1), ("pred NULL", True, dict(pred=None), -1), ("dets NULL", False, dict(dets=None), -1),
    ("count NULL", True, dict(count=None), -1), ("keep NULL", False, dict(keep=None), -1), ("status NULL", False, dict(status=None), -1),
    ("ws NULL", False, dict(ws=None), -1),
    ("fp32 feats misaligned", False, dict(feats0=P + 0x10002), -4), ("fp16 feats misaligned", False, dict(dtype=1, feats2=P + 0x30001), -4),
    ("pred misaligned", True, dict(pred=P + 0x50002), -4), ("dets misaligned", False, dict(dets=P + 0x100002), -4),
    ("keep misaligned", True, dict(keep=P + 0x102001), -4), ("ws misaligned", False, dict(ws=P + 0x200008), -4),
    ("ws too small", False, dict(ws_bytes=WS_BYTES - 1), -6), ("ws too small, pred", True, dict(ws_bytes=WS_BYTES - 1), -6),
]


@pytest.mark.parametrize("what,pred,over,code", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, pred, over, code):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    assert lib.mganms_run(C.byref(_desc(_lib, pred, **over)), None) == code, what
    assert lib.mgacbam_last_error(), what
    assert lib.mganms_run(None, None) == -1


def test_size_query(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    assert lib.mganms_ws_bytes(C.byref(_desc(_lib))) == WS_BYTES == _lib.nms_ws_bytes(_desc(_lib)) == _lib.nms_ws_bytes(_desc(_lib, True))
    assert lib.mganms_ws_bytes(C.byref(_desc(_lib, ws=None, ws_bytes=0, feats0=None, dets=None))) == WS_BYTES     # buffers do not enter the size
    assert lib.mganms_ws_bytes(C.byref(_desc(_lib, True, pred=None))) == WS_BYTES
    assert lib.mganms_ws_bytes(C.byref(_desc(_lib, cand_cap=84 * 3, flags=_lib.NMS_MULTI_LABEL))) == a16(8) + a16(2 * 252 * 8) + a16(2 * 252 * 16)
    assert lib.mganms_ws_bytes(C.byref(_desc(_lib, B=3))) > WS_BYTES
    for over in (dict(n_levels=5), dict(dtype=7), dict(conf_thres=2.0), dict(stride1=8), dict(B=0), dict(cand_cap=0), dict(flags=8)):
        assert lib.mganms_ws_bytes(C.byref(_desc(_lib, **over))) == 0 and lib.mgacbam_last_error(), over
        with pytest.raises(RuntimeError):
            _lib.nms_ws_bytes(_desc(_lib, **over))
    assert lib.mganms_ws_bytes(None) == 0


def test_fill_sets_every_field():
    import torch
    from mga_yolo_amd import _lib
    from mga_yolo_amd._binding import fill_nms
    feats = [torch.zeros(2, 67, h, h) for h in (8, 4, 2)]
    outs = (torch.zeros(2, 7, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 7, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    D = _lib.NmsDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_nms(D, feats, None, (8, 16, 32), 3, 0.3, 0.5, 7, 40, _lib.NMS_AGNOSTIC, 84, *outs)
    assert [D.feats[l] for l in range(4)] == [f.data_ptr() for f in feats] + [None] and D.pred is None
    assert (list(D.H), list(D.W), list(D.stride)) == ([8, 4, 2, 0], [8, 4, 2, 0], [8, 16, 32, 0])
    assert (D.n_levels, D.A, D.B, D.nc, D.dtype, D.max_det, D.max_nms, D.flags, D.cand_cap, D.reserved) == (3, 0, 2, 3, _lib.F32, 7, 40, 2, 84, 0)
    assert abs(D.conf_thres - 0.3) < 1e-7 and abs(D.iou_thres - 0.5) < 1e-7 and D.ws is None and D.ws_bytes == 0
    assert (D.dets, D.count, D.keep, D.status) == tuple(t.data_ptr() for t in outs)
    pred = torch.zeros(2, 7, 84, dtype=torch.float16)
    ws = torch.zeros(64, dtype=torch.uint8)
    fill_nms(D, None, pred, (), 3, 0.3, 0.5, 7, 40, 0, 84, *outs, ws=ws)
    assert [D.feats[l] for l in range(4)] == [None] * 4 and D.pred == pred.data_ptr() and (D.n_levels, D.A, D.dtype) == (0, 84, _lib.F16)
    assert (D.ws, D.ws_bytes) == (ws.data_ptr(), 64)


@pytest.fixture
def stub_ops():
    """Stand-ins for the two module objects the reference makes of ultralytics/utils/ops.py, and one module that merely has the name."""
    def ref_nms(*a, **k):
        return "reference"
    made = {}
    for name in ("ultralytics", "ultralytics.utils", "ultralytics.utils.ops", "mga_yolo.external.ultralytics.ultralytics.utils.ops"):
        if name not in sys.modules:
            made[name] = sys.modules[name] = types.ModuleType(name)
    for name in ("ultralytics.utils.ops", "mga_yolo.external.ultralytics.ultralytics.utils.ops"):
        if name in made:
            made[name].non_max_suppression = ref_nms
    if not made.keys() >= {"ultralytics.utils.ops", "mga_yolo.external.ultralytics.ultralytics.utils.ops"}:
        for name in made:
            del sys.modules[name]
        pytest.skip("the reference itself is importable here: the stub would shadow it")
    yield [sys.modules["ultralytics.utils.ops"], sys.modules["mga_yolo.external.ultralytics.ultralytics.utils.ops"]], ref_nms
    for name in made:
        sys.modules.pop(name, None)


def test_install_nms_is_opt_in_and_uninstall_restores(stub_ops):
    import mga_yolo_amd
    from mga_yolo_amd import detpost
    mods, ref_nms = stub_ops
    try:
        mga_yolo_amd.install()                                  # the default leaves the post-process alone
        assert all(m.non_max_suppression is ref_nms for m in mods)
        patched = mga_yolo_amd.install(nms=True)
        assert all(m.non_max_suppression is detpost.non_max_suppression for m in mods)
        assert {"ultralytics.utils.ops", "mga_yolo.external.ultralytics.ultralytics.utils.ops"} <= set(patched)
        assert mga_yolo_amd.install(nms=True) is not None       # a second call rebinds nothing and records nothing to undo twice
    finally:
        mga_yolo_amd.uninstall()
    assert all(m.non_max_suppression is ref_nms for m in mods)
