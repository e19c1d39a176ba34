"""include/ext/mgamaps.h without a GPU: the header against its record in mga_yolo_amd._lib.LAYOUT_HEADERS (read by tests/abi_header.py) and
against the built library; flags = 0 is mgadet_forward / mgadet_backward / mganms_run refusal for refusal (their own tables, imported);
MGAMAPS_LAYOUT_NHWC changes none of them and adds its own; the layout classifier of mga_yolo_amd.detmaps on host tensors; the plans' keyword."""
import ctypes as C
import inspect

import pytest
import torch

import abi_header as A
import test_det_abi as TD
import test_nms_abi as TN
from abi_header import FAKE as P
from mga_yolo_amd import _lib

NAME = "ext/mgamaps.h"
NHWC = 1
SYMBOLS = ["mgamaps_det_backward", "mgamaps_det_forward", "mgamaps_nms_run"]


def test_the_record_sits_in_a_table_of_its_own():
    REC = _lib.LAYOUT_HEADERS[NAME]
    assert list(_lib.LAYOUT_HEADERS) == [NAME]
    assert NAME not in _lib.HEADERS and NAME not in _lib.EXT_HEADERS and NAME not in _lib.METRIC_HEADERS and NAME not in _lib.ALL_HEADERS
    assert list(_lib.EXT_HEADERS) == ["ext/mgamatch.h"] and list(_lib.METRIC_HEADERS) == ["ext/mgaconfusion.h"]
    assert len(_lib.ALL_HEADERS) == len(_lib.HEADERS) + len(_lib.EXT_HEADERS) + len(_lib.METRIC_HEADERS)
    assert sorted(_lib.HEADERS) == A.headers()                    # one record per header directly under include/, as before
    assert "mgamaps.h" not in A.headers()
    h = A.read(NAME)
    assert h.includes == ("mgadet.h", "mganms.h") and not h.structs and REC.structs == {}
    text = open(A.INCLUDE + "/" + NAME).read()
    for word in ("SAME BITS", "does not depend on the layout", "to the element", "Refusals", "Not built", "non-NULL pred"):
        assert word in text, word


def test_symbols_declared_bound_and_exported(built_lib):
    REC = _lib.LAYOUT_HEADERS[NAME]
    declared = sorted(A.read(NAME).functions)
    assert declared == sorted(REC.symbols) == SYMBOLS
    raw = C.CDLL(built_lib)
    assert all(hasattr(raw, fn) for fn in declared)
    others = {fn for rec in _lib.ALL_HEADERS.values() for fn in rec.symbols}
    assert not set(declared) & others
    lib = _lib.load()                                              # load() binds the fourth table exactly as the others
    for fn, (res, args) in REC.symbols.items():
        assert getattr(lib, fn).restype is res and getattr(lib, fn).argtypes == args
    assert REC.symbols["mgamaps_det_forward"][1] == [C.POINTER(_lib.DetDesc), C.c_int32, C.c_void_p]
    assert REC.symbols["mgamaps_nms_run"][1] == [C.POINTER(_lib.NmsDesc), C.c_int32, C.c_void_p]


def test_constants_equal_the_mirrors():
    assert A.read(NAME).constants == _lib.LAYOUT_HEADERS[NAME].constants == dict(MGAMAPS_LAYOUT_NHWC=1)
    assert _lib.MAPS_LAYOUT_NHWC == NHWC


def test_the_headers_it_extends_gained_nothing():
    """mgadet.h and mganms.h: the symbols and constants tests/test_abi_headers.py pins, and a comment that names the new entry points"""
    assert sorted(A.read("mgadet.h").functions) == ["mgadet_backward", "mgadet_forward", "mgadet_ws_bytes"]
    assert sorted(A.read("mganms.h").functions) == ["mganms_run", "mganms_ws_bytes"]
    assert A.read("mgadet.h").constants == dict(MGADET_MAX_LEVELS=4, MGADET_MAX_TOPK=16, MGADET_MAX_GT=256)
    assert A.read("mganms.h").constants == dict(MGANMS_MAX_LEVELS=4, MGANMS_MULTI_LABEL=1, MGANMS_AGNOSTIC=2)
    for name in ("mgadet.h", "mganms.h"):
        text = open(A.INCLUDE + "/" + name).read()
        assert "Not built: channels_last" not in text and "channels_last features" not in text and "ext/mgamaps.h" in text


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, NHWC], ids=["flags0", "nhwc"])
@pytest.mark.parametrize("what,over,fwd,bwd", TD.CASES, ids=[c[0] for c in TD.CASES])
def test_the_criterion_s_refusals_in_either_layout(built_lib, what, over, fwd, bwd, flags):
    lib = _lib.load()
    D = TD._desc(_lib, **over)
    for new, old, want in ((lib.mgamaps_det_forward, lib.mgadet_forward, fwd), (lib.mgamaps_det_backward, lib.mgadet_backward, bwd)):
        if want is None:
            continue                                         # the call would get past its checks and launch: not on this machine
        assert old(C.byref(D), None) == want, what
        old_msg = lib.mgacbam_last_error().decode()
        assert new(C.byref(D), flags, None) == want, what
        msg = lib.mgacbam_last_error().decode()
        assert msg and msg.split(": ", 1)[1] == old_msg.split(": ", 1)[1], (what, msg, old_msg)      # the same refusal, under its own name
        assert msg.startswith("mgamaps_det_")


@pytest.mark.parametrize("flags", [0, NHWC], ids=["flags0", "nhwc"])
@pytest.mark.parametrize("what,pred,over,code", TN.CASES, ids=[c[0] for c in TN.CASES])
def test_the_post_process_s_refusals_in_either_layout(built_lib, what, pred, over, code, flags):
    lib = _lib.load()
    D = TN._desc(_lib, pred, **over)
    assert lib.mganms_run(C.byref(D), None) == code, what
    old_msg = lib.mgacbam_last_error().decode()
    assert lib.mgamaps_nms_run(C.byref(D), flags, None) == code, what
    msg = lib.mgacbam_last_error().decode()
    assert msg.startswith("mgamaps_nms_run: ") and msg.split(": ", 1)[1] == old_msg.split(": ", 1)[1], (what, msg, old_msg)
    assert lib.mgamaps_nms_run(None, flags, None) == -1 and lib.mgamaps_det_forward(None, flags, None) == -1


@pytest.mark.parametrize("flags", [2, -1, 3, 1 << 16])
def test_an_unknown_flag_is_refused(built_lib, flags):
    lib = _lib.load()
    for fn, D in ((lib.mgamaps_det_forward, TD._desc(_lib)), (lib.mgamaps_det_backward, TD._desc(_lib)), (lib.mgamaps_nms_run, TN._desc(_lib)),
                  (lib.mgamaps_nms_run, TN._desc(_lib, True))):
        assert fn(C.byref(D), flags, None) == _lib.E_ARG == -7
        assert b"flags=0x" in lib.mgacbam_last_error()


def test_nhwc_with_a_decoded_prediction_is_refused(built_lib):
    lib = _lib.load()
    D = TN._desc(_lib, True)                                       # a descriptor with no other fault: with flags = 0 it would launch
    assert lib.mgamaps_nms_run(C.byref(D), NHWC, None) == -7
    assert b"pred" in lib.mgacbam_last_error() and b"MGAMAPS_LAYOUT_NHWC" in lib.mgacbam_last_error()
    # ... and it comes last: another fault of the same descriptor is refused for what it is
    assert lib.mgamaps_nms_run(C.byref(TN._desc(_lib, True, ws_bytes=TN.WS_BYTES - 1)), NHWC, None) == -6
    assert lib.mgamaps_nms_run(C.byref(TN._desc(_lib, True, pred=P + 0x50002)), NHWC, None) == -4


def test_alignment_stays_to_the_element(built_lib):
    lib = _lib.load()
    odd = dict(dtype=_lib.F16, feats1=P + 0x20001)
    assert lib.mgamaps_det_forward(C.byref(TD._desc(_lib, **odd)), NHWC, None) == -4
    assert lib.mgamaps_det_backward(C.byref(TD._desc(_lib, dtype=_lib.F16, g_feats0=P + 0x50001)), NHWC, None) == -4
    assert lib.mgamaps_nms_run(C.byref(TN._desc(_lib, **odd)), NHWC, None) == -4
    assert b"aligned to its element (2 bytes)" in lib.mgacbam_last_error()
    # two bytes off a 16-byte boundary is aligned enough for fp16: the first refusal is then the one planted behind the alignment
    even = dict(dtype=_lib.F16, feats1=P + 0x20002)
    assert lib.mgamaps_det_forward(C.byref(TD._desc(_lib, ws_bytes=0, **even)), NHWC, None) == -6
    assert lib.mgamaps_nms_run(C.byref(TN._desc(_lib, ws_bytes=0, **even)), NHWC, None) == -6


def test_the_size_queries_serve_both_layouts(built_lib):
    """There is no layout in a descriptor, so one size: the exact size passes the workspace check under NHWC, one byte less does not"""
    lib = _lib.load()
    assert lib.mgadet_ws_bytes(C.byref(TD._desc(_lib))) == TD.WS_BYTES and lib.mganms_ws_bytes(C.byref(TN._desc(_lib))) == TN.WS_BYTES
    assert lib.mgamaps_det_forward(C.byref(TD._desc(_lib, ws_bytes=TD.WS_BYTES - 1)), NHWC, None) == -6
    assert lib.mgamaps_nms_run(C.byref(TN._desc(_lib, ws_bytes=TN.WS_BYTES - 1)), NHWC, None) == -6


# ---- the layout classifier ------------------------------------------------------------------------------------------------------------------
def _maps(sizes=((8, 8), (4, 4), (2, 2)), nc=3, B=2, dtype=torch.float32):
    return [torch.randn(B, 64 + nc, h, w).to(dtype) for h, w in sizes]


def _cl(ts):
    return [t.contiguous(memory_format=torch.channels_last) for t in ts]


def test_layout_classifier():
    from mga_yolo_amd.detmaps import device_maps, maps_layout
    f = _maps()
    assert maps_layout(f) == "nchw" and maps_layout(_cl(f)) == "nhwc"
    assert maps_layout([f[0], _cl(f)[1], f[2]]) == "copy" and maps_layout([_cl(f)[0], f[1], _cl(f)[2]]) == "copy"
    # a 1 x 1 level is both layouts at once: it goes with the others, whichever way it was made
    tiny = _maps(((4, 4), (2, 2), (1, 1)))
    assert tiny[2].is_contiguous() and tiny[2].is_contiguous(memory_format=torch.channels_last)
    assert maps_layout(tiny) == "nchw"
    assert maps_layout(_cl(tiny[:2]) + [tiny[2]]) == "nhwc" and maps_layout(_cl(tiny)) == "nhwc"
    assert maps_layout([tiny[2]]) == "nchw"                       # alone it is NCHW: today's path
    # views that are not dense: a channel slice of either layout, a spatial slice, an expanded batch
    wide = _maps(nc=4)
    assert maps_layout([w[:, :-1] for w in wide]) == "copy" and maps_layout([w[:, :-1] for w in _cl(wide)]) == "copy"
    assert maps_layout([w[:, :, :, :-1] for w in _cl(wide)]) == "copy"
    assert maps_layout([w[:1].expand(2, -1, -1, -1) for w in _cl(wide)]) == "copy"
    # element types the library has not, or two of them
    assert maps_layout(_cl(_maps(dtype=torch.float64))) == "copy"
    assert maps_layout([_cl(f)[0], _cl(f)[1].half(), _cl(f)[2]]) == "copy"
    assert maps_layout(_cl(_maps(dtype=torch.bfloat16))) == "nhwc" and maps_layout(_cl(_maps(dtype=torch.float16))) == "nhwc"
    # what a device call is handed: channels_last maps themselves, with the flag; everything else NCHW contiguous, without
    src = _cl(f)
    got, flags = device_maps(src)
    assert flags == 1 and all(g is s for g, s in zip(got, src))
    got, flags = device_maps([src[0], f[1], src[2]])
    assert flags == 0 and all(g.is_contiguous() for g in got) and all(torch.equal(g, t) for g, t in zip(got, f))
    got, flags = device_maps(f)
    assert flags == 0 and all(g is t for g, t in zip(got, f))


def test_zero_maps_strides():
    from mga_yolo_amd.detmaps import zero_maps
    shapes = [(2, 6, 4), (2, 3, 2), (2, 1, 1)]
    for f, (B, H, W) in zip(zero_maps(shapes, 3, torch.float16, "cpu", channels_last=True), shapes):
        assert f.shape == (B, 67, H, W) and f.dtype == torch.float16 and not f.any()
        assert f.stride() == (H * W * 67, 1, W * 67, 67)
    for got, (B, H, W) in zip(zero_maps(shapes, 3, torch.float32, "cpu"), shapes):
        assert got.stride() == (67 * H * W, H * W, W, 1) and not got.any()
    assert [f.stride() for f in zero_maps(shapes, 3, torch.float32, "cpu", False)] == [f.stride() for f in zero_maps(shapes, 3, torch.float32, "cpu")]


def test_plan_maps_refuses_the_other_layout():
    from mga_yolo_amd.detmaps import plan_maps
    f = _maps()
    assert plan_maps("plan", f, False) == 0 and plan_maps("plan", _cl(f), True) == _lib.MAPS_LAYOUT_NHWC
    for feats, cl in ((f, True), (_cl(f), False), ([_cl(f)[0], f[1], f[2]], False), ([w[:, :-1] for w in _cl(_maps(nc=4))], True)):
        with pytest.raises(ValueError, match="channels_last="):
            plan_maps("plan", feats, cl)


def test_the_plans_take_the_keyword():
    from mga_yolo_amd import DetLossPlan, DetPostPlan
    for plan in (DetLossPlan, DetPostPlan):
        p = inspect.signature(plan.create).parameters["channels_last"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
