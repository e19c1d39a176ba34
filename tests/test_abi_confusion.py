"""include/ext/mgaconfusion.h without a GPU: the header against its record in mga_yolo_amd._lib.METRIC_HEADERS (read by tests/abi_header.py),
against the built library, against the C compiler and against the layout pinned by hand below; every refusal before a launch; the size
query; fill_confusion.  include/ext/mgamatch.h beside it is tests/test_abi_match.py's."""
import ctypes as C
import re

import pytest

import abi_header as A
from abi_header import FAKE as P, a16
from mga_yolo_amd import _lib

NAME = "ext/mgaconfusion.h"
REC = _lib.METRIC_HEADERS[NAME]
# By hand (LP64): six pointers; six int32; four floats; five pointers; ws, ws_bytes; reserved, padded to 8
PINNED = (152, dict(dets=0, count=8, batch_idx=16, cls=24, bboxes=32, n=40, B=48, max_det=52, n_cap=56, m_cap=60, nc=64, flags=68, img_w=72,
                    img_h=76, conf_thres=80, iou_thres=84, det_out=88, lab_out=96, cm=104, acc=112, status=120, ws=128, ws_bytes=136,
                    reserved=144))
_SCALARS = {"int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t}


def test_the_record_sits_in_a_table_of_its_own():
    assert NAME not in _lib.HEADERS and NAME not in _lib.EXT_HEADERS and list(_lib.METRIC_HEADERS) == [NAME]
    assert _lib.ALL_HEADERS[NAME] is REC and len(_lib.ALL_HEADERS) == len(_lib.HEADERS) + len(_lib.EXT_HEADERS) + len(_lib.METRIC_HEADERS)
    assert "mgaconfusion.h" not in A.headers()
    h = A.read(NAME)
    assert h.includes == ("mgatargets.h",) and "MGACBAM_E_ARG" not in h.constants
    text = open(A.INCLUDE + "/" + NAME).read()
    for word in ("unstable sort", "LOWER label row", "LOWER detection index", "excluded from reference parity", "Not built", "Refusals", "Launches: 2"):
        assert word in text, word


def test_symbols_declared_bound_and_exported(built_lib):
    declared = sorted(A.read(NAME).functions)
    assert declared == sorted(REC.symbols) == ["mgacm_run", "mgacm_ws_bytes"]
    raw = C.CDLL(built_lib)
    assert all(hasattr(raw, fn) for fn in declared)
    others = {fn for t in (_lib.HEADERS, _lib.EXT_HEADERS) for rec in t.values() for fn in rec.symbols}
    assert not set(declared) & others
    lib = _lib.load()                                              # load() binds the third table exactly as the others
    for fn, (res, args) in REC.symbols.items():
        assert getattr(lib, fn).restype is res and getattr(lib, fn).argtypes == args


def test_constants_equal_the_mirrors():
    assert A.read(NAME).constants == REC.constants == dict(MGACM_MAX_NC=119, MGACM_SINGLE_CLS=1)
    assert (119 + 1) ** 2 * 4 == 57600 <= 64 * 1024                # the cells fit a workgroup's static LDS
    assert A.read("mgadet.h").constants["MGADET_MAX_GT"] == 256    # m_cap's bound, named in the header's text


def test_struct_mirror_equals_the_header_s_the_compiler_s_and_the_pinned_layout():
    parsed = A.read(NAME).structs
    assert list(parsed) == list(REC.structs) == ["mgacm_desc"]
    M = REC.structs["mgacm_desc"]
    assert M is _lib.ConfusionDesc
    fields = parsed["mgacm_desc"]
    assert [f for _, f, _ in fields] == [f[0] for f in M._fields_]
    for (ctype, field, length), (_, tm) in zip(fields, M._fields_):
        ctype = re.sub(r"\bconst\b", "", ctype).strip()
        assert length is None
        th = C.c_void_p if ctype.endswith("*") else _SCALARS[ctype]
        assert A.same_ctype(tm, th), f"{field} is {ctype} in the header, {tm.__name__} in the mirror"
    size, offsets = A.layout(M)
    assert (size, offsets) == PINNED
    assert bytes(M()) == bytes(size)                               # a fresh mirror is zero bytes
    compiled = A.compiler_layout((NAME,))
    if compiled is not None:
        assert compiled["mgacm_desc"] == PINNED


# B = 2: one overflow word and one bad-class word per image
WS_BYTES = a16(2 * 2 * 4)
_PTRS = ("dets", "count", "batch_idx", "cls", "bboxes", "n", "det_out", "lab_out", "cm", "status")


def _desc(with_acc=False, **over):
    D = _lib.ConfusionDesc()
    for i, name in enumerate(_PTRS + (("acc",) if with_acc else ())):
        setattr(D, name, P + 0x1000 * (i + 1))
    D.B, D.max_det, D.n_cap, D.m_cap, D.nc, D.flags, D.reserved = 2, 5, 7, 4, 3, 0, 0
    D.img_w, D.img_h, D.conf_thres, D.iou_thres = 64.0, 48.0, 0.25, 0.45
    D.ws, D.ws_bytes = P + 0x200000, WS_BYTES
    for k, v in over.items():
        setattr(D, k, v)
    return D


NAN, INF = float("nan"), float("inf")
CASES = [  # (what, accumulation on, overrides, code, a word of the message)
    ("B 0", False, dict(B=0), -2, "B=0"), ("max_det 0", False, dict(max_det=0), -2, "max_det=0"), ("n_cap -1", False, dict(n_cap=-1), -2, "n_cap=-1"),
    ("B * max_det = 2^31", False, dict(B=1 << 16, max_det=1 << 15), -2, "2^31"), ("n_cap = 2^29", False, dict(n_cap=1 << 29), -2, "2^29"),
    ("nc 0", False, dict(nc=0), -7, "nc=0"), ("nc 120", False, dict(nc=120), -7, "nc=120"), ("nc negative", False, dict(nc=-1), -7, "nc=-1"),
    ("m_cap 0", False, dict(m_cap=0), -7, "m_cap=0"), ("m_cap 257", False, dict(m_cap=257), -7, "m_cap=257"),
    ("unknown flag", False, dict(flags=2), -7, "flags=0x2"), ("reserved set", False, dict(reserved=1), -7, "reserved=1"),
    ("img_w 0", False, dict(img_w=0.0), -7, "img_w"), ("img_h negative", False, dict(img_h=-1.0), -7, "img_h"),
    ("img_w NaN", False, dict(img_w=NAN), -7, "img_w"), ("img_h inf", False, dict(img_h=INF), -7, "img_h"),
    ("conf_thres NaN", False, dict(conf_thres=NAN), -7, "conf_thres"), ("conf_thres inf", False, dict(conf_thres=INF), -7, "conf_thres"),
    ("conf_thres -inf", False, dict(conf_thres=-INF), -7, "conf_thres"),
    ("iou_thres NaN", False, dict(iou_thres=NAN), -7, "iou_thres"), ("iou_thres 1", False, dict(iou_thres=1.0), -7, "iou_thres"),
    ("iou_thres negative", False, dict(iou_thres=-0.01), -7, "iou_thres"), ("iou_thres inf", False, dict(iou_thres=INF), -7, "iou_thres"),
    ("dets NULL", False, dict(dets=None), -1, "dets"), ("count NULL", False, dict(count=None), -1, "count"),
    ("det_out NULL", False, dict(det_out=None), -1, "det_out"), ("cm NULL", True, dict(cm=None), -1, "cm"),
    ("status NULL", False, dict(status=None), -1, "status"), ("ws NULL", False, dict(ws=None), -1, "ws"),
    ("cls NULL", False, dict(cls=None), -1, "cls"), ("bboxes NULL", True, dict(bboxes=None), -1, "bboxes"),
    ("batch_idx NULL", False, dict(batch_idx=None), -1, "batch_idx"), ("lab_out NULL", False, dict(lab_out=None), -1, "lab_out"),
    ("dets misaligned", False, dict(dets=P + 0x1002), -4, "4-byte"), ("count misaligned", False, dict(count=P + 0x2001), -4, "4-byte"),
    ("n misaligned", False, dict(n=P + 0x6002), -4, "4-byte"), ("lab_out misaligned", False, dict(lab_out=P + 0x8003), -4, "4-byte"),
    ("cm misaligned", False, dict(cm=P + 0x9002), -4, "4-byte"), ("acc misaligned", True, dict(acc=P + 0xb004), -4, "8-byte"),
    ("ws misaligned", False, dict(ws=P + 0x200008), -4, "16-byte"),
    ("ws too small", False, dict(ws_bytes=WS_BYTES - 1), -6, "ws"), ("ws too small, accumulating", True, dict(ws_bytes=0), -6, "ws"),
]


@pytest.mark.parametrize("what,acc,over,code,word", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, acc, over, code, word):
    lib = _lib.load()
    assert lib.mgacm_run(C.byref(_desc(acc, **over)), None) == code, what
    msg = lib.mgacbam_last_error().decode()
    assert msg.startswith("mgacm_run: ") and word in msg, (what, msg)
    assert lib.mgacm_run(None, None) == -1 and b"desc is NULL" in lib.mgacbam_last_error()


def test_the_bounds_themselves_pass_the_checks(built_lib):
    """nc = 119, m_cap = 256, iou_thres = 0 and a negative conf_thres are inside: with them the first refusal is the one planted behind them"""
    lib = _lib.load()
    assert lib.mgacm_run(C.byref(_desc(nc=119, m_cap=256, iou_thres=0.0, conf_thres=-1.0, flags=1, ws_bytes=0)), None) == -6
    assert lib.mgacm_run(C.byref(_desc(n_cap=0, batch_idx=None, cls=None, bboxes=None, lab_out=None, n=None, ws_bytes=0)), None) == -6


def test_size_query(built_lib):
    lib = _lib.load()
    assert lib.mgacm_ws_bytes(C.byref(_desc())) == WS_BYTES == _lib.confusion_ws_bytes(_desc()) == _lib.confusion_ws_bytes(_desc(True))
    assert lib.mgacm_ws_bytes(C.byref(_desc(ws=None, ws_bytes=0, dets=None, cm=None))) == WS_BYTES          # buffers do not enter the size
    assert lib.mgacm_ws_bytes(C.byref(_desc(B=9))) == a16(2 * 9 * 4)
    assert lib.mgacm_ws_bytes(C.byref(_desc(nc=119))) == WS_BYTES                                           # the cells live in LDS, not in ws
    for over in (dict(B=0), dict(nc=0), dict(nc=120), dict(m_cap=300), dict(flags=4), dict(reserved=2), dict(img_w=-3.0), dict(iou_thres=1.0),
                 dict(conf_thres=NAN)):
        assert lib.mgacm_ws_bytes(C.byref(_desc(**over))) == 0 and lib.mgacbam_last_error(), over
        with pytest.raises(RuntimeError):
            _lib.confusion_ws_bytes(_desc(**over))
    assert lib.mgacm_ws_bytes(None) == 0


def test_fill_sets_every_field():
    import torch
    from mga_yolo_amd._binding import fill_confusion
    i32 = torch.int32
    dets, count = torch.zeros(2, 5, 6), torch.zeros(2, dtype=i32)
    lab = (torch.zeros(7), torch.zeros(7), torch.zeros(7, 4))
    n = torch.zeros(1, dtype=i32)
    outs = (torch.zeros(2, 5, dtype=i32), torch.zeros(7, dtype=i32), torch.zeros(4, 4, dtype=i32))
    acc, status = torch.zeros(4, 4, dtype=torch.int64), torch.zeros(1, dtype=i32)
    ws = torch.zeros(16, dtype=torch.uint8)
    D = _lib.ConfusionDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_confusion(D, dets, count, *lab, n, 4, 3, _lib.CM_SINGLE_CLS, 96.0, 64.0, 0.25, 0.5, *outs, acc, status, ws=ws)
    assert (D.dets, D.count, D.batch_idx, D.cls, D.bboxes, D.n) == tuple(t.data_ptr() for t in (dets, count, *lab, n))
    assert (D.B, D.max_det, D.n_cap, D.m_cap, D.nc, D.flags, D.reserved) == (2, 5, 7, 4, 3, 1, 0)
    assert (D.img_w, D.img_h, D.conf_thres, D.iou_thres) == (96.0, 64.0, 0.25, 0.5)
    assert (D.det_out, D.lab_out, D.cm, D.acc, D.status) == tuple(t.data_ptr() for t in (*outs, acc, status))
    assert (D.ws, D.ws_bytes) == (ws.data_ptr(), 16)
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    none = (torch.zeros(0), torch.zeros(0), torch.zeros(0, 4))
    fill_confusion(D, dets, count, *none, None, 1, 80, 0, 64.0, 64.0, 0.25, 0.45, outs[0], torch.zeros(0, dtype=i32), torch.zeros(81, 81, dtype=i32),
                   None, status)
    assert (D.batch_idx, D.cls, D.bboxes, D.lab_out, D.n, D.n_cap, D.nc, D.flags) == (None, None, None, None, None, 0, 80, 0)
    assert (D.acc, D.ws, D.ws_bytes, D.reserved) == (None, None, 0, 0) and D.conf_thres == 0.25 and D.iou_thres == C.c_float(0.45).value
