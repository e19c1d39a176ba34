"""include/ext/mgamatch.h without a GPU: the header against its record in mga_yolo_amd._lib.EXT_HEADERS (read by tests/abi_header.py), against
the built library, against the C compiler and against the layout pinned by hand below; every refusal before a launch; the size query;
fill_match.  The headers directly under include/ are tests/test_abi_headers.py's."""
import ctypes as C
import re

import pytest

import abi_header as A
from abi_header import FAKE as P, a16
from mga_yolo_amd import _lib

NAME = "ext/mgamatch.h"
REC = _lib.EXT_HEADERS[NAME]
# By hand (LP64): six pointers; four int32, two floats, two int32; sixteen floats; two int32; eleven pointers; ws, ws_bytes; reserved, padded to 8
PINNED = (264, dict(dets=0, count=8, batch_idx=16, cls=24, bboxes=32, n=40, B=48, max_det=52, n_cap=56, m_cap=60, img_w=64, img_h=68, niou=72,
                    flags=76, iouv=80, rows_cap=144, tgt_cap=148, tp=152, best_iou=160, best_gt=168, rows_tp=176, rows_conf=184, rows_cls=192,
                    rows_img=200, tgt_cls=208, tgt_img=216, state=224, status=232, ws=240, ws_bytes=248, reserved=256))
_SCALARS = {"int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t}


def test_the_header_lies_below_include_and_beside_no_record():
    assert NAME not in _lib.HEADERS and "mgamatch.h" not in A.headers() and list(_lib.EXT_HEADERS) == [NAME]
    h = A.read(NAME)
    assert h.includes == ("mgatargets.h",) and "MGACBAM_E_ARG" not in h.constants
    for word in ("stable sort", "LOWER label row", "excluded from reference parity"):       # the tie rule and its standing are stated
        assert word in open(A.INCLUDE + "/" + NAME).read()


def test_symbols_declared_bound_and_exported(built_lib):
    declared = sorted(A.read(NAME).functions)
    assert declared == sorted(REC.symbols) == ["mgamatch_run", "mgamatch_ws_bytes"]
    raw = C.CDLL(built_lib)
    assert all(hasattr(raw, fn) for fn in declared)
    others = {fn for rec in _lib.HEADERS.values() for fn in rec.symbols}
    assert not set(declared) & others
    lib = _lib.load()                                              # load() binds the second table exactly as the first
    for fn, (res, args) in REC.symbols.items():
        assert getattr(lib, fn).restype is res and getattr(lib, fn).argtypes == args


def test_constants_equal_the_mirrors():
    assert A.read(NAME).constants == REC.constants == dict(MGAMATCH_MAX_IOU=16, MGAMATCH_SINGLE_CLS=1)
    assert A.read("mgadet.h").constants["MGADET_MAX_GT"] == 256    # m_cap's bound, named in the header's text


def test_struct_mirror_equals_the_header_s_the_compiler_s_and_the_pinned_layout():
    parsed = A.read(NAME).structs
    assert list(parsed) == list(REC.structs) == ["mgamatch_desc"]
    M = REC.structs["mgamatch_desc"]
    fields = parsed["mgamatch_desc"]
    assert [f for _, f, _ in fields] == [f[0] for f in M._fields_]
    for (ctype, field, length), (_, tm) in zip(fields, M._fields_):
        ctype = re.sub(r"\bconst\b", "", ctype).strip()
        th = C.c_void_p if ctype.endswith("*") else _SCALARS[ctype]
        if length is not None:
            th = th * A.read(NAME).constants[length]
        assert A.same_ctype(tm, th), f"{field} is {ctype} in the header, {tm.__name__} in the mirror"
    size, offsets = A.layout(M)
    assert (size, offsets) == PINNED
    assert bytes(M()) == bytes(size)                               # a fresh mirror is zero bytes
    compiled = A.compiler_layout((NAME,))
    if compiled is not None:
        assert compiled["mgamatch_desc"] == PINNED


# B = 2, max_det = 5, niou = 10: one overflow word per image and the four of state's snapshot
WS_BYTES = a16((2 + 4) * 4)
_PTRS = ("dets", "count", "batch_idx", "cls", "bboxes", "n", "tp", "best_iou", "best_gt", "status")
_ACC = ("rows_tp", "rows_conf", "rows_cls", "rows_img", "tgt_cls", "tgt_img", "state")


def _desc(acc=False, **over):
    D = _lib.MatchDesc()
    for i, name in enumerate(_PTRS + (_ACC if acc else ())):
        setattr(D, name, P + 0x1000 * (i + 1))
    D.B, D.max_det, D.n_cap, D.m_cap, D.img_w, D.img_h, D.niou, D.flags, D.reserved = 2, 5, 7, 4, 64.0, 48.0, 10, 0, 0
    for t in range(10):
        D.iouv[t] = 0.5 + 0.05 * t
    D.rows_cap, D.tgt_cap = (40, 30) if acc else (0, 0)
    D.ws, D.ws_bytes = P + 0x200000, WS_BYTES
    for k, v in over.items():
        m = re.fullmatch(r"iouv(\d+)", k)
        if m:
            D.iouv[int(m.group(1))] = v
        else:
            setattr(D, k, v)
    return D


CASES = [  # (what, accumulation on, overrides, code)
    ("B 0", False, dict(B=0), -2), ("max_det 0", False, dict(max_det=0), -2), ("n_cap -1", False, dict(n_cap=-1), -2),
    ("B * max_det = 2^31", False, dict(B=1 << 16, max_det=1 << 15), -2), ("n_cap = 2^29", False, dict(n_cap=1 << 29), -2),
    ("niou 0", False, dict(niou=0), -7), ("niou 17", False, dict(niou=17), -7),
    ("iouv not ascending", False, dict(iouv3=0.6), -7), ("iouv repeated", False, dict(iouv1=0.5), -7), ("iouv 0", False, dict(iouv0=0.0), -7),
    ("iouv > 1", False, dict(iouv9=1.01), -7), ("iouv NaN", False, dict(iouv4=float("nan")), -7),
    ("m_cap 0", False, dict(m_cap=0), -7), ("m_cap 257", False, dict(m_cap=257), -7), ("unknown flag", False, dict(flags=2), -7),
    ("reserved set", False, dict(reserved=1), -7), ("img_w 0", False, dict(img_w=0.0), -7), ("img_h negative", False, dict(img_h=-1.0), -7),
    ("img_w NaN", False, dict(img_w=float("nan")), -7), ("img_h inf", False, dict(img_h=float("inf")), -7),
    ("rows_cap 0", True, dict(rows_cap=0), -7), ("tgt_cap 0", True, dict(tgt_cap=0), -7),
    ("dets NULL", False, dict(dets=None), -1), ("count NULL", False, dict(count=None), -1), ("tp NULL", False, dict(tp=None), -1),
    ("best_iou NULL", False, dict(best_iou=None), -1), ("best_gt NULL", False, dict(best_gt=None), -1), ("status NULL", False, dict(status=None), -1),
    ("ws NULL", False, dict(ws=None), -1), ("cls NULL", False, dict(cls=None), -1), ("bboxes NULL", True, dict(bboxes=None), -1),
    ("state alone", False, dict(state=P + 0x50000), -1), ("no state", True, dict(state=None), -1), ("no rows_tp", True, dict(rows_tp=None), -1),
    ("no tgt_img", True, dict(tgt_img=None), -1),
    ("dets misaligned", False, dict(dets=P + 0x1002), -4), ("count misaligned", False, dict(count=P + 0x2001), -4),
    ("n misaligned", False, dict(n=P + 0x6002), -4), ("best_gt misaligned", False, dict(best_gt=P + 0x9003), -4),
    ("rows_conf misaligned", True, dict(rows_conf=P + 0xc002), -4), ("state misaligned", True, dict(state=P + 0x11001), -4),
    ("ws misaligned", False, dict(ws=P + 0x200008), -4),
    ("ws too small", False, dict(ws_bytes=WS_BYTES - 1), -6), ("ws too small, accumulating", True, dict(ws_bytes=0), -6),
]


@pytest.mark.parametrize("what,acc,over,code", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, acc, over, code):
    lib = _lib.load()
    assert lib.mgamatch_run(C.byref(_desc(acc, **over)), None) == code, what
    assert lib.mgacbam_last_error(), what
    assert lib.mgamatch_run(None, None) == -1


def test_size_query(built_lib):
    lib = _lib.load()
    assert lib.mgamatch_ws_bytes(C.byref(_desc())) == WS_BYTES == _lib.match_ws_bytes(_desc()) == _lib.match_ws_bytes(_desc(True))
    assert lib.mgamatch_ws_bytes(C.byref(_desc(ws=None, ws_bytes=0, dets=None, tp=None))) == WS_BYTES          # buffers do not enter the size
    assert lib.mgamatch_ws_bytes(C.byref(_desc(B=9))) == a16((9 + 4) * 4)
    assert lib.mgamatch_ws_bytes(C.byref(_desc(n_cap=0, batch_idx=None, cls=None, bboxes=None, n=None, tp=P + 1, rows_tp=None))) == WS_BYTES
    for over in (dict(B=0), dict(niou=0), dict(iouv2=0.5), dict(m_cap=300), dict(flags=4), dict(reserved=2), dict(img_w=-3.0)):
        assert lib.mgamatch_ws_bytes(C.byref(_desc(**over))) == 0 and lib.mgacbam_last_error(), over
        with pytest.raises(RuntimeError):
            _lib.match_ws_bytes(_desc(**over))
    assert lib.mgamatch_ws_bytes(None) == 0


def test_fill_sets_every_field():
    import torch
    from mga_yolo_amd._binding import fill_match
    i32 = torch.int32
    dets, count = torch.zeros(2, 5, 6), torch.zeros(2, dtype=i32)
    lab = (torch.zeros(7), torch.zeros(7), torch.zeros(7, 4))
    n = torch.zeros(1, dtype=i32)
    outs = (torch.zeros(2, 5, 3, dtype=torch.uint8), torch.zeros(2, 5), torch.zeros(2, 5, dtype=i32), torch.zeros(1, dtype=i32))
    acc = (torch.zeros(40, 3, dtype=torch.uint8), torch.zeros(40), torch.zeros(40), torch.zeros(40, dtype=i32), torch.zeros(30),
           torch.zeros(30, dtype=i32), torch.zeros(4, dtype=i32))
    ws = torch.zeros(16, dtype=torch.uint8)
    D = _lib.MatchDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_match(D, dets, count, *lab, n, 4, 96.0, 64.0, [0.5, 0.75, 0.9], _lib.MATCH_SINGLE_CLS, *outs, acc=acc, ws=ws)
    assert (D.dets, D.count, D.batch_idx, D.cls, D.bboxes, D.n) == tuple(t.data_ptr() for t in (dets, count, *lab, n))
    assert (D.B, D.max_det, D.n_cap, D.m_cap, D.img_w, D.img_h, D.niou, D.flags, D.reserved) == (2, 5, 7, 4, 96.0, 64.0, 3, 1, 0)
    assert list(D.iouv) == [0.5, 0.75, C.c_float(0.9).value] + [0.0] * 13 and (D.rows_cap, D.tgt_cap) == (40, 30)
    assert (D.tp, D.best_iou, D.best_gt, D.status) == tuple(t.data_ptr() for t in outs)
    assert tuple(getattr(D, k) for k in _ACC) == tuple(t.data_ptr() for t in acc) and (D.ws, D.ws_bytes) == (ws.data_ptr(), 16)
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    none = (torch.zeros(0), torch.zeros(0), torch.zeros(0, 4))
    fill_match(D, dets, count, *none, None, 1, 64.0, 64.0, [0.5], 0, *outs)
    assert (D.batch_idx, D.cls, D.bboxes, D.n, D.n_cap, D.niou, D.flags) == (None, None, None, None, 0, 1, 0)
    assert all(getattr(D, k) is None for k in _ACC) and (D.rows_cap, D.tgt_cap, D.ws, D.ws_bytes, D.reserved) == (0, 0, None, 0, 0)
