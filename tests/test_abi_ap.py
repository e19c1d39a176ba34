"""include/ext/mgaap.h without a GPU: the header against its record in mga_yolo_amd._lib.CURVE_HEADERS (read by tests/abi_header.py),
against the built library, against the C compiler and against the layout pinned by hand below; every refusal before a launch; the size
query against the header's formula; fill_ap.  The headers of the three stages before it are tests/test_abi_match.py's and
tests/test_abi_confusion.py's."""
import ctypes as C
import re

import pytest

import abi_header as A
from abi_header import FAKE as P, a16
from mga_yolo_amd import _lib

NAME = "ext/mgaap.h"
REC = _lib.CURVE_HEADERS[NAME]
# By hand (LP64): seven pointers; four int32; four pointers; ws, ws_bytes; reserved, padded to 8
PINNED = (128, dict(rows_tp=0, rows_conf=8, rows_cls=16, rows_img=24, tgt_cls=32, tgt_img=40, state=48, rows_cap=56, tgt_cap=60, niou=64, nc=68,
                    grid_ap=72, grid_curve=80, result=88, status=96, ws=104, ws_bytes=112, reserved=120))
_SCALARS = {"int32_t": C.c_int32, "size_t": C.c_size_t}


def test_the_record_sits_in_a_table_of_its_own():
    assert list(_lib.CURVE_HEADERS) == [NAME] and _lib._TABLES["CURVE_HEADERS"] is _lib.CURVE_HEADERS
    assert all(NAME not in t for t in (_lib.HEADERS, _lib.EXT_HEADERS, _lib.METRIC_HEADERS, _lib.LAYOUT_HEADERS, _lib.ALL_HEADERS))
    assert _lib._EVERY_HEADER[NAME] is REC and len(_lib._EVERY_HEADER) == sum(len(t) for t in _lib._TABLES.values())
    assert "mgaap.h" not in A.headers()
    h = A.read(NAME)
    assert h.includes == ("mgatargets.h",) and "MGACBAM_E_ARG" not in h.constants
    text = open(A.INCLUDE + "/" + NAME).read()
    for word in ("unstable sort", "accumulation order", "-0.0 compares equal to +0.0", "excluded from reference parity", "LAST index", "Not built",
                 "Refusals", "Launches: 3 + 3 * passes + 7 * niou", "mgaap_ws_bytes = ", "3 takes precedence"):
        assert word in text, word
    for other, word in (("ext/mgamatch.h", "include/ext/mgaap.h"), ("ext/mgaconfusion.h", "include/ext/mgaap.h")):
        assert word in open(A.INCLUDE + "/" + other).read(), other     # the stages before it point at it


def test_symbols_declared_bound_and_exported(built_lib):
    declared = sorted(A.read(NAME).functions)
    assert declared == sorted(REC.symbols) == ["mgaap_run", "mgaap_ws_bytes"]
    raw = C.CDLL(built_lib)
    assert all(hasattr(raw, fn) for fn in declared)
    others = {fn for t in (_lib.HEADERS, _lib.EXT_HEADERS, _lib.METRIC_HEADERS, _lib.LAYOUT_HEADERS) for rec in t.values() for fn in rec.symbols}
    assert not set(declared) & others
    lib = _lib.load()                                              # load() binds this table exactly as the others
    for fn, (res, args) in REC.symbols.items():
        assert getattr(lib, fn).restype is res and getattr(lib, fn).argtypes == args


def test_constants_equal_the_mirrors():
    assert A.read(NAME).constants == REC.constants == dict(MGAAP_MAX_NC=1024, MGAAP_TILE=2048, MGAAP_AP_POINTS=101, MGAAP_CURVE_POINTS=1000)
    assert A.read("ext/mgamatch.h").constants["MGAMATCH_MAX_IOU"] == 16 == _lib.MATCH_MAX_IOU     # niou's bound, named in the header's text
    lay = _lib.ap_result_layout(80, 10)
    assert lay["total"] == 8 * 80 * (10 + 3001) and lay["nt"][0] == 8 * 80 * 3010 and lay["n_det"][0] == lay["nt"][0] + 4 * 80


def test_struct_mirror_equals_the_header_s_the_compiler_s_and_the_pinned_layout():
    parsed = A.read(NAME).structs
    assert list(parsed) == list(REC.structs) == ["mgaap_desc"]
    M = REC.structs["mgaap_desc"]
    assert M is _lib.ApDesc
    fields = parsed["mgaap_desc"]
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
        assert compiled["mgaap_desc"] == PINNED


def ws_formula(rows_cap, nc):
    """the header's formula, restated"""
    T = (rows_cap + 2047) // 2048
    return a16(32) + a16(4 * (nc + 2)) + 6 * a16(4 * rows_cap) + a16(8 * rows_cap) + a16(1024 * T) + a16(4 * T) + 2 * a16(16 * T)


_PTRS = ("rows_tp", "rows_conf", "rows_cls", "rows_img", "tgt_cls", "tgt_img", "state", "grid_ap", "grid_curve", "result", "status")
ROWS, NC = 5000, 3
WS_BYTES = ws_formula(ROWS, NC)


def _desc(**over):
    D = _lib.ApDesc()
    for i, name in enumerate(_PTRS):
        setattr(D, name, P + 0x1000 * (i + 1))
    D.rows_cap, D.tgt_cap, D.niou, D.nc, D.reserved = ROWS, 100, 10, NC, 0
    D.ws, D.ws_bytes = P + 0x200000, WS_BYTES
    for k, v in over.items():
        setattr(D, k, v)
    return D


CASES = [  # (what, overrides, code, a word of the message)
    ("niou 0", dict(niou=0), -7, "niou=0"), ("niou 17", dict(niou=17), -7, "niou=17"), ("niou negative", dict(niou=-1), -7, "niou=-1"),
    ("nc 0", dict(nc=0), -7, "nc=0"), ("nc 1025", dict(nc=1025), -7, "nc=1025"), ("nc negative", dict(nc=-3), -7, "nc=-3"),
    ("reserved set", dict(reserved=1), -7, "reserved=1"),
    ("rows_cap 0", dict(rows_cap=0), -2, "rows_cap=0"), ("tgt_cap 0", dict(tgt_cap=0), -2, "tgt_cap=0"), ("rows_cap negative", dict(rows_cap=-1), -2, "rows_cap=-1"),
    ("rows_cap = 2^31 / niou", dict(rows_cap=(1 << 31) // 10), -2, "2^31"), ("tgt_cap = 2^31 / niou", dict(tgt_cap=(1 << 31) // 10), -2, "2^31"),
    ("rows_cap = 2^31 / 16", dict(niou=16, rows_cap=1 << 27), -2, "2^31"),
    ("rows_tp NULL", dict(rows_tp=None), -1, "rows_tp"), ("rows_conf NULL", dict(rows_conf=None), -1, "rows_conf"),
    ("rows_cls NULL", dict(rows_cls=None), -1, "rows_cls"), ("tgt_cls NULL", dict(tgt_cls=None), -1, "tgt_cls"), ("state NULL", dict(state=None), -1, "state"),
    ("grid_ap NULL", dict(grid_ap=None), -1, "grid_ap"), ("grid_curve NULL", dict(grid_curve=None), -1, "grid_curve"),
    ("result NULL", dict(result=None), -1, "result"), ("status NULL", dict(status=None), -1, "status"), ("ws NULL", dict(ws=None), -1, "ws"),
    ("rows_conf misaligned", dict(rows_conf=P + 0x2002), -4, "4-byte"), ("rows_img misaligned", dict(rows_img=P + 0x4001), -4, "4-byte"),
    ("tgt_img misaligned", dict(tgt_img=P + 0x6003), -4, "4-byte"), ("state misaligned", dict(state=P + 0x7002), -4, "4-byte"),
    ("status misaligned", dict(status=P + 0xb001), -4, "4-byte"),
    ("grid_ap misaligned", dict(grid_ap=P + 0x8004), -4, "8-byte"), ("grid_curve misaligned", dict(grid_curve=P + 0x9004), -4, "8-byte"),
    ("result misaligned", dict(result=P + 0xa004), -4, "8-byte"), ("ws misaligned", dict(ws=P + 0x200008), -4, "16-byte"),
    ("ws too small", dict(ws_bytes=WS_BYTES - 1), -6, "ws"), ("ws empty", dict(ws_bytes=0), -6, "ws"),
]


@pytest.mark.parametrize("what,over,code,word", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, over, code, word):
    lib = _lib.load()
    assert lib.mgaap_run(C.byref(_desc(**over)), None) == code, what
    msg = lib.mgacbam_last_error().decode()
    assert msg.startswith("mgaap_run: ") and word in msg, (what, msg)
    assert lib.mgaap_run(None, None) == -1 and b"desc is NULL" in lib.mgacbam_last_error()


def test_the_bounds_themselves_pass_the_checks(built_lib):
    """nc = 1024, niou = 16 and 1, caps just below 2^31 / niou, rows_img / tgt_img NULL and an odd rows_tp are inside: with them the first
    refusal is the one planted behind them"""
    lib = _lib.load()
    assert lib.mgaap_run(C.byref(_desc(nc=1024, niou=16, rows_cap=(1 << 27) - 1, tgt_cap=(1 << 27) - 1, ws_bytes=0)), None) == -6
    assert lib.mgaap_run(C.byref(_desc(nc=1, niou=1, rows_cap=(1 << 31) - 1, tgt_cap=1, ws_bytes=0)), None) == -6
    assert lib.mgaap_run(C.byref(_desc(rows_img=None, tgt_img=None, rows_tp=P + 0x1001, ws_bytes=0)), None) == -6


def test_size_query_against_the_formula(built_lib):
    lib = _lib.load()
    assert lib.mgaap_ws_bytes(C.byref(_desc())) == WS_BYTES == _lib.ap_ws_bytes(_desc())
    assert lib.mgaap_ws_bytes(C.byref(_desc(ws=None, ws_bytes=0, rows_tp=None, result=None))) == WS_BYTES           # buffers do not enter the size
    assert lib.mgaap_ws_bytes(C.byref(_desc(niou=1))) == WS_BYTES == lib.mgaap_ws_bytes(C.byref(_desc(tgt_cap=7)))   # nor niou, nor tgt_cap
    for rows, nc in ((1, 1), (2047, 80), (2048, 80), (2049, 300), (1 << 17, 1), (1 << 20, 80), (1500000, 80), (1 << 21, 1024)):
        assert lib.mgaap_ws_bytes(C.byref(_desc(rows_cap=rows, nc=nc))) == ws_formula(rows, nc), (rows, nc)
    assert ws_formula(1 << 21, 80) == 68194672                                                                        # 65.0 MiB
    for over in (dict(niou=0), dict(nc=0), dict(nc=1025), dict(rows_cap=0), dict(tgt_cap=-2), dict(reserved=2), dict(rows_cap=(1 << 31) // 10)):
        assert lib.mgaap_ws_bytes(C.byref(_desc(**over))) == 0 and lib.mgacbam_last_error(), over
        with pytest.raises(RuntimeError):
            _lib.ap_ws_bytes(_desc(**over))
    assert lib.mgaap_ws_bytes(None) == 0


def test_fill_sets_every_field():
    import torch
    from mga_yolo_amd._binding import fill_ap
    i32 = torch.int32
    rows = (torch.zeros(9, 10, dtype=torch.uint8), torch.zeros(9), torch.zeros(9), torch.zeros(9, dtype=i32))
    tgt = (torch.zeros(5), torch.zeros(5, dtype=i32))
    state, status = torch.zeros(4, dtype=i32), torch.zeros(1, dtype=i32)
    grids = (torch.zeros(101, dtype=torch.float64), torch.zeros(1000, dtype=torch.float64))
    result, ws = torch.zeros(_lib.ap_result_layout(3, 10)["total"], dtype=torch.uint8), torch.zeros(32, dtype=torch.uint8)
    D = _lib.ApDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_ap(D, *rows, *tgt, state, 3, *grids, result, status, ws=ws)
    assert (D.rows_tp, D.rows_conf, D.rows_cls, D.rows_img, D.tgt_cls, D.tgt_img, D.state) == tuple(t.data_ptr() for t in (*rows, *tgt, state))
    assert (D.rows_cap, D.tgt_cap, D.niou, D.nc, D.reserved) == (9, 5, 10, 3, 0)
    assert (D.grid_ap, D.grid_curve, D.result, D.status) == tuple(t.data_ptr() for t in (*grids, result, status))
    assert (D.ws, D.ws_bytes) == (ws.data_ptr(), 32)
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_ap(D, rows[0][:, :1], rows[1], rows[2], None, tgt[0], None, state, 1024, *grids, result, status)
    assert (D.rows_img, D.tgt_img, D.ws, D.ws_bytes, D.reserved) == (None, None, None, 0, 0) and (D.niou, D.nc) == (1, 1024)
