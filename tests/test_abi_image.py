"""include/ext/mgaimage.h without a GPU: the header against its record in mga_yolo_amd._lib.IMAGE_HEADERS (read by tests/abi_header.py),
against the built library, against the C compiler and against the layout pinned by hand below; every refusal before a launch; fill_image."""
import ctypes as C
import re

import pytest

import abi_header as A
from abi_header import FAKE as P
from mga_yolo_amd import _lib

NAME = "ext/mgaimage.h"
REC = _lib.IMAGE_HEADERS[NAME]
# By hand (LP64): two pointers; nine int32; padded to 8
PINNED = (56, dict(src=0, dst=8, B=16, C=20, in_h=24, in_w=28, out_h=32, out_w=36, dtype=40, flags=44, reserved=48))
_SCALARS = {"int32_t": C.c_int32}


def test_the_record_sits_in_a_table_of_its_own():
    assert list(_lib.IMAGE_HEADERS) == [NAME] and _lib._TABLES["IMAGE_HEADERS"] is _lib.IMAGE_HEADERS
    assert all(NAME not in t for t in (_lib.HEADERS, _lib.EXT_HEADERS, _lib.METRIC_HEADERS, _lib.LAYOUT_HEADERS, _lib.CURVE_HEADERS, _lib.ALL_HEADERS))
    assert _lib._EVERY_HEADER[NAME] is REC and len(_lib._EVERY_HEADER) == sum(len(t) for t in _lib._TABLES.values())
    assert "mgaimage.h" not in A.headers()
    h = A.read(NAME)
    assert h.includes == ("mgatargets.h",) and "MGACBAM_E_ARG" not in h.constants
    text = open(A.INCLUDE + "/" + NAME).read()
    for word in ("correctly rounded fp32 division", "126 of the 256 byte values", "align_corners=False", "include/mgaresample.h", "Refusals", "Not built",
                 "No workspace", "One launch per call", "k_img_convert", "k_img_resize"):
        assert word in text, word


def test_symbols_declared_bound_and_exported(built_lib):
    declared = sorted(A.read(NAME).functions)
    assert declared == sorted(REC.symbols) == ["mgaimg_run"]
    raw = C.CDLL(built_lib)
    assert all(hasattr(raw, fn) for fn in declared)
    others = {fn for k, t in _lib._TABLES.items() if k != "IMAGE_HEADERS" for rec in t.values() for fn in rec.symbols}
    assert not set(declared) & others
    lib = _lib.load()
    for fn, (res, args) in REC.symbols.items():
        assert getattr(lib, fn).restype is res and getattr(lib, fn).argtypes == args


def test_constants_equal_the_mirrors():
    assert A.read(NAME).constants == REC.constants == dict(MGAIMG_SRC_NHWC=1, MGAIMG_DST_NHWC=2, MGAIMG_REVERSE_C=4, MGAIMG_MAX_C=4,
                                                           MGAIMG_TILE_PX=1024, MGAIMG_TILE_W=1024, MGAIMG_TILE_H=64)
    seen = A.visible_constants(NAME)
    assert (seen["MGACBAM_F32"], seen["MGACBAM_F16"], seen["MGACBAM_BF16"]) == (_lib.F32, _lib.F16, _lib.BF16) == (0, 1, 2)
    assert seen["MGACBAM_E_ARG"] == _lib.E_ARG == -7


def test_struct_mirror_equals_the_header_s_the_compiler_s_and_the_pinned_layout():
    parsed = A.read(NAME).structs
    assert list(parsed) == list(REC.structs) == ["mgaimg_desc"]
    M = REC.structs["mgaimg_desc"]
    assert M is _lib.ImageDesc
    fields = parsed["mgaimg_desc"]
    assert [f for _, f, _ in fields] == [f[0] for f in M._fields_]
    for (ctype, field, length), (_, tm) in zip(fields, M._fields_):
        ctype = re.sub(r"\bconst\b", "", ctype).strip()
        assert length is None
        th = C.c_void_p if ctype.endswith("*") else _SCALARS[ctype]
        assert A.same_ctype(tm, th), f"{field} is {ctype} in the header, {tm.__name__} in the mirror"
    size, offsets = A.layout(M)
    assert (size, offsets) == PINNED
    assert bytes(M()) == bytes(size)
    compiled = A.compiler_layout((NAME,))
    if compiled is not None:
        assert compiled["mgaimg_desc"] == PINNED


def _desc(**over):
    D = _lib.ImageDesc()
    D.src, D.dst = P + 0x1001, P + 0x100000                        # an odd src is inside: it has no alignment requirement
    D.B, D.C, D.in_h, D.in_w, D.out_h, D.out_w = 2, 3, 40, 56, 64, 64
    D.dtype, D.flags, D.reserved = _lib.F32, 0, 0
    for k, v in over.items():
        setattr(D, k, v)
    return D


BIG = 1 << 31
CASES = [  # (what, overrides, code, a word of the message)
    ("src NULL", dict(src=None), -1, "src"), ("dst NULL", dict(dst=None), -1, "dst"),
    ("B 0", dict(B=0), -2, "B=0"), ("B negative", dict(B=-1), -2, "B=-1"),
    ("in_h 0", dict(in_h=0), -2, "in=0x56"), ("in_w 0", dict(in_w=0), -2, "in=40x0"),
    ("out_h 0", dict(out_h=0), -2, "out=0x64"), ("out_w negative", dict(out_w=-5), -2, "out=64x-5"),
    ("C 0", dict(C=0), -2, "C=0"), ("C 5", dict(C=5), -2, "C=5"), ("C negative", dict(C=-1), -2, "C=-1"),
    ("source at 2^31", dict(B=1, C=1, in_h=1 << 16, in_w=1 << 15, out_h=1, out_w=1), -2, "2^31"),
    ("destination at 2^31", dict(B=2, C=4, in_h=1, in_w=1, out_h=1 << 14, out_w=1 << 14), -2, "2^31"),
    ("far above 2^31", dict(B=BIG - 1, C=4, in_h=BIG - 1, in_w=BIG - 1, out_h=BIG - 1, out_w=BIG - 1), -2, "2^31"),
    ("dtype 3", dict(dtype=3), -3, "dtype 3"), ("dtype negative", dict(dtype=-1), -3, "dtype -1"),
    ("flag bit 8", dict(flags=8), -7, "flags=0x8"), ("flag bit 31", dict(flags=-(1 << 31)), -7, "flags=0x80000000"),
    ("flags 7 | 16", dict(flags=23), -7, "flags=0x17"), ("reserved set", dict(reserved=1), -7, "reserved=1"),
    ("fp32 dst off by 2", dict(dst=P + 0x100002), -4, "4-byte"), ("fp32 dst off by 1", dict(dst=P + 0x100001), -4, "4-byte"),
    ("fp16 dst off by 1", dict(dtype=1, dst=P + 0x100001), -4, "2-byte"), ("bf16 dst off by 3", dict(dtype=2, dst=P + 0x100003), -4, "2-byte"),
]


@pytest.mark.parametrize("what,over,code,word", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, over, code, word):
    lib = _lib.load()
    assert lib.mgaimg_run(C.byref(_desc(**over)), None) == code, what
    msg = lib.mgacbam_last_error().decode()
    assert msg.startswith("mgaimg_run: ") and word in msg, (what, msg)
    assert lib.mgaimg_run(None, None) == -1 and b"desc is NULL" in lib.mgacbam_last_error()


def test_the_order_of_the_checks(built_lib):
    """what lies just inside each bound passes that check: the refusal is then the one planted behind it (a misaligned dst, the last check)"""
    lib = _lib.load()
    bad_dst = P + 0x100001
    for over in (dict(C=1), dict(C=4), dict(flags=7), dict(dtype=2, dst=P + 0x100003),
                 dict(B=1, C=1, in_h=1, in_w=BIG - 1, out_h=1, out_w=1), dict(B=1, C=1, in_h=1, in_w=1, out_h=BIG - 1, out_w=1),
                 dict(B=(BIG - 1) // 4, C=4, in_h=1, in_w=1, out_h=1, out_w=1)):
        assert lib.mgaimg_run(C.byref(_desc(**dict(dict(dst=bad_dst), **over))), None) == -4, over
    assert lib.mgaimg_run(C.byref(_desc(dtype=1, dst=P + 0x100002, in_h=0)), None) == -2          # the shape is checked before the alignment
    assert lib.mgaimg_run(C.byref(_desc(dtype=9, flags=8)), None) == -3                          # the dtype before the flags


def test_fill_sets_every_field():
    import torch
    from mga_yolo_amd._binding import fill_image
    src = torch.zeros(2, 3, 5, 7, dtype=torch.uint8)
    dst = torch.zeros(2, 3, 10, 14, dtype=torch.float16)
    D = _lib.ImageDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    fill_image(D, src, dst)
    assert (D.src, D.dst) == (src.data_ptr(), dst.data_ptr())
    assert (D.B, D.C, D.in_h, D.in_w, D.out_h, D.out_w, D.dtype, D.flags, D.reserved) == (2, 3, 5, 7, 10, 14, _lib.F16, 0, 0)
    C.memset(C.byref(D), 0xFF, C.sizeof(D))
    nhwc = torch.zeros(2, 5, 7, 3, dtype=torch.uint8)
    cl = torch.zeros(2, 3, 5, 7, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    fill_image(D, nhwc, cl, src_nhwc=True, reverse_channels=True)
    assert (D.B, D.C, D.in_h, D.in_w, D.out_h, D.out_w, D.dtype, D.flags, D.reserved) == (2, 3, 5, 7, 5, 7, _lib.BF16, 7, 0)
    one = torch.zeros(2, 1, 5, 7).contiguous(memory_format=torch.channels_last)                   # C = 1: both formats at once, the same bytes
    fill_image(D, src[:, :1].contiguous(), one)
    assert (D.C, D.dtype, D.flags) == (1, _lib.F32, 0)
