"""CPU-side checks of the target-pyramid entry points (include/mgatargets.h) on the built library: the scratch query, and every refusal --
each returned, with its message, before anything is launched (there is no GPU here: a call that got past its checks would fail
differently).  The header against the binding is tests/test_abi_headers.py's."""
import ctypes as C

import pytest

from abi_header import FAKE as P, a16


def _desc(_lib, strides=(8, 16, 32), **over):
    D = _lib.TargetsDesc()
    D.src = P
    for l, s in enumerate(strides):
        D.dst[l], D.stride[l] = P + 0x1000 * (l + 1), s
    D.n_levels, D.B, D.H, D.W = len(strides), 2, 100, 76
    D.src_dtype, D.method, D.flags = _lib.TGT_SRC_U8, _lib.TGT_AVGPOOL, 0
    for k, v in over.items():
        if k.startswith("dst"):
            D.dst[int(k[3:])] = v
        else:
            setattr(D, k, v)
    return D


# the closing's scratch at (2, 100, 76), strides 8 / 16 / 32: levels of 13x10, 7x5 and 4x3 cells, fp32, each 16-byte aligned
CLOSE_BYTES = a16(2 * 13 * 10 * 4) + a16(2 * 7 * 5 * 4) + a16(2 * 4 * 3 * 4)
CLOSE = dict(method=1, flags=1, scratch=P + 0x8000, scratch_bytes=CLOSE_BYTES)

CASES = [  # (what, strides, overrides, expected code of mgatgt_forward)
    ("src NULL", (8, 16, 32), dict(src=None), -1), ("dst NULL", (8, 16, 32), dict(dst1=None), -1),
    ("n_levels 0", (8, 16, 32), dict(n_levels=0), -5), ("n_levels 5", (8, 16, 32), dict(n_levels=5), -5),
    ("stride 0", (8, 0), {}, -7), ("stride 3", (3,), {}, -7), ("stride 128", (64, 128), {}, -7), ("stride 1", (1, 2), {}, -7),
    ("descending strides", (16, 8), {}, -7), ("repeated stride", (8, 8), {}, -7),
    ("B*H*W = 2^31", (8,), dict(B=8, H=16384, W=16384), -2), ("B*H*W > 2^31", (8,), dict(B=64, H=8192, W=8192), -2),
    ("B = 0", (8,), dict(B=0), -2), ("H = 0", (8,), dict(H=0), -2), ("W < 0", (8,), dict(W=-4), -2),
    ("unknown method", (8,), dict(method=2), -7), ("unknown dtype", (8,), dict(src_dtype=2), -3),
    ("unknown flag", (8,), dict(method=1, flags=2), -7),
    ("closing with avgpool", (8, 16, 32), dict(CLOSE, method=0), -7),
    ("closing, scratch NULL", (8, 16, 32), dict(CLOSE, scratch=None), -1),
    ("closing, scratch short", (8, 16, 32), dict(CLOSE, scratch_bytes=CLOSE_BYTES - 1), -6),
    ("closing, scratch misaligned", (8, 16, 32), dict(CLOSE, scratch=P + 0x8004), -4),
    ("dst misaligned", (8, 16, 32), dict(dst2=P + 0x3002), -4), ("dst misaligned by one", (8,), dict(dst0=P + 0x1001), -4),
    ("fp32 src misaligned", (8,), dict(src_dtype=1, src=P + 2), -4),
]


@pytest.mark.parametrize("what,strides,over,want", CASES, ids=[c[0] for c in CASES])
def test_refusals_come_with_a_message_before_any_launch(built_lib, what, strides, over, want):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    D = _desc(_lib, strides, **over)
    assert lib.mgatgt_forward(C.byref(D), None) == want, what
    assert lib.mgacbam_last_error(), what
    if want == -6:
        msg = lib.mgacbam_last_error().decode()
        assert "holds" in msg and "needs" in msg


def test_null_descriptor(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    assert lib.mgatgt_forward(None, None) == -1 and lib.mgacbam_last_error()
    assert lib.mgatgt_scratch_bytes(None) == 0 and lib.mgacbam_last_error()


def test_the_largest_size_passes_the_shape_check(built_lib):
    """B*H*W = 2^31 - 2^16 is in range: the call gets as far as the next check (a NULL dst)"""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    D = _desc(_lib, (8,), B=1, H=32768, W=65534, dst0=None)
    assert 32768 * 65534 < 2 ** 31 and lib.mgatgt_forward(C.byref(D), None) == -1
    assert b"dst[0]" in lib.mgacbam_last_error()


def test_scratch_bytes(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    q = lambda D: lib.mgatgt_scratch_bytes(C.byref(D))
    # nothing without the flag, and no message: 0 is the answer, not a refusal
    for method in (0, 1):
        assert q(_desc(_lib, method=method)) == 0 and not lib.mgacbam_last_error()
        assert _lib.targets_scratch_bytes(_desc(_lib, method=method)) == 0
    # with it: every level, whatever pointers the descriptor carries (the query reads none)
    assert q(_desc(_lib, **CLOSE)) == CLOSE_BYTES == 1040 + 288 + 96 and not lib.mgacbam_last_error()
    assert q(_desc(_lib, src=None, dst0=None, method=1, flags=1)) == CLOSE_BYTES
    assert q(_desc(_lib, (8,), method=1, flags=1)) == 1040 and q(_desc(_lib, (8, 16), method=1, flags=1)) == 1040 + 288
    assert q(_desc(_lib, (2, 64), method=1, flags=1)) == a16(2 * 50 * 38 * 4) + a16(2 * 2 * 2 * 4)
    assert q(_desc(_lib, (4, 8, 16, 32), method=1, flags=1, B=1, H=7, W=5)) == a16(2 * 2 * 4) + 3 * 16
    # a descriptor the call would refuse: 0 with the message
    for bad in (dict(method=0, flags=1), dict(method=1, flags=1, n_levels=0), dict(method=1, flags=1, B=0)):
        assert q(_desc(_lib, **bad)) == 0 and lib.mgacbam_last_error()
        with pytest.raises(RuntimeError):
            _lib.targets_scratch_bytes(_desc(_lib, **bad))
    assert q(_desc(_lib, (8, 4), method=1, flags=1)) == 0 and b"ascending" in lib.mgacbam_last_error()


def test_fill_helper_sets_every_field():
    import torch
    from mga_yolo_amd import _lib
    from mga_yolo_amd._binding import fill_targets
    src = torch.zeros(2, 100, 76, dtype=torch.uint8)
    dsts = [torch.zeros(2, 1, 13, 10), torch.zeros(2, 1, 7, 5)]
    D = _lib.TargetsDesc()
    C.memset(C.byref(D), 0xFF, C.sizeof(D))                                  # every field starts as garbage
    fill_targets(D, src, dsts, (8, 16), _lib.TGT_MAXPOOL)
    assert D.src == src.data_ptr() and [D.dst[l] for l in range(4)] == [dsts[0].data_ptr(), dsts[1].data_ptr(), None, None]
    assert list(D.stride) == [8, 16, 0, 0] and (D.n_levels, D.B, D.H, D.W) == (2, 2, 100, 76)
    assert (D.src_dtype, D.method, D.flags, D.reserved, D.scratch, D.scratch_bytes) == (_lib.TGT_SRC_U8, _lib.TGT_MAXPOOL, 0, 0, None, 0)
    scratch = torch.zeros(2048, dtype=torch.uint8)
    fill_targets(D, src.float(), dsts, (8, 16), _lib.TGT_MAXPOOL, _lib.TGT_CLOSE3, scratch)
    assert (D.src_dtype, D.flags, D.scratch, D.scratch_bytes) == (_lib.TGT_SRC_F32, _lib.TGT_CLOSE3, scratch.data_ptr(), 2048)
