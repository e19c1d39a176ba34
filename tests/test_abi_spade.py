"""CPU-side checks of the MaskSPADE entry points (include/mgaspade.h) on the built library: the size queries, and every argument error --
each returned before anything is launched (there is no GPU here: a call that got past its checks would fail differently).  The header
against the binding is tests/test_abi_headers.py's."""
import pytest

from abi_header import FAKE as P, a16


def test_size_queries(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    # hand-computed.  ctx = mean | rstd (B*C floats each) | two weight packs of 2*9*C*hidden floats | gamma (B*C*H*W fp32)
    assert lib.mgaspade_ctx_bytes(2, 16, 8, 8, 16) == 2 * a16(2 * 16 * 4) + 2 * (2 * 9 * 16 * 16 * 4) + 2 * 16 * 64 * 4 == 45312
    assert lib.mgaspade_ctx_bytes(1, 64, 20, 20, 64) == 2 * 64 * 4 + 2 * (2 * 9 * 64 * 64 * 4) + 64 * 400 * 4 == 692736
    # scratch = 4 + 2 plane sums | dW partials (nchunk, 2, C, hidden*9) | 9 tap planes | dW0 partials (tiles, hidden*10).
    # (2,16,8,8): 8x16 tiling -> 1 tile per sample, 2 tiles, 2 chunks;  (1,64,20,20): 32x4 tiling -> 5 tiles, 5 chunks
    assert lib.mgaspade_scratch_bytes(2, 16, 8, 8, 16) == (6 * 32 + 2 * 2 * 16 * 144 + 2 * 9 * 64 + 2 * 160) * 4 == 43520
    assert lib.mgaspade_scratch_bytes(1, 64, 20, 20, 64) == (6 * 64 + 5 * 2 * 64 * 576 + 9 * 400 + 5 * 640) * 4 == 1503296
    for fn in (lib.mgaspade_ctx_bytes, lib.mgaspade_scratch_bytes):
        prev = 0
        for B in (1, 2, 4, 8, 16):
            n = fn(B, 64, 20, 20, 64)
            assert n >= prev and n % 16 == 0
            prev = n
        assert fn(2, 64, 40, 40, 64) >= fn(2, 64, 20, 20, 64) and fn(2, 128, 20, 20, 64) >= fn(2, 64, 20, 20, 64)
        assert fn(2, 64, 20, 20, 64) >= fn(2, 64, 20, 20, 16)
        for bad in ((0, 16, 8, 8, 16), (2, 24, 8, 8, 16), (2, 2048, 8, 8, 16), (2, 16, 8, 8, 24), (2, 16, 8, 8, 128), (2, 16, 0, 8, 16)):
            assert fn(*bad) == 0
            assert lib.mgacbam_last_error()
    assert _lib.spade_ctx_bytes(2, 16, 8, 8, 16) == 45312 and _lib.spade_scratch_bytes(2, 16, 8, 8, 16) == 43520
    with pytest.raises(RuntimeError):
        _lib.spade_ctx_bytes(2, 24, 8, 8, 16)


def _level(_lib, **over):
    L = _lib.SpadeLevel()
    for n in ("x", "mask", "y", "gy", "gx", "gmask", "w0", "b0", "wg", "bg", "wb", "bb", "gw0", "gb0", "gwg", "gbg", "gwb", "gbb", "ctx", "scratch"):
        setattr(L, n, P)
    L.B, L.C, L.H, L.W, L.hidden, L.dtype = 2, 16, 8, 8, 16, _lib.F32
    L.norm_type, L.training, L.use_sigmoid_mask, L.save_gamma, L.eps, L.momentum, L.flags = _lib.NORM_IN, 1, 1, 1, 1e-6, 0.1, 0
    L.ctx_bytes, L.scratch_bytes = 45312, 43520
    for k, v in over.items():
        setattr(L, k, v)
    return L


CASES = [  # (what, overrides, expected code forward, expected code backward)  None = that direction does not look at it
    ("x NULL", dict(x=None), -1, -1), ("ctx NULL", dict(ctx=None), -1, -1), ("y NULL", dict(y=None), -1, None),
    ("gy NULL", dict(gy=None), None, -1), ("gx NULL", dict(gx=None), None, -1), ("scratch NULL", dict(scratch=None), None, -1),
    ("param NULL", dict(wb=None), -1, -1), ("param grad NULL", dict(gwg=None), None, -1),
    ("gmask without mask", dict(mask=None), None, -1),
    ("bn without running stats", dict(norm_type=1), -1, -1),
    ("flags", dict(flags=1), -2, -2), ("C % 16", dict(C=24), -2, -2), ("C > 1024", dict(C=2048), -2, -2), ("hidden % 16", dict(hidden=8), -2, -2),
    ("hidden > 64", dict(hidden=128), -2, -2), ("B = 0", dict(B=0), -2, -2), ("norm_type", dict(norm_type=7), -2, -2),
    ("one spatial element", dict(H=1, W=1), -2, None), ("dtype", dict(dtype=3), -3, -3),
    ("x misaligned", dict(x=0x10004), -4, -4), ("ctx misaligned", dict(ctx=0x10008), -4, -4), ("y misaligned", dict(y=0x10002), -4, None),
    ("gy misaligned", dict(gy=0x10004), None, -4), ("gx misaligned", dict(gx=0x10004), None, -4),
    ("scratch misaligned", dict(scratch=0x10004), None, -4),
    ("ctx too small", dict(ctx_bytes=45311), -6, -6), ("scratch too small", dict(scratch_bytes=43519), None, -6),
]


@pytest.mark.parametrize("what,over,fwd,bwd", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_come_before_any_launch(built_lib, what, over, fwd, bwd):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for fn, want in ((lib.mgaspade_forward, fwd), (lib.mgaspade_backward, bwd)):
        if want is None:
            continue
        arr = (_lib.SpadeLevel * 1)(_level(_lib, **over))
        assert fn(arr, 1, None) == want, what
        assert lib.mgacbam_last_error()
        if want == -6:
            msg = lib.mgacbam_last_error().decode()
            assert "holds" in msg and "needs" in msg


def test_level_count_and_null_array(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    arr = (_lib.SpadeLevel * 1)(_level(_lib))
    for fn in (lib.mgaspade_forward, lib.mgaspade_backward):
        assert fn(None, 1, None) == -1
        assert fn(arr, 0, None) == -5 and fn(arr, _lib.MAX_LEVELS + 1, None) == -5
    # a forward that keeps no gamma needs the smaller ctx only; the second level's error is found before the first is launched
    two = (_lib.SpadeLevel * 2)(_level(_lib), _level(_lib, C=24))
    assert lib.mgaspade_forward(two, 2, None) == -2
    small = 45312 - 2 * 16 * 64 * 4
    ok_small = (_lib.SpadeLevel * 1)(_level(_lib, save_gamma=0, ctx_bytes=small, C=24))
    assert lib.mgaspade_forward(ok_small, 1, None) == -2
    assert lib.mgaspade_forward((_lib.SpadeLevel * 1)(_level(_lib, save_gamma=0, ctx_bytes=small - 1)), 1, None) == -6
    assert lib.mgaspade_forward((_lib.SpadeLevel * 1)(_level(_lib, save_gamma=1, ctx_bytes=small)), 1, None) == -6
