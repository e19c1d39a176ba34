"""CPU-side checks of the MaskSPADE layout flag (MGASPADE_LAYOUT_NHWC in mgaspade_level_t.flags) on the built library: that it is
MGACBAM_LAYOUT_NHWC's value, that a flagged level gets past the flags check and meets every later check, that every other bit is still
refused, and that the binding writes the field.  Levels are built over fake pointers as tests/test_abi_spade.py builds them: every
call here returns before anything is launched (there is no GPU here: a call that got past its checks would crash on the pointers)."""
import pytest
import torch

from abi_header import read
from test_abi_spade import _level

NHWC = 2
E_SHAPE, E_ALIGN, E_SIZE = -2, -4, -6


def _both(lib):
    return (lib.mgaspade_forward, lib.mgaspade_backward)


def test_a_flagged_level_passes_the_flags_check_and_meets_the_capacity_check(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for fn in _both(lib):
        arr = (_lib.SpadeLevel * 1)(_level(_lib, flags=NHWC, ctx_bytes=45311))
        assert fn(arr, 1, None) == E_SIZE
        msg = lib.mgacbam_last_error().decode()
        assert "holds" in msg and "needs" in msg, msg


def test_layout_constant():
    from mga_yolo_amd import _lib
    spade, cbam = read("mgaspade.h").constants["MGASPADE_LAYOUT_NHWC"], read("mgacbam.h").constants["MGACBAM_LAYOUT_NHWC"]
    assert spade == _lib.SPADE_LAYOUT_NHWC == NHWC == cbam == _lib.LAYOUT_NHWC


@pytest.mark.parametrize("what,over,fwd,bwd", [
    ("x misaligned", dict(x=0x10004), E_ALIGN, E_ALIGN),
    ("C % 16", dict(C=24), E_SHAPE, E_SHAPE),
    ("scratch too small", dict(scratch_bytes=43519), None, E_SIZE),
], ids=["x-misaligned", "C-24", "scratch-short"])
def test_errors_of_a_flagged_level(built_lib, what, over, fwd, bwd):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for fn, want in zip(_both(lib), (fwd, bwd)):
        if want is None:
            continue
        arr = (_lib.SpadeLevel * 1)(_level(_lib, flags=NHWC, **over))
        assert fn(arr, 1, None) == want, what
        assert lib.mgacbam_last_error()


@pytest.mark.parametrize("flags", [1, 3, 4, 6, 8, 0x10002])
def test_every_other_bit_is_still_refused(built_lib, flags):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for fn in _both(lib):
        arr = (_lib.SpadeLevel * 1)(_level(_lib, flags=flags))
        assert fn(arr, 1, None) == E_SHAPE
        assert "flags" in lib.mgacbam_last_error().decode()


def test_a_bad_flagged_level_fails_the_call_before_any_launch(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for fn in _both(lib):
        two = (_lib.SpadeLevel * 2)(_level(_lib), _level(_lib, flags=NHWC, C=24))
        assert fn(two, 2, None) == E_SHAPE


class _Cfg:
    hidden, bn, training, use_sigmoid_mask, eps, momentum = 16, False, True, True, 1e-6, 0.1


def test_fill_spade_writes_the_flag():
    from mga_yolo_amd import _lib
    from mga_yolo_amd._binding import fill_spade
    x = torch.zeros(2, 16, 8, 8).contiguous(memory_format=torch.channels_last)
    ctx = torch.zeros(64, dtype=torch.uint8)
    L = _lib.SpadeLevel()
    fill_spade(L, x, None, [None] * 6, _Cfg, None, ctx, y=torch.empty_like(x), flags=_lib.SPADE_LAYOUT_NHWC)
    assert L.flags == NHWC and (L.B, L.C, L.H, L.W) == (2, 16, 8, 8)
    fill_spade(L, x, None, [None] * 6, _Cfg, None, ctx, y=torch.empty_like(x))
    assert L.flags == 0
