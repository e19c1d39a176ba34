"""CPU-side checks of the channels-last mask head (MGAHEAD_LAYOUT_NHWC, ABI 15): the flag, the two layout-aware size queries and the
argument checks of NHWC levels.  No kernel is launched here: every call below must fail its argument checks before anything touches a
device."""
import pytest

from abi_header import fake, read


def test_head_layout_flag_keeps_the_other_flags_bits(built_lib):
    from mga_yolo_amd import _lib
    assert _lib.HEAD_LAYOUT_NHWC & (_lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32) == 0


# the head goldens' shapes, the checksum shapes, H*W % 4 != 0, C = 20 / 36 / 768, hidden = 8 / 192
SHAPES = [(2, 64, 16, 16, 16), (3, 48, 9, 11, 12), (32, 64, 80, 80, 16), (32, 128, 40, 40, 32), (32, 256, 20, 20, 64),
          (32, 512, 20, 20, 128), (8, 192, 160, 160, 48), (2, 256, 160, 160, 64), (1, 8, 2, 333, 8), (2, 20, 7, 9, 8),
          (2, 36, 5, 7, 8), (2, 768, 10, 10, 192), (1, 16, 5, 36, 200), (1, 8, 1, 500, 40), (4, 3, 6, 6, 8)]


def test_head_size_queries_are_declared_bound_and_layout_aware(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for name in ("mgahead_ctx_bytes_flags", "mgahead_bwd_scratch_bytes_flags"):
        assert name in _lib.HEADERS["mgacbam.h"].symbols and name in read("mgacbam.h").functions and hasattr(lib, name)
    for B, Cc, H, W, hid in SHAPES:
        for fl in (0, _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32):
            assert lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, fl) == lib.mgahead_ctx_bytes(B, Cc, H, W, hid)
            assert lib.mgahead_bwd_scratch_bytes_flags(B, Cc, H, W, hid, fl) == lib.mgahead_bwd_scratch_bytes(B, Cc, H, W, hid)
        for fl in (_lib.HEAD_LAYOUT_NHWC, _lib.HEAD_LAYOUT_NHWC | _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32):
            c = lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, fl)
            s = lib.mgahead_bwd_scratch_bytes_flags(B, Cc, H, W, hid, fl)
            assert c > 0 and c % 16 == 0 and s > 0 and s % 16 == 0
            assert c >= B * hid * H * W * 4 and s >= B * hid * H * W * 4          # z / g_a (B, hidden, H, W) fp32 at least
    for bad in [(0, 64, 8, 8, 16), (2, 0, 8, 8, 16), (2, 64, 8, 8, 0), (1, 8, 2, 501, 8)]:
        assert lib.mgahead_ctx_bytes_flags(*bad, _lib.HEAD_LAYOUT_NHWC) == 0
        assert lib.mgahead_bwd_scratch_bytes_flags(*bad, _lib.HEAD_LAYOUT_NHWC) == 0


def _levels(_lib, B, Cc, H, W, hid, dtype, flags):
    lib = _lib.load()
    P = _lib.HeadParams(*([fake()] * 8), hid, 1e-3, 0.03, 1)
    fl = (_lib.HeadFwdLevel * 1)()
    F = fl[0]
    F.x = F.logits = F.ctx = fake()
    F.ctx_bytes = lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, flags)
    F.p, F.B, F.C, F.H, F.W, F.dtype, F.flags = P, B, Cc, H, W, dtype, flags
    bl = (_lib.HeadBwdLevel * 1)()
    Bw = bl[0]
    for f in ("x", "g_logits", "ctx", "scratch", "gx", "gw1", "gbn_weight", "gbn_bias", "gwh", "gbh"):
        setattr(Bw, f, fake())
    Bw.ctx_bytes = lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, flags)
    Bw.scratch_bytes = lib.mgahead_bwd_scratch_bytes_flags(B, Cc, H, W, hid, flags)
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = P, B, Cc, H, W, dtype, flags
    return fl, bl


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_undersized_nhwc_head_buffers_are_an_error_not_a_launch(built_lib, dtype):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for B, Cc, H, W, hid in [(2, 64, 16, 16, 16), (3, 36, 7, 9, 8), (2, 768, 10, 10, 192)]:
        NH = _lib.HEAD_LAYOUT_NHWC
        fl, bl = _levels(_lib, B, Cc, H, W, hid, dtype, NH)
        fl[0].ctx_bytes -= 16
        assert lib.mgahead_forward(fl, 1, None) == _lib.E_SIZE and b"ctx" in lib.mgacbam_last_error()
        bl[0].scratch_bytes -= 16
        assert lib.mgahead_backward(bl, 1, None) == _lib.E_SIZE and b"scratch" in lib.mgacbam_last_error()
        bl[0].scratch_bytes += 16
        bl[0].ctx_bytes -= 16
        assert lib.mgahead_backward(bl, 1, None) == _lib.E_SIZE and b"ctx" in lib.mgacbam_last_error()
        # the capacity is checked against the NHWC layout: a buffer sized by the NCHW query is refused where it is smaller
        nc, nh = lib.mgahead_ctx_bytes(B, Cc, H, W, hid), lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, NH)
        if nc < nh:
            fl[0].ctx_bytes = nc
            assert lib.mgahead_forward(fl, 1, None) == _lib.E_SIZE
        ns, nhs = lib.mgahead_bwd_scratch_bytes(B, Cc, H, W, hid), lib.mgahead_bwd_scratch_bytes_flags(B, Cc, H, W, hid, NH)
        if ns < nhs:
            bl[0].ctx_bytes = nh
            bl[0].scratch_bytes = ns
            assert lib.mgahead_backward(bl, 1, None) == _lib.E_SIZE


def test_misaligned_nhwc_head_features_are_refused(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    NH = _lib.HEAD_LAYOUT_NHWC
    # (dtype, C, misalignment in bytes): fp32 with C % 4 == 0 needs 16 B; fp16 / bf16 with C % 8 == 0 16 B, with C % 4 == 0 (only) 8 B
    for dtype, Cc, off in [(_lib.F32, 64, 4), (_lib.F32, 64, 8), (_lib.BF16, 64, 8), (_lib.F16, 64, 4), (_lib.F16, 36, 4), (_lib.F32, 36, 8)]:
        for extra in (0, _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32):
            fl, bl = _levels(_lib, 2, Cc, 8, 8, 16, dtype, NH | extra)
            fl[0].x = fake() + off
            assert lib.mgahead_forward(fl, 1, None) == _lib.E_ALIGN, (dtype, Cc, off)
            for f in ("x", "gx"):
                setattr(bl[0], f, fake() + off)
                assert lib.mgahead_backward(bl, 1, None) == _lib.E_ALIGN, (dtype, Cc, off, f)
                setattr(bl[0], f, fake())
