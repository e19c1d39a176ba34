"""CPU-side checks of the channels-last (MGACBAM_LAYOUT_NHWC) part of the C ABI (ABI 15) and of the Python layout decision.
No kernel is launched here: every call below must fail its argument checks before anything touches a device."""
import pytest
import torch

from abi_header import fake, read


def test_layout_flag_keeps_the_other_flags_bits(built_lib):
    from mga_yolo_amd import _lib
    assert _lib.LAYOUT_NHWC & _lib.FWD_SAVE_PROJ == 0 and _lib.LAYOUT_NHWC & _lib.BWD_HAVE_PROJ == 0   # bit 0 keeps its meaning


def test_size_queries_are_declared_bound_and_layout_aware(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for name in ("mgacbam_fwd_ws_bytes", "mgacbam_bwd_scratch_bytes_flags"):
        assert name in _lib.HEADERS["mgacbam.h"].symbols and name in read("mgacbam.h").functions and hasattr(lib, name)
    for B, Cc, H, W, hid, k in [(2, 64, 16, 16, 4, 7), (32, 64, 80, 80, 4, 7), (1, 48, 17, 17, 3, 3), (3, 5, 7, 9, 1, 5), (2, 1024, 10, 10, 64, 7)]:
        assert lib.mgacbam_fwd_ws_bytes(B, Cc, H, W, hid, 0) == 0
        assert lib.mgacbam_fwd_ws_bytes(B, Cc, H, W, hid, _lib.FWD_SAVE_PROJ) == 0
        ws = lib.mgacbam_fwd_ws_bytes(B, Cc, H, W, hid, _lib.LAYOUT_NHWC)
        assert ws > 0 and ws % 16 == 0
        assert ws >= B * (4 * Cc + 4) * 4                          # at least one chunk of partials per sample
        assert lib.mgacbam_bwd_scratch_bytes_flags(B, Cc, H, W, hid, k, 0) == lib.mgacbam_bwd_scratch_bytes(B, Cc, H, W, hid, k)
        assert lib.mgacbam_bwd_scratch_bytes_flags(B, Cc, H, W, hid, k, _lib.LAYOUT_NHWC) > 0
        assert _lib.scratch_bytes(B, Cc, H, W, hid, k, _lib.LAYOUT_NHWC) == lib.mgacbam_bwd_scratch_bytes_flags(B, Cc, H, W, hid, k, _lib.LAYOUT_NHWC)
        assert _lib.fwd_ws_bytes(B, Cc, H, W, hid, _lib.LAYOUT_NHWC) == ws and _lib.fwd_ws_bytes(B, Cc, H, W, hid, 0) == 0
    assert lib.mgacbam_fwd_ws_bytes(0, 64, 8, 8, 4, _lib.LAYOUT_NHWC) == 0        # bad shape
    assert lib.mgacbam_bwd_scratch_bytes_flags(2, 64, 8, 8, 4, 4, _lib.LAYOUT_NHWC) == 0   # even k


def _levels(_lib, B, Cc, H, W, hid, k, dtype):
    P = _lib.Params(*([fake()] * 6), hid, k, 1, 1e-4, 1e-6)
    fl = (_lib.FwdLevel * 1)()
    F = fl[0]
    F.x = F.mask = F.y = F.ctx = F.ws = fake()
    F.p, F.B, F.C, F.H, F.W, F.dtype, F.flags = P, B, Cc, H, W, dtype, _lib.LAYOUT_NHWC
    F.ctx_bytes = _lib.ctx_bytes(B, Cc, H, W, hid)
    F.ws_bytes = _lib.fwd_ws_bytes(B, Cc, H, W, hid, _lib.LAYOUT_NHWC)
    bl = (_lib.BwdLevel * 1)()
    Bw = bl[0]
    for f in ("x", "mask", "gy", "ctx", "scratch", "gx", "gmask", "gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta"):
        setattr(Bw, f, fake())
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = P, B, Cc, H, W, dtype, _lib.LAYOUT_NHWC
    Bw.ctx_bytes = _lib.ctx_bytes(B, Cc, H, W, hid)
    Bw.scratch_bytes = _lib.scratch_bytes(B, Cc, H, W, hid, k, _lib.LAYOUT_NHWC)
    return fl, bl


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_undersized_nhwc_work_buffers_are_an_error_not_a_launch(built_lib, dtype):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    B, Cc, H, W, hid, k = 2, 64, 16, 16, 4, 7
    fl, bl = _levels(_lib, B, Cc, H, W, hid, k, dtype)
    need_ws = fl[0].ws_bytes
    fl[0].ws_bytes = 0
    assert lib.mgacbam_forward(fl, 1, None) == _lib.E_SIZE
    msg = lib.mgacbam_last_error().decode()
    assert "ws" in msg and "holds 0 bytes" in msg
    fl[0].ws_bytes = need_ws
    fl[0].ws = None
    assert lib.mgacbam_forward(fl, 1, None) == _lib.E_NULL
    fl[0].ws = fake()
    fl[0].ctx_bytes -= 16
    assert lib.mgacbam_forward(fl, 1, None) == _lib.E_SIZE and b"ctx" in lib.mgacbam_last_error()
    bl[0].scratch_bytes = 16
    assert lib.mgacbam_backward(bl, 1, None) == _lib.E_SIZE and b"scratch" in lib.mgacbam_last_error()
    # the NCHW requirement is not the NHWC one: a scratch sized by the NCHW query for this shape is refused when it is smaller
    nchw = lib.mgacbam_bwd_scratch_bytes(B, Cc, H, W, hid, k)
    nhwc = _lib.scratch_bytes(B, Cc, H, W, hid, k, _lib.LAYOUT_NHWC)
    if nchw < nhwc:
        bl[0].scratch_bytes = nchw
        assert lib.mgacbam_backward(bl, 1, None) == _lib.E_SIZE


def test_misaligned_nhwc_features_are_refused(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    fl, bl = _levels(_lib, 2, 64, 16, 16, 4, 7, _lib.F32)
    fl[0].x = fake() + 4                                          # fp32 with C % 4 == 0: 16-byte lanes
    assert lib.mgacbam_forward(fl, 1, None) == _lib.E_ALIGN
    fl[0].x = fake()
    fl[0].y = fake() + 8
    assert lib.mgacbam_forward(fl, 1, None) == _lib.E_ALIGN
    for f in ("x", "gy", "gx"):
        setattr(bl[0], f, fake() + 4)
        assert lib.mgacbam_backward(bl, 1, None) == _lib.E_ALIGN, f
        setattr(bl[0], f, fake())
    fl2, _ = _levels(_lib, 2, 64, 16, 16, 4, 7, _lib.BF16)        # bf16 with C % 8 == 0: 16-byte lanes as well
    fl2[0].x = fake() + 8
    assert lib.mgacbam_forward(fl2, 1, None) == _lib.E_ALIGN


def test_ws_query_covers_every_element_type(built_lib):
    """The queries take no element type: the answer must cover the largest requirement (fp32 and fp16 chunk differently)."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for Cc in (8, 64, 256, 512, 1024, 2048, 48, 5):
        for dtype in (0, 1, 2):
            fl, bl = _levels(_lib, 3, Cc, 9, 11, 4, 5, dtype)
            fl[0].ctx_bytes -= 16                                  # stop at the ctx check, which follows the ws check
            fl[0].ws_bytes = lib.mgacbam_fwd_ws_bytes(3, Cc, 9, 11, 4, _lib.LAYOUT_NHWC)
            assert lib.mgacbam_forward(fl, 1, None) == _lib.E_SIZE and b"ctx" in lib.mgacbam_last_error(), (Cc, dtype)


def test_layout_decision():
    from mga_yolo_amd.functional import _is_nhwc
    x = torch.randn(2, 8, 5, 6)
    assert not _is_nhwc(x)                                                          # NCHW
    assert _is_nhwc(x.to(memory_format=torch.channels_last))                        # channels_last
    for shape in [(2, 1, 5, 6), (2, 8, 1, 1)]:                                      # ambiguous: both contiguities hold -> NCHW path
        t = torch.randn(*shape).to(memory_format=torch.channels_last)
        assert t.is_contiguous() and not _is_nhwc(t)
    assert not _is_nhwc(x[:, :, :, ::2])                                            # arbitrary strides: NCHW path (copied)
    assert not _is_nhwc(x.to(memory_format=torch.channels_last)[:, :4])
    assert not _is_nhwc(x.permute(0, 1, 3, 2))
    assert not _is_nhwc(torch.randn(8, 5, 6))


# ---------------------------------------------------------------------------------------------------------------------------
# coverage of tests/test_gpu_channels_last_edges.py: its rows are checked against a copy of host.cuh's nhwc_vec / nhwc_geo, and that copy
# against the library's own size query, so a change of the tiling fails here instead of silently thinning what the GPU rows reach
# ---------------------------------------------------------------------------------------------------------------------------
def _nhwc_vec(C, dtype):
    return 8 if (dtype != "f32" and C % 8 == 0) else (4 if C % 4 == 0 else 1)


def _nhwc_geo(C, H, W, vec):
    ng = -(-C // vec)
    cs = max(4, min(1 << (ng - 1).bit_length(), 64))
    ch = (256 // cs) * (4 if vec == 8 else 8)
    ntile = -(-(H * W) // ch)
    rp = -(-ntile // 64)
    nchunk = -(-ntile // rp)
    return dict(vec=vec, ng=ng, cs=cs, nj=-(-ng // cs), ch=ch, ntile=ntile, rp=rp, nchunk=nchunk, ragged=ntile % rp != 0,
                ncb=-(-C // 64), fold_partial=C > 64 and C % 64 != 0)


def test_channels_last_edge_rows_reach_every_tiling_branch(built_lib):
    from mga_yolo_amd import _lib
    from test_gpu_channels_last_edges import EDGE_ROWS
    lib = _lib.load()
    rows = []
    for name, dt, B, C, H, W, k, kind, mask3d, mask_grad in EDGE_ROWS:
        nchunk = max(_nhwc_geo(C, H, W, _nhwc_vec(C, d))["nchunk"] for d in ("f32", "f16"))
        assert lib.mgacbam_fwd_ws_bytes(B, C, H, W, 4, _lib.LAYOUT_NHWC) == B * nchunk * (4 * C + 4) * 4, name
        rows.append(dict(_nhwc_geo(C, H, W, _nhwc_vec(C, dt)), name=name, dt=dt, B=B, C=C, H=H, W=W, k=k, kind=kind, mask3d=mask3d,
                         mask_grad=mask_grad))
    branches = {
        "vec 1, nj 3, partial fold block": lambda r: r["vec"] == 1 and r["nj"] >= 3 and r["fold_partial"],
        "vec 1, rp 2, ragged": lambda r: r["vec"] == 1 and r["rp"] >= 2 and r["ragged"],
        "vec 4, cs 4, rp 2, ragged": lambda r: r["vec"] == 4 and r["cs"] == 4 and r["rp"] >= 2 and r["ragged"],
        "vec 4, cs 64, rp 2, ragged": lambda r: r["vec"] == 4 and r["cs"] == 64 and r["rp"] >= 2 and r["ragged"],
        "vec 4 in half precision, nj 2": lambda r: r["vec"] == 4 and r["dt"] != "f32" and r["nj"] >= 2,
        "vec 8, nj 2, partial fold block": lambda r: r["vec"] == 8 and r["nj"] >= 2 and r["fold_partial"],
        "vec 8, rp 5, ragged": lambda r: r["vec"] == 8 and r["rp"] >= 5 and r["ragged"],
        "vec 1 in half precision": lambda r: r["vec"] == 1 and r["dt"] != "f32",
        "W = 1": lambda r: r["W"] == 1,
        "a tile spans many image rows": lambda r: r["cs"] == 4 and r["W"] == 3 and r["ch"] // r["W"] >= 100 and r["ntile"] >= 2,
        "a tile inside one image row": lambda r: r["W"] > r["ch"],
        "fp16": lambda r: r["dt"] == "f16",
        "bf16": lambda r: r["dt"] == "bf16",
        "3-D mask": lambda r: r["mask3d"],
        "mask without grad": lambda r: r["kind"] != "none" and not r["mask_grad"],
        "raw-probability mask": lambda r: r["kind"] == "prob",
        "B = 1": lambda r: r["B"] == 1,
        "B > 1, not a multiple of 8": lambda r: r["B"] > 1 and r["B"] % 8 != 0,
    }
    missed = [b for b, hit in branches.items() if not any(hit(r) for r in rows)]
    assert not missed, missed
    assert {1, 3, 5, 9, 15} <= {r["k"] for r in rows}
    assert {"randn", "sparse", "none", "tiny", "all_negative", "prob", "mixed"} <= {r["kind"] for r in rows}
