"""CPU-side checks of the channels-last part of the MaskECA C ABI (MGACBAM_LAYOUT_NHWC on mgacbam_eca_*_level_t, still ABI 15) and of
the rows tests/test_gpu_eca_channels_last.py runs at the corners of the tiling.  No kernel is launched here: every call below must fail
its argument checks before anything touches a device."""
import ctypes as C

import pytest

from abi_header import a16, fake, read

SHAPES = [(1, 1, 1, 1), (2, 64, 16, 16), (32, 64, 80, 80), (32, 128, 40, 40), (32, 256, 20, 20), (1, 48, 17, 17), (3, 5, 7, 9),
          (2, 1024, 10, 10), (2, 130, 48, 47), (1, 72, 140, 120), (11, 7, 30, 31), (5, 12, 700, 3), (2, 4096, 4, 4)]


def test_size_queries_are_declared_bound_and_layout_aware(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for name in ("mgacbam_eca_ctx_bytes_flags", "mgacbam_eca_scratch_bytes_flags"):
        assert name in _lib.HEADERS["mgacbam.h"].symbols and name in read("mgacbam.h").functions and hasattr(lib, name)
    N = _lib.LAYOUT_NHWC
    for B, Cc, H, W in SHAPES:
        ctx0, scr0 = lib.mgacbam_eca_ctx_bytes(B, Cc, H, W), lib.mgacbam_eca_scratch_bytes(B, Cc, H, W)
        assert ctx0 > 0 and scr0 > 0
        assert lib.mgacbam_eca_ctx_bytes_flags(B, Cc, H, W, 0) == ctx0 == _lib.eca_ctx_bytes(B, Cc, H, W)
        assert lib.mgacbam_eca_scratch_bytes_flags(B, Cc, H, W, 0) == scr0 == _lib.eca_scratch_bytes(B, Cc, H, W)
        ctx1, scr1 = lib.mgacbam_eca_ctx_bytes_flags(B, Cc, H, W, N), lib.mgacbam_eca_scratch_bytes_flags(B, Cc, H, W, N)
        assert ctx1 >= ctx0 + B * (2 * Cc + 4) * 4 and ctx1 % 16 == 0   # at least one chunk of partials per sample
        assert scr1 >= scr0 + B * Cc * 4 and scr1 % 16 == 0
        assert _lib.eca_ctx_bytes(B, Cc, H, W, N) == ctx1 and _lib.eca_scratch_bytes(B, Cc, H, W, N) == scr1
        sizes = [(lib.mgacbam_eca_ctx_bytes_flags(b, Cc, H, W, N), lib.mgacbam_eca_scratch_bytes_flags(b, Cc, H, W, N)) for b in (1, 2, 3, 8, 9, 33)]
        for prev, cur in zip(sizes, sizes[1:]):                      # monotone in B (16-byte rounding: not strictly at C = 1)
            assert cur[0] >= prev[0] and cur[1] >= prev[1], (Cc, H, W)
        assert sizes[-1][0] > sizes[0][0] and sizes[-1][1] > sizes[0][1]
    assert lib.mgacbam_eca_ctx_bytes_flags(0, 64, 8, 8, N) == 0       # bad shape
    assert lib.mgacbam_eca_scratch_bytes_flags(2, 64, 0, 8, N) == 0
    assert lib.mgacbam_eca_ctx_bytes_flags(2, 64, 8, 8, 1) == 0       # unknown flag bit
    assert lib.mgacbam_eca_scratch_bytes_flags(2, 64, 8, 8, 4) == 0


def _levels(_lib, B, Cc, H, W, k, dtype, flags):
    P = _lib.EcaParams(fake(), fake(), k, 1, 1e-4, 1e-6)
    fl = (_lib.EcaFwdLevel * 1)()
    F = fl[0]
    F.x = F.mask = F.y = F.ctx = fake()
    F.p, F.B, F.C, F.H, F.W, F.dtype, F.flags = P, B, Cc, H, W, dtype, flags
    F.ctx_bytes = _lib.eca_ctx_bytes(B, Cc, H, W, flags)
    bl = (_lib.EcaBwdLevel * 1)()
    Bw = bl[0]
    for f in ("x", "mask", "gy", "ctx", "scratch", "gx", "gmask", "gw", "gbeta"):
        setattr(Bw, f, fake())
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = P, B, Cc, H, W, dtype, flags
    Bw.ctx_bytes = _lib.eca_ctx_bytes(B, Cc, H, W, flags)
    Bw.scratch_bytes = _lib.eca_scratch_bytes(B, Cc, H, W, flags)
    return fl, bl


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_nchw_sized_work_buffers_are_refused_for_an_nhwc_level(built_lib, dtype):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    B, Cc, H, W, k = 2, 64, 16, 16, 5
    fl, bl = _levels(_lib, B, Cc, H, W, k, dtype, _lib.LAYOUT_NHWC)
    fl[0].ctx_bytes = lib.mgacbam_eca_ctx_bytes(B, Cc, H, W)
    assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_SIZE
    msg = lib.mgacbam_last_error().decode()
    assert "ctx" in msg and f"holds {fl[0].ctx_bytes} bytes" in msg
    bl[0].scratch_bytes = lib.mgacbam_eca_scratch_bytes(B, Cc, H, W)
    assert lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_SIZE
    msg = lib.mgacbam_last_error().decode()
    assert "scratch" in msg and f"holds {bl[0].scratch_bytes} bytes" in msg
    bl[0].scratch_bytes = _lib.eca_scratch_bytes(B, Cc, H, W, _lib.LAYOUT_NHWC)
    bl[0].ctx_bytes = lib.mgacbam_eca_ctx_bytes(B, Cc, H, W)
    assert lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_SIZE and b"ctx" in lib.mgacbam_last_error()


def test_query_covers_every_element_type(built_lib):
    """The queries take no element type: a buffer of the queried size passes the capacity checks for fp32, fp16 and bf16 (which chunk
    differently), so the call gets as far as the NEXT level's failing check."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for Cc in (8, 64, 256, 512, 1024, 2048, 48, 5):
        for dtype in (0, 1, 2):
            fl, bl = _levels(_lib, 3, Cc, 9, 11, 3, dtype, _lib.LAYOUT_NHWC)
            two = (_lib.EcaFwdLevel * 2)()
            C.memmove(C.byref(two[0]), C.byref(fl[0]), C.sizeof(_lib.EcaFwdLevel))
            C.memmove(C.byref(two[1]), C.byref(fl[0]), C.sizeof(_lib.EcaFwdLevel))
            two[1].dtype = 7                                          # every level is checked before any launch
            assert lib.mgacbam_eca_forward(two, 2, None) == -3, (Cc, dtype, lib.mgacbam_last_error())
            twob = (_lib.EcaBwdLevel * 2)()
            C.memmove(C.byref(twob[0]), C.byref(bl[0]), C.sizeof(_lib.EcaBwdLevel))
            C.memmove(C.byref(twob[1]), C.byref(bl[0]), C.sizeof(_lib.EcaBwdLevel))
            twob[1].dtype = 7
            assert lib.mgacbam_eca_backward(twob, 2, None) == -3, (Cc, dtype, lib.mgacbam_last_error())


def test_misaligned_nhwc_features_and_unknown_flags_are_refused(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    fl, bl = _levels(_lib, 2, 64, 16, 16, 5, _lib.F32, _lib.LAYOUT_NHWC)
    fl[0].x = fake() + 4                                          # fp32 with C % 4 == 0: 16-byte lanes
    assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_ALIGN
    fl[0].x = fake()
    fl[0].y = fake() + 8
    assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_ALIGN
    for f in ("x", "gy", "gx"):
        setattr(bl[0], f, fake() + 4)
        assert lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_ALIGN, f
        setattr(bl[0], f, fake())
    fl2, _ = _levels(_lib, 2, 64, 16, 16, 5, _lib.BF16, _lib.LAYOUT_NHWC)     # bf16 with C % 8 == 0: 16-byte lanes as well
    fl2[0].x = fake() + 8
    assert lib.mgacbam_eca_forward(fl2, 1, None) == _lib.E_ALIGN
    fl3, bl3 = _levels(_lib, 2, 6, 16, 16, 3, _lib.F16, _lib.LAYOUT_NHWC)     # C = 6: scalar lanes, 2-byte alignment is enough ...
    fl3[0].x = fake() + 2
    fl3[0].ctx_bytes = 0                                                      # ... so the call gets past it, to the capacity check
    assert lib.mgacbam_eca_forward(fl3, 1, None) == _lib.E_SIZE
    fl3[0].x = fake() + 1
    assert lib.mgacbam_eca_forward(fl3, 1, None) == _lib.E_ALIGN
    for bad in (1, 4, _lib.LAYOUT_NHWC | 8, 1 << 30):
        fl, bl = _levels(_lib, 2, 64, 16, 16, 5, _lib.F32, _lib.LAYOUT_NHWC)
        fl[0].flags = bl[0].flags = bad
        rc = lib.mgacbam_eca_forward(fl, 1, None)
        assert rc < 0 and b"flag" in lib.mgacbam_last_error(), bad
        rc = lib.mgacbam_eca_backward(bl, 1, None)
        assert rc < 0 and b"flag" in lib.mgacbam_last_error(), bad
    fl, bl = _levels(_lib, 2, 64, 16, 16, 5, _lib.F32, _lib.LAYOUT_NHWC)
    fl[0].C = bl[0].C = 4100                                        # a channels-last level keeps 3 floats per channel in LDS
    assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_SHAPE and lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_SHAPE


def test_plan_signature_keeps_its_default():
    import inspect
    from mga_yolo_amd.plan import EcaPyramidPlan
    p = inspect.signature(EcaPyramidPlan.__init__).parameters
    assert p["channels_last"].default is False and list(p)[-1] == "channels_last"


# ---------------------------------------------------------------------------------------------------------------------------
# coverage of tests/test_gpu_eca_channels_last.py: its rows are checked against a copy of host.cuh's nhwc_vec / nhwc_geo, and that copy
# against the library's own size queries, so a change of the tiling fails here instead of silently thinning what the GPU rows reach
# ---------------------------------------------------------------------------------------------------------------------------
def _nhwc_vec(Cc, dtype):
    return 8 if (dtype != "f32" and Cc % 8 == 0) else (4 if Cc % 4 == 0 else 1)


def _nhwc_geo(Cc, H, W, vec):
    ng = -(-Cc // vec)
    cs = max(4, min(1 << (ng - 1).bit_length(), 64))
    ch = (256 // cs) * (4 if vec == 8 else 8)
    ntile = -(-(H * W) // ch)
    rp = -(-ntile // 64)
    nchunk = -(-ntile // rp)
    return dict(vec=vec, ng=ng, cs=cs, nj=-(-ng // cs), ch=ch, ntile=ntile, rp=rp, nchunk=nchunk, ragged=ntile % rp != 0,
                ncb=-(-Cc // 64), fold_partial=Cc > 64 and Cc % 64 != 0)


def test_eca_edge_rows_reach_every_tiling_branch(built_lib):
    from mga_yolo_amd import _lib
    from test_gpu_channels_last_edges import EDGE_ROWS
    from test_gpu_eca_channels_last import ECA_EDGE_ROWS
    lib = _lib.load()
    N = _lib.LAYOUT_NHWC
    cbam = {(dt, B, Cc, H, W): (kind, m3, mg) for _, dt, B, Cc, H, W, _, kind, m3, mg in EDGE_ROWS}
    rows = []
    for name, dt, B, Cc, H, W, k, kind, mask3d, mask_grad in ECA_EDGE_ROWS:
        assert cbam[(dt, B, Cc, H, W)] == (kind, mask3d, mask_grad), name       # shapes and mask kinds are the MaskCBAM rows'
        nchunk = max(_nhwc_geo(Cc, H, W, _nhwc_vec(Cc, d))["nchunk"] for d in ("f32", "f16"))
        assert lib.mgacbam_eca_ctx_bytes_flags(B, Cc, H, W, N) - lib.mgacbam_eca_ctx_bytes(B, Cc, H, W) == a16(B * nchunk * (2 * Cc + 4) * 4), name
        assert lib.mgacbam_eca_scratch_bytes_flags(B, Cc, H, W, N) - lib.mgacbam_eca_scratch_bytes(B, Cc, H, W) == a16(B * nchunk * Cc * 4), name
        rows.append(dict(_nhwc_geo(Cc, H, W, _nhwc_vec(Cc, dt)), name=name, dt=dt, B=B, C=Cc, H=H, W=W, k=k, kind=kind, mask3d=mask3d,
                         mask_grad=mask_grad))
    want = [("f32", 130, 23, 17), ("f32", 130, 48, 47), ("f32", 16, 190, 190), ("f32", 256, 40, 52), ("f16", 260, 20, 13), ("bf16", 520, 12, 12),
            ("bf16", 72, 140, 120), ("f16", 64, 100, 100), ("f32", 3, 9, 1), ("f32", 12, 700, 3), ("f32", 7, 30, 31), ("f32", 20, 37, 41)]
    assert [(r["dt"], r["C"], r["H"], r["W"]) for r in rows] == want
    branches = {
        "vec 1, nj 3, partial fold block": lambda r: r["vec"] == 1 and r["nj"] >= 3 and r["fold_partial"],
        "vec 1, rp 2, ragged": lambda r: r["vec"] == 1 and r["rp"] >= 2 and r["ragged"],
        "vec 4, cs 4, rp 2, ragged": lambda r: r["vec"] == 4 and r["cs"] == 4 and r["rp"] >= 2 and r["ragged"],
        "vec 4, cs 64, rp 2, ragged": lambda r: r["vec"] == 4 and r["cs"] == 64 and r["rp"] >= 2 and r["ragged"],
        "vec 4 in half precision, nj 2": lambda r: r["vec"] == 4 and r["dt"] != "f32" and r["nj"] >= 2,
        "vec 8, nj 2, partial fold block": lambda r: r["vec"] == 8 and r["nj"] >= 2 and r["fold_partial"],
        "vec 8, rp 5, ragged": lambda r: r["vec"] == 8 and r["rp"] >= 5 and r["ragged"],
        "W = 1": lambda r: r["W"] == 1,
        "several tiles of cs 4 over a 3-pixel-wide image": lambda r: r["cs"] == 4 and r["W"] == 3 and r["ntile"] >= 2,
        "a last tile with pixels past the image": lambda r: (r["H"] * r["W"]) % r["ch"] != 0,
        "fewer channel groups than lanes": lambda r: r["ng"] < r["cs"],
        "fp16": lambda r: r["dt"] == "f16",
        "bf16": lambda r: r["dt"] == "bf16",
        "3-D mask": lambda r: r["mask3d"],
        "mask without grad": lambda r: r["kind"] != "none" and not r["mask_grad"],
        "no mask": lambda r: r["kind"] == "none",
        "raw-probability mask": lambda r: r["kind"] == "prob",
        "use = 0": lambda r: r["kind"] == "tiny",
        "B = 1": lambda r: r["B"] == 1,
        "B = 11": lambda r: r["B"] == 11 and r["C"] == 7,
        "taps wider than the channel axis": lambda r: r["k"] > r["C"],
        "C = 3 with k = 3": lambda r: r["C"] == 3 and r["k"] == 3,
    }
    missed = [b for b, hit in branches.items() if not any(hit(r) for r in rows)]
    assert not missed, missed
    assert {r["k"] for r in rows} == {1, 3, 5, 15}
    assert {"none", "tiny", "all_negative", "prob", "mixed", "sparse", "randn"} <= {r["kind"] for r in rows}
