"""CPU-side checks of the NCHW MaskECA levels: the channel limit that k_eca_bwd's LDS sets (api_eca.hip: kEcaNchwMaxC), refused by the size
queries, the forward and the backward alike, and the launch geometry of the rows tests/test_gpu_eca_nchw.py runs.  No kernel is launched
here: every call below must fail its argument checks before anything touches a device."""
import pytest

from abi_header import fake
from eca_nchw_rows import ECA_BWD_STATIC_LDS, KNOB_ROWS, LDS_PER_WORKGROUP, NCHW_ROWS, nchw_geo, nchw_max_c, row_case

LIMIT = nchw_max_c()


def _levels(_lib, lib, B, Cc, H, W, k, dtype):
    """One forward and one backward NCHW level on fake pointers; the capacities are those of a C the queries accept (they grow with C)."""
    P = _lib.EcaParams(fake(), fake(), k, 1, 1e-4, 1e-6)
    fl = (_lib.EcaFwdLevel * 1)()
    F = fl[0]
    F.x = F.mask = F.y = F.ctx = fake()
    F.p, F.B, F.C, F.H, F.W, F.dtype, F.flags = P, B, Cc, H, W, dtype, 0
    bl = (_lib.EcaBwdLevel * 1)()
    Bw = bl[0]
    for f in ("x", "mask", "gy", "ctx", "scratch", "gx", "gmask", "gw", "gbeta"):
        setattr(Bw, f, fake())
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = P, B, Cc, H, W, dtype, 0
    return fl, bl


def test_the_limit_is_what_k_eca_bwd_fits_in_lds():
    """vec 4 asks for the most (256 * vec combine floats beside the 3 floats per channel); the limit holds for every NCHW level."""
    assert LIMIT == 5117
    for vec in (1, 4):
        assert (3 * LIMIT + 256 * vec) * 4 + ECA_BWD_STATIC_LDS <= LDS_PER_WORKGROUP
    assert (3 * (LIMIT + 1) + 256 * 4) * 4 + ECA_BWD_STATIC_LDS > LDS_PER_WORKGROUP
    assert max(r[3] for r in NCHW_ROWS) == 5000 <= LIMIT                 # the widest row of the GPU table stays inside


@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (16, 16)], ids=["vec4_nv1", "vec1", "vec4"])
def test_a_level_at_the_limit_passes_and_one_channel_more_is_refused_everywhere(built_lib, hw):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    B, (H, W), k = 2, hw, 7
    queries = [lambda c: lib.mgacbam_eca_ctx_bytes(B, c, H, W), lambda c: lib.mgacbam_eca_scratch_bytes(B, c, H, W),
               lambda c: lib.mgacbam_eca_ctx_bytes_flags(B, c, H, W, 0), lambda c: lib.mgacbam_eca_scratch_bytes_flags(B, c, H, W, 0)]
    for q in queries:
        assert q(LIMIT) > q(LIMIT - 1) > 0
        assert q(LIMIT + 1) == 0 and q(65536) == 0
        msg = lib.mgacbam_last_error().decode()
        assert f"C <= {LIMIT}" in msg and "NCHW" in msg and "LDS" in msg, msg
    need_ctx, need_scr = queries[0](LIMIT), queries[1](LIMIT)
    for dtype in (_lib.F32, _lib.F16, _lib.BF16):
        # at the limit the level gets past the shape checks, as far as the capacity check after them
        fl, bl = _levels(_lib, lib, B, LIMIT, H, W, k, dtype)
        fl[0].ctx_bytes = need_ctx - 1
        assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_SIZE, lib.mgacbam_last_error()
        bl[0].ctx_bytes, bl[0].scratch_bytes = need_ctx, need_scr - 1
        assert lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_SIZE and b"scratch" in lib.mgacbam_last_error()
        # one channel more: E_SHAPE from both, whatever the buffers hold
        fl, bl = _levels(_lib, lib, B, LIMIT + 1, H, W, k, dtype)
        fl[0].ctx_bytes = bl[0].ctx_bytes = bl[0].scratch_bytes = 1 << 40
        assert lib.mgacbam_eca_forward(fl, 1, None) == _lib.E_SHAPE
        assert f"C <= {LIMIT}" in lib.mgacbam_last_error().decode()
        assert lib.mgacbam_eca_backward(bl, 1, None) == _lib.E_SHAPE
        assert f"C <= {LIMIT}" in lib.mgacbam_last_error().decode()
    # a channels-last level keeps its own, lower limit and its own message
    assert lib.mgacbam_eca_ctx_bytes_flags(B, LIMIT, H, W, _lib.LAYOUT_NHWC) == 0 and b"channels-last" in lib.mgacbam_last_error()


def test_a_refused_level_of_a_pyramid_stops_the_whole_call(built_lib):
    """Every level is checked before anything is launched: a good level in front of an over-wide one does not run."""
    import ctypes as C
    from mga_yolo_amd import _lib
    lib = _lib.load()
    good, _ = _levels(_lib, lib, 2, 64, 8, 8, 3, _lib.F32)
    good[0].ctx_bytes = lib.mgacbam_eca_ctx_bytes(2, 64, 8, 8)
    wide, _ = _levels(_lib, lib, 2, LIMIT + 1, 8, 8, 3, _lib.F32)
    two = (_lib.EcaFwdLevel * 2)()
    C.memmove(C.byref(two[0]), C.byref(good[0]), C.sizeof(_lib.EcaFwdLevel))
    C.memmove(C.byref(two[1]), C.byref(wide[0]), C.sizeof(_lib.EcaFwdLevel))
    assert lib.mgacbam_eca_forward(two, 2, None) == _lib.E_SHAPE and f"C <= {LIMIT}".encode() in lib.mgacbam_last_error()


def test_the_message_reaches_the_python_caller(built_lib):
    from mga_yolo_amd import _lib
    _lib.load()
    assert _lib.eca_ctx_bytes(1, LIMIT, 2, 2) > 0 and _lib.eca_scratch_bytes(1, LIMIT, 2, 2) > 0
    for ask in (_lib.eca_ctx_bytes, _lib.eca_scratch_bytes):
        with pytest.raises(RuntimeError, match=f"an NCHW level takes C <= {LIMIT}"):
            ask(1, LIMIT + 1, 2, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# coverage of tests/test_gpu_eca_nchw.py
# ---------------------------------------------------------------------------------------------------------------------------
def test_nchw_rows_have_the_geometry_their_comments_state():
    """Holds the geometry column of every row of NCHW_ROWS (the numbers its comment states) against eca_nchw_rows.nchw_geo, which restates
    host.cuh's vec_of, choose_tune (pool_tx, chan_tx) and group_cpt BY HAND: it follows host.cuh only as long as somebody keeps it in
    step, and a change of the tuning rules has to be made there too.  Then every branch the table is there for must still be reached by
    some row, so a tuning change that moves a row off its branch fails here, on the CPU, instead of thinning what the GPU rows cover."""
    rows = []
    for name, dt, B, Cc, H, W, k, kind, mask3d, mask_grad, tiny_thr, want in NCHW_ROWS:
        g = nchw_geo(B, Cc, H, W)
        assert want and {key: g[key] for key in want} == want, (name, g)
        assert g["lds"] + ECA_BWD_STATIC_LDS <= LDS_PER_WORKGROUP, name
        rows.append(dict(g, name=name, dt=dt, B=B, C=Cc, H=H, W=W, k=k, kind=kind, mask3d=mask3d, mask_grad=mask_grad, thr=tiny_thr))
    assert len({r["name"] for r in rows}) == len(rows) == 21
    f32 = lambda r: r["dt"] == "f32"
    half = lambda r: r["dt"] != "f32"
    branches = {
        "vec 1, ragged sweep, clamped channels": lambda r: r["vec"] == 1 and r["rem"] and r["crem"] and r["C"] > r["cpb"],
        "vec 4, TX 128 ragged": lambda r: r["vec"] == 4 and r["tx"] == 128 and r["rem"],
        "vec 4, TX 256 ragged": lambda r: f32(r) and r["vec"] == 4 and r["tx"] == 256 and r["rem"],
        "vec 1, TX 256 ragged": lambda r: r["vec"] == 1 and r["tx"] == 256 and r["rem"],
        "half precision, TX 256 ragged": lambda r: half(r) and r["tx"] == 256 and r["rem"],
        "last tile of one lane": lambda r: r["tiles"] > 1 and r["last"] == 1,
        "ctx 64 by the channels-per-row widening": lambda r: r["ctx"] == 64 and r["B"] * r["tiles"] < 768 and r["nv"] >= 64,
        "ctx 64 by the grid size": lambda r: r["ctx"] == 64 and r["B"] * r["tiles"] >= 768 and r["C"] >= 4 * r["ty"],
        "ctx 32": lambda r: r["ctx"] == 32,
        "ctx 16, ragged tiles": lambda r: r["ctx"] == 16 and r["last"] < 16,
        "ctx 1, TY 256": lambda r: r["ctx"] == 1 and r["ty"] == 256,
        "C < TY": lambda r: r["C"] < r["ty"],
        "TY < C < 2 TY": lambda r: r["ty"] < r["C"] < 2 * r["ty"],
        "C = 3 TY": lambda r: r["C"] == 3 * r["ty"],
        "inactive tile lanes": lambda r: r["last"] < r["ctx"],
        "cpt 2 by group_cpt, clamped channels": lambda r: r["cpt"] == 2 and r["tx"] < 256 and r["crem"],
        "cpt 2 at TX 256, C odd": lambda r: r["cpt"] == 2 and r["tx"] == 256 and r["C"] % 2,
        "8-byte half vectors": lambda r: half(r) and r["vec"] == 4,
        "scalar fp16": lambda r: r["dt"] == "f16" and r["vec"] == 1,
        "scalar bf16": lambda r: r["dt"] == "bf16" and r["vec"] == 1,
        "all 15 taps": lambda r: r["k"] == 15 and r["C"] >= 15,
        "k > C": lambda r: r["k"] > r["C"] > 1,
        "no mask": lambda r: r["kind"] == "none",
        "mask without grad": lambda r: r["kind"] != "none" and not r["mask_grad"],
        "3-D mask": lambda r: r["mask3d"],
        "raw-probability mask, fp32": lambda r: r["kind"] == "prob" and f32(r),
        "raw-probability mask, half": lambda r: r["kind"] == "prob" and half(r),
        "use = 0": lambda r: r["kind"] == "tiny" and r["thr"] > 0,
        "use = 1 with S < eps": lambda r: r["kind"] == "tiny" and r["thr"] == 0.0,
        "W = 1": lambda r: r["W"] == 1,
        "B = 1": lambda r: r["B"] == 1 and r["C"] > 1,
        "B = 11": lambda r: r["B"] % 8 == 3,
        "one element": lambda r: r["B"] * r["C"] * r["H"] * r["W"] == 1,
        "near the LDS limit": lambda r: r["lds"] > LDS_PER_WORKGROUP - 2048,
    }
    missed = [b for b, hit in branches.items() if not any(hit(r) for r in rows)]
    assert not missed, missed
    assert {r["k"] for r in rows} == {1, 3, 5, 7, 9, 15}
    assert {"none", "tiny", "all_negative", "prob", "mixed", "sparse", "randn"} <= {r["kind"] for r in rows}
    by = {r["name"]: r for r in rows}
    assert {by[n]["dt"] for n in KNOB_ROWS} == {"f32", "f16", "bf16"} and len(KNOB_ROWS) == 5


@pytest.mark.parametrize("name", ["v1_tx64_c130", "w1_c3", "k_gt_c_b11", "live0"])
def test_small_rows_sit_off_the_branch_thresholds(name):
    """row_case asserts on the host that no sample's S / N is within 1e-3 of tiny_thr and no S within 1e-3 of eps (and, for the
    tiny_thr = 0 row, that the fp64 autograd oracle and the hand-derived one agree); the small rows with use = 0 / live = 0 samples are
    checked here without a GPU."""
    c = row_case(name)
    assert c.y_o.dtype.is_floating_point and c.g_o["gx"].shape == c.x.shape
