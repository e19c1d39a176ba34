"""CPU-side checks of the NCHW mask-head levels and of what tests/test_gpu_head_nchw.py runs: the launch geometry of every row of
tests/head_nchw_rows.py, the hand restatement behind it against the library's size queries, the argument checks of an NCHW level that
tests/test_abi.py does not reach, and the element-wise metric itself -- the fp32 oracle passes its bars, five wrong results do not.  No
kernel is launched here: every call below must fail its argument checks before anything touches a device."""
import pytest
import torch

from abi_header import fake
from conftest import rel_err
from head_nchw_rows import (CASES, HEAD_NCHW_ROWS, HO, OUTPUTS, TOL, U_BAR, U_ORACLE32, head_geo, measure_oracle_u, oracle32, row_case)


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the rows have the geometry their comments state
# ---------------------------------------------------------------------------------------------------------------------------
def test_head_nchw_rows_have_the_geometry_their_comments_state():
    """Holds the geometry column of every row of HEAD_NCHW_ROWS against head_nchw_rows.head_geo, which restates api_head.hip's head_waves
    and head_tiling, head.cuh's head_out_shape and the K / M / share arithmetic of head_gemm_body, k_head_bwd_gw and k_head_bwd_gw2 BY
    HAND: it follows the sources only as long as somebody keeps it in step.  Then every branch the table is there for must still be
    reached by some row, so a tuning change that moves a row off its branch fails here, on the CPU."""
    rows = []
    for name, dts, B, Cc, hid, H, W, ev, want in HEAD_NCHW_ROWS:
        g = head_geo(B, Cc, hid, H, W)
        assert want and {k: g[k] for k in want} == want, (name, {k: g[k] for k in want})
        nbytes = 4 * B * max(Cc, hid) * H * W
        assert nbytes <= 6 << 20, (name, nbytes)                                 # a few MB at the most
        rows.append(dict(g, name=name, dts=dts, B=B, C=Cc, hid=hid, H=H, W=W, HW=H * W, ev=ev))
    assert len({r["name"] for r in rows}) == len(rows)
    half = lambda r: any(d != "f32" for d in r["dts"])
    branches = {
        "forward K wave with nothing to do": lambda r: r["fw_kw"] == 4 and r["fw_kempty"] == 1 and (r["fw_ksteps"], r["fw_kper"]) == (36, 12),
        "forward kw 2, even split": lambda r: r["fw_kw"] == 2 and r["fw_ksteps"] == 2 * r["fw_kper"],
        "forward kw 2, uneven split, vec 1": lambda r: r["fw_kw"] == 2 and r["vec"] == 1 and r["fw_ksteps"] < 2 * r["fw_kper"],
        "wperm with the kk0 < K guard, vec 1": lambda r: r["fw_w"] == "guard" and r["vec"] == 1,
        "wperm with the kk0 < K guard, vec 4": lambda r: r["fw_w"] == "guard" and r["vec"] == 4 and r["C"] > 16,
        "wperm, whole groups": lambda r: r["fw_w"] == "perm",
        "gather form of the weights": lambda r: r["fw_w"] == "gather" and r["C"] > 4,
        "gather form, half precision": lambda r: r["fw_w"] == "gather" and half(r),
        "forward mw 3 -> 4 at MTW 2": lambda r: r["fw_mtw"] == 2 and r["fw_mw3"],
        "forward mw 3 -> 4 at MTW 4": lambda r: r["fw_mtw"] == 4 and r["fw_mw3"],
        "forward, second M block": lambda r: r["fw_mblk"] == 2,
        "forward, one full M block at MTW 4": lambda r: r["fw_mtw"] == 4 and r["hidp"] == 256 and r["fw_mblk"] == 1,
        "forward pw 2": lambda r: r["fw_pw"] == 2,
        "gx mw 3 -> 4": lambda r: r["gx_mw3"],
        "gx, second M block": lambda r: r["gx_mblk"] == 2,
        "gx, three M blocks": lambda r: r["gx_mblk"] == 3,
        "gx kw 4, ragged K": lambda r: r["gx_kw"] == 4 and r["hid"] % 4,
        "gx kw 4 in half precision (half_gx grouping, one K wave empty)": lambda r: r["gx_kw"] == 4 and half(r) and r["gx_kempty_half"] == 1,
        "gx kw 2": lambda r: r["gx_kw"] == 2,
        "padded M rows (hidden % 16 != 0) beyond 128": lambda r: r["hid"] > 128 and r["hid"] % 16,
        "k_head_bwd_gw shares that own no pixels": lambda r: not r["gw2"] and r["gw_empty"] > 0,
        "k_head_bwd_gw every share busy": lambda r: not r["gw2"] and r["gw_empty"] == 0,
        "k_head_bwd_gw at vec 4 in several passes": lambda r: not r["gw2"] and r["vec"] == 4 and r["gw_passes"] > 1,
        "k_head_bwd_gw2 uneven shares": lambda r: r["gw2"] and r["gw_uneven"] and r["nshare"] > 1,
        "k_head_bwd_gw2 ragged last chunk": lambda r: r["gw2"] and r["gw_last"] == 16 and r["nshare"] > 1,
        "k_head_bwd_gw2 ncb > 1, 4 channels in the last block": lambda r: r["gw2"] and r["ncb"] == 3 and r["clast"] == 4,
        "k_head_bwd_gw ncb > 1, 8 channels in the last block": lambda r: r["ncb"] == 3 and r["clast"] == 8,
        "k_head_bwd_gw2 at hidp 64": lambda r: r["gw2"] and r["hidp"] == 64 and r["ncb"] == 2,
        "k_head_bwd_gw2 many shares": lambda r: r["gw2"] and r["nshare"] >= 25,
        "act_ppt 2 at H*W = 512": lambda r: r["HW"] == 512 and r["act_ppt"] == 2,
        "act_ppt 1 just below": lambda r: 504 <= r["HW"] < 512 and r["act_ppt"] == 1 and r["nwg1"] == 2 * r["B"],
        "act_ppt 4 at H*W = 2048": lambda r: r["HW"] == 2048 and r["act_ppt"] == 4,
        "act_ppt 2, vec 1, ragged run": lambda r: r["act_ppt"] == 2 and r["vec"] == 1,
        "k_head_out per 2, full last run": lambda r: r["out_per"] == 2 and r["out_last"] == r["out_px"],
        "k_head_out per > 1, short last run": lambda r: r["out_per"] > 1 and r["out_last"] < r["out_px"],
        "k_head_out per 3": lambda r: r["out_per"] == 3,
        "k_head_out ppt escalated 1 -> 4 (widest row)": lambda r: r["W"] == 500 and r["hid"] > 32 and r["out_ppt"] == 4 and r["out_per"] == 32,
        "k_head_out ppt escalated 1 -> 2": lambda r: r["hid"] > 32 and r["out_ppt"] == 2,
        "k_head_out two chunks of constants": lambda r: r["out_chunks"] == 2,
        "k_head_out three chunks of constants": lambda r: r["out_chunks"] == 3,
        "k_head_stats four partial rows in flight": lambda r: r["nwg"] >= 4 * 256,
        "k_head_bwd_fin eight partial rows in flight": lambda r: r["nwg1"] >= 8 * 16,
        "last forward tile of 5 pixels, vec 1": lambda r: r["vec"] == 1 and r["last_px"] == 5 and r["tps"] > 1,
        "last forward tile of one pixel": lambda r: r["last_px"] == 1 and r["tps"] > 1,
        "C = hidden = 1": lambda r: r["C"] == 1 and r["hid"] == 1,
    }
    missed = [b for b, hit in branches.items() if not any(hit(r) for r in rows)]
    assert not missed, missed
    assert {r["hid"] for r in rows if r["ev"]} == {8, 24, 80, 130, 384}                      # the eval-mode rows
    assert all(r["ev"] for r in rows if r["hid"] in (8, 24, 80, 130, 384))
    assert {d for r in rows for d in r["dts"]} == {"f32", "f16", "bf16"} and all(r["dts"][0] == "f32" for r in rows)
    assert {g for _, _, tr, g in CASES if tr} == {"flat"} and {g for _, _, tr, g in CASES if not tr} == {"flat", "env"}


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the restatement against the built library
# ---------------------------------------------------------------------------------------------------------------------------
def test_restated_layouts_equal_the_library_s_size_queries(built_lib):
    """mgahead_ctx_bytes is a function of (B, hidden, H*W, hidp, nwg) and mgahead_bwd_scratch_bytes of (B, hidden, H*W, hidp, nwg1, ncb,
    nshare) (api_head.hip: head_ctx_layout, head_scratch_layout), so equal byte counts pin head_geo's vec, forward pw (through
    tile_px -> nwg), act_ppt, ncb, gw2 and nshare to the library's.  What no size depends on -- kw and the K-step split, mw and the M blocks,
    the gx tiling, k_head_out's ppt / runs -- stays a hand restatement of head_tiling and head_gemm_body."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    shapes = [r[2:7] for r in HEAD_NCHW_ROWS]
    for hid in (16, 64, 128, 129):
        for Cc in (64, 65, 128):
            for H, W in ((4, 127), (16, 32), (7, 292), (32, 64)):                             # H*W = 508, 512, 2044, 2048
                for B in (1, 3):
                    shapes.append((B, Cc, hid, H, W))
    for B, Cc, hid, H, W in shapes:
        g = head_geo(B, Cc, hid, H, W)
        assert lib.mgahead_ctx_bytes(B, Cc, H, W, hid) == g["ctx_bytes"], (B, Cc, hid, H, W, g)
        assert lib.mgahead_bwd_scratch_bytes(B, Cc, H, W, hid) == g["scratch_bytes"], (B, Cc, hid, H, W, g)
        assert lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, 0) == g["ctx_bytes"]


# ---------------------------------------------------------------------------------------------------------------------------
# (c) argument validation of an NCHW level
# ---------------------------------------------------------------------------------------------------------------------------
BWD_PTRS = ("x", "g_logits", "ctx", "scratch", "gx", "gw1", "gbn_weight", "gbn_bias", "gwh", "gbh")


def _levels(_lib, lib, B, Cc, hid, H, W, dtype, eps=1e-3, momentum=0.03):
    HP = _lib.HeadParams(*([fake()] * 8), hid, eps, momentum, 1)
    fl = (_lib.HeadFwdLevel * 1)()
    F = fl[0]
    F.x = F.logits = F.ctx = fake()
    F.p, F.B, F.C, F.H, F.W, F.dtype, F.flags = HP, B, Cc, H, W, dtype, 0
    F.ctx_bytes = lib.mgahead_ctx_bytes(B, Cc, H, W, hid)
    bl = (_lib.HeadBwdLevel * 1)()
    Bw = bl[0]
    for f in BWD_PTRS:
        setattr(Bw, f, fake())
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = HP, B, Cc, H, W, dtype, 0
    Bw.ctx_bytes, Bw.scratch_bytes = F.ctx_bytes, lib.mgahead_bwd_scratch_bytes(B, Cc, H, W, hid)
    return fl, bl


@pytest.mark.parametrize("hw,dt,need", [((8, 8), "F32", 16), ((8, 8), "F16", 8), ((8, 8), "BF16", 8), ((7, 5), "F32", 4), ((7, 5), "F16", 2),
                                        ((7, 5), "BF16", 2)])
def test_misaligned_features_are_refused(built_lib, hw, dt, need):
    """x (and gx) of an NCHW level must be aligned to vec elements: 16 / 8 bytes when H*W % 4 == 0, else one element."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    (H, W), dtype = hw, getattr(_lib, dt)
    for off in {need // 2, 1}:
        fl, bl = _levels(_lib, lib, 2, 20, 8, H, W, dtype)
        fl[0].x = fake() + off
        assert lib.mgahead_forward(fl, 1, None) == _lib.E_ALIGN
        assert f"x must be {need}-byte aligned".encode() in lib.mgacbam_last_error(), lib.mgacbam_last_error()
        for f in ("x", "gx"):
            fl, bl = _levels(_lib, lib, 2, 20, 8, H, W, dtype)
            setattr(bl[0], f, fake() + off)
            assert lib.mgahead_backward(bl, 1, None) == _lib.E_ALIGN, f
            assert f"x/gx must be {need}-byte aligned".encode() in lib.mgacbam_last_error(), lib.mgacbam_last_error()


def test_misaligned_work_buffers_are_refused(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for off in (4, 8):
        fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32)
        fl[0].ctx = fake() + off
        assert lib.mgahead_forward(fl, 1, None) == _lib.E_ALIGN and b"ctx 16-byte" in lib.mgacbam_last_error()
        for f in ("ctx", "scratch"):
            fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32)
            setattr(bl[0], f, fake() + off)
            assert lib.mgahead_backward(bl, 1, None) == _lib.E_ALIGN and b"ctx/scratch 16-byte" in lib.mgacbam_last_error(), f


@pytest.mark.parametrize("eps,momentum", [(0.0, 0.1), (-1e-5, 0.1), (float("nan"), 0.1), (1e-5, -0.01), (1e-5, 1.01), (1e-5, float("nan"))])
def test_bad_eps_and_momentum_are_a_shape_error(built_lib, eps, momentum):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32, eps, momentum)
    assert lib.mgahead_forward(fl, 1, None) == _lib.E_SHAPE and b"eps=" in lib.mgacbam_last_error()
    assert lib.mgahead_backward(bl, 1, None) == _lib.E_SHAPE and b"momentum=" in lib.mgacbam_last_error()


def test_every_null_pointer_of_a_level_is_named(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for f in BWD_PTRS:
        fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32)
        setattr(bl[0], f, None)
        assert lib.mgahead_backward(bl, 1, None) == _lib.E_NULL, f
        assert b"mask head backward" in lib.mgacbam_last_error()
    for f in ("x", "logits", "ctx"):
        fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32)
        setattr(fl[0], f, None)
        assert lib.mgahead_forward(fl, 1, None) == _lib.E_NULL, f
    for f in ("w1", "bn_weight", "bn_bias", "running_mean", "running_var", "wh", "bh"):          # (num_batches_tracked may be NULL)
        fl, bl = _levels(_lib, lib, 2, 20, 8, 7, 5, _lib.F32)
        setattr(fl[0].p, f, None)
        setattr(bl[0].p, f, None)
        assert lib.mgahead_forward(fl, 1, None) == _lib.E_NULL and b"parameter" in lib.mgacbam_last_error(), f
        assert lib.mgahead_backward(bl, 1, None) == _lib.E_NULL and b"parameter" in lib.mgacbam_last_error(), f


# ---------------------------------------------------------------------------------------------------------------------------
# (d) the metric finds what it is for
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_bars_are_eight_times_the_oracle_s_own_error():
    silu = ("logits", "gx", "gw1", "ggamma", "gbeta", "gwh")
    assert set(U_BAR) == set(U_ORACLE32) == set(OUTPUTS)
    for k in OUTPUTS:
        assert U_BAR[k] == 8 * U_ORACLE32[k] + (4e-6 if k in silu else 0.0)
        assert U_BAR[k] < 5e-5                                                  # every bar stays below half the tensor-scale one


def test_the_table_of_the_oracle_s_own_error_is_what_a_measurement_gives():
    """U_ORACLE32 (and with it every fp32 bar) against measure_oracle_u() on this host, within a factor of 4 either way: the fp32 sums of
    torch's BLAS depend on the host's blocking, but a table gone stale after a change of rows, inputs or oracle shows here."""
    got = measure_oracle_u()
    for k, (u, cid) in got.items():
        print(f"{k} {u:.2e} ({cid}) table {U_ORACLE32[k]:.1e}")
        assert U_ORACLE32[k] / 4 <= u <= 4 * U_ORACLE32[k], (k, u, cid)


def mutants(c, o32):
    """Five wrong results, each wrong at ONE place, as -> {name: (output, value)}: the fp32 oracle's output plus the difference the
    mistake makes, worked out in fp64 from the fp64 oracle's intermediates."""
    B, Cc, hid, H, W = c.B, c.C, c.hid, c.H, c.W
    HW = H * W
    geo = head_geo(B, Cc, hid, H, W)
    p, x, gl = HO._p64(c.p), c.x.double().view(B, Cc, HW), c.gl.double()
    g_z = c.g_z.view(B, hid, HW)
    out = {}
    # z misses the last channel's term at the last real pixel of the first forward tile; the logits that follow from it
    px = min(geo["tile_px"], HW) - 1
    z = c.c64.z.clone().view(B, hid, HW)
    z[0, :, px] -= p.w1[:, Cc - 1] * x[0, Cc - 1, px]
    lo = HO.forward(c.x, c.p, c.training, double=True, z=z.view(B, hid, H, W))[0]
    out["z without its last channel at one pixel"] = ("logits", o32["logits"].double() + (lo - c.want["logits"]))
    # the pixel at the end of the first image row of the last sample takes its right-hand tap from the pixel the index wraps to
    lo = o32["logits"].double().clone()
    lo[B - 1, 0, 0, W - 1] += (p.wh[0, :, 1, 2] * c.c64.s[B - 1, :, 1, 0]).sum()
    out["logits with the tap that wraps the row end"] = ("logits", lo)
    # gx misses one hidden channel's g_z at one pixel (the last but one of the last sample)
    gx = o32["gx"].double().clone().view(B, Cc, HW)
    gx[B - 1, :, HW - 2] -= p.w1[hid // 2, :] * g_z[B - 1, hid // 2, HW - 2]
    out["gx without one hidden channel at one pixel"] = ("gx", gx.view(B, Cc, H, W))
    # dW1's last row (the last hidden channel) misses the last 64-pixel chunk of the last sample
    p0 = (-(-HW // 64) - 1) * 64
    gw1 = o32["gw1"].double().clone()
    gw1[hid - 1] -= torch.einsum("p,cp->c", g_z[B - 1, hid - 1, p0:], x[B - 1, :, p0:])
    out["gw1 row without the last pixel chunk"] = ("gw1", gw1)
    # dW_h's tap (0,1) of the last hidden channel paired with g one image row further down: what tap (1,1) pairs
    gwh = o32["gwh"].double().clone()
    sp = torch.nn.functional.pad(c.c64.s, (1, 1, 1, 1))
    gwh[0, hid - 1, 0, 1] = torch.einsum("bhw,bhw->", torch.roll(gl, 1, dims=2)[:, 0], sp[:, hid - 1, 0:H, 1:1 + W])
    out["gwh tap with g shifted by a row"] = ("gwh", gwh)
    return out


def _oracle32_one_thread(c):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return oracle32(c.x, c.gl, c.p, c.training)
    finally:
        torch.set_num_threads(threads)


@pytest.mark.parametrize("training,gkind", [(False, "env"), (False, "flat"), (True, "flat")], ids=["eval-env", "eval-flat", "train-flat"])
@pytest.mark.parametrize("name", ["v1_guard", "ksplit_c132", "v1_w333"])          # a vec 1 row, a K-split row, a wide row
def test_the_metric_passes_the_fp32_oracle_and_finds_five_single_place_mistakes(name, training, gkind):
    """The fp32 oracle's own outputs pass every bar of tests/test_gpu_head_nchw.py, and five results that are wrong at one place each
    exceed the element-wise bar on the output they touch, in every mode.  That at least three of the five PASS rel_err < 1e-4, the only
    bar this path had, holds in EVAL MODE UNDER THE ENVELOPE ONLY, and is asserted there: a missing term of gx at a pixel where
    dL/dlogits is small, a row of dW1 and a tap of dW_h of a nearly dead hidden channel, each an element that is small beside its
    tensor's largest.  Without the envelope, and in training mode (every g_z carries the batch terms gbeta / n and zhat ggamma / n), gx
    has no such elements and two of the five remain hidden from rel_err; no sparser single-place mistake of gx or logits was found."""
    c = row_case(name, "f32", training, gkind)
    o32 = _oracle32_one_thread(c)
    for k in OUTPUTS:
        u = HO.elem_u(o32[k], c.want[k], c.mag[k])
        assert rel_err(o32[k], c.want[k]) < TOL["f32"] and u < U_BAR[k], (k, u)
    hidden_from_rel_err = []
    for what, (k, val) in mutants(c, o32).items():
        u, old = HO.elem_u(val, c.want[k], c.mag[k]), rel_err(val, c.want[k])
        print(f"{name} {'train' if training else 'eval'} {gkind} {what}: u {u:.2e} (bar {U_BAR[k]:.1e}), rel_err {old:.2e}")
        assert u > U_BAR[k], (what, u)
        if old < TOL["f32"]:
            hidden_from_rel_err.append(what)
    assert "gwh tap with g shifted by a row" in hidden_from_rel_err and "gw1 row without the last pixel chunk" in hidden_from_rel_err
    if gkind == "env":
        assert len(hidden_from_rel_err) >= 3 and "gx without one hidden channel at one pixel" in hidden_from_rel_err


@pytest.mark.parametrize("name,training,drop", [("hw2048", False, 64), ("hw2048", True, 4), ("hw512", False, 4), ("hw508", True, 1),
                                                ("gw2_ragged", True, 16), ("v1_w333", True, 2), ("out2_h40", True, 16)])
def test_the_tail_of_the_last_run_carries_its_weight_in_every_reduction(name, training, drop):
    """Under the uniform dL/dlogits every case runs with, the four reductions of k_head_bwd_act / k_head_bwd_fin (ggamma, gbeta, dW_h,
    db_h) and dW1 without the last `drop` pixels of the last sample -- the end of the last run at each act_ppt, the ragged last 64-pixel
    chunk -- exceed their bars on every one of the five outputs.  (Under the envelope alone they would not: those pixels carry 1e-5 of
    the weight there.)"""
    c = row_case(name, "f32", training, "flat")
    B, hid, HW = c.B, c.hid, c.H * c.W
    p = HO._p64(c.p)
    g, s, zhat = c.gl.double(), c.c64.s, c.c64.zhat
    sig = torch.sigmoid(c.c64.a)
    ga_all = torch.nn.functional.conv_transpose2d(g, p.wh, padding=1) * (sig * (1 + c.c64.a * (1 - sig)))
    gp = torch.nn.functional.pad(g, (1, 1, 1, 1))

    def sums(keep):
        """The five reductions with each pixel's own contribution weighted by keep (dW_h is summed at the pixel of s: k_head_bwd_act)."""
        g_a, sk = ga_all * keep, s * keep
        gwh = torch.zeros_like(p.wh)
        for u in range(3):
            for v in range(3):                                                  # sum_p s[p] g[p - (u-1, v-1)]
                gwh[0, :, u, v] = torch.einsum("bhw,bjhw->j", gp[:, 0, 2 - u:2 - u + c.H, 2 - v:2 - v + c.W], sk)
        return dict(ggamma=(g_a * zhat).sum(dim=(0, 2, 3)), gbeta=g_a.sum(dim=(0, 2, 3)), gwh=gwh, gbh=(g * keep).sum(dim=(0, 2, 3)),
                    gw1=torch.einsum("bjhw,bchw->jc", c.g_z * keep, c.x.double()))

    keep = torch.ones(B, 1, c.H, c.W, dtype=torch.float64)
    for k, val in sums(keep).items():                                           # nothing dropped: the oracle's own results
        assert HO.elem_u(val, c.want[k], c.mag[k]) < 1e-12, k
    keep.view(B, HW)[B - 1, HW - drop:] = 0
    mutant = sums(keep)
    for k, val in mutant.items():
        u = HO.elem_u(val, c.want[k], c.mag[k])
        print(f"{name} {'train' if training else 'eval'} last {drop} px dropped: {k} u {u:.2e} (bar {U_BAR[k]:.1e})")
        assert u > U_BAR[k], (k, u)
