"""CPU-side checks of what tests/test_gpu_cbam_nchw.py covers: the hand restatement of the NCHW MaskCBAM launch rules
(cbam_nchw_rows.cbam_nchw_geo) against the library's own size queries, every row of NCHW_ROWS against the restatement, every launch form the
table is there for against the rows, and the rows' host-side guards.  No kernel is launched here."""
import pytest
import torch

from cbam_nchw_rows import (ENV_ROWS, KNOB_ROWS, MAX_TIE_CHANNELS, MAX_TIE_PIXELS, NCHW_ROWS, ONE_MIB, ROW_IDS, cbam_nchw_geo, ctx_fields,
                            row_case, scratch_total, sync_len)

# shapes beside the rows' own: every pool_tx / chan_tx / strip count / wsa_th regime, the 1 MiB rule from both sides, the workload's levels
SWEEP_B = (1, 2, 3, 8, 9, 32)
SWEEP_C = (1, 3, 7, 16, 40, 64, 130, 256, 512, 2052, 4100)
SWEEP_HW = ((1, 1), (2, 2), (4, 4), (9, 7), (6, 6), (16, 16), (23, 17), (20, 20), (28, 1), (40, 40), (64, 64), (63, 64), (8, 260), (8, 400),
            (6, 150), (80, 80), (30, 31), (3, 129), (100, 100))
SWEEP_K = (1, 3, 7, 15)
SWEEP_HIDDEN = (1, 4, 5, 8, 16, 17, 32)


def _shapes():
    for r in NCHW_ROWS:
        yield r[2:8]
    for B in SWEEP_B:
        for C in SWEEP_C:
            for H, W in SWEEP_HW:
                if B * C * H * W > 3e7:
                    continue
                for k in SWEEP_K:
                    for hid in SWEEP_HIDDEN:
                        yield B, C, H, W, k, hid


def _hold_against_library(lib, **knobs):
    n = 0
    for B, C, H, W, k, hid in _shapes():
        g = cbam_nchw_geo(B, C, H, W, k, hid, **knobs)
        assert lib.mgacbam_bwd_scratch_bytes(B, C, H, W, hid, k) == scratch_total(B, C, H, W, hid, k, g), (B, C, H, W, k, hid, knobs, g)
        want = ctx_fields(B, C, H, W, hid)
        assert lib.mgacbam_ctx_bytes(B, C, H, W, hid) == want["total"], (B, C, H, W, hid)
        n += 1
    return n


def test_the_restatement_gives_the_librarys_scratch_and_ctx_sizes(built_lib):
    """scratch_layout's size follows vec and chan_tx (the tile partials), conv_twq and wsa_th (the dWsa tile partials), pool_tx (the hidden
    partials) and wide_proj_shape (the MFMA planes: hidden, vec, chan_tx, the 1 MiB rule); ctx_layout's follows nflag.  So a retune of any of
    them in host.cuh fails here unless cbam_nchw_rows.py is retuned with it -- and then the rows' geometry columns fail below."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    assert _hold_against_library(lib) > 10000
    for r in NCHW_ROWS:                                              # every field offset and the Python description of the hand-off region
        B, C, H, W, k, hid = r[2:8]
        assert _lib.ctx_layout(B, C, H, W, hid) == {n: v for n, v in ctx_fields(B, C, H, W, hid).items()}, r[0]
        assert _lib.sync_len(B, C, H, W) == sync_len(B, C, H, W), r[0]


@pytest.mark.parametrize("env", [dict(MGACBAM_POOL_TX="1", MGACBAM_CHAN_TX="1"), dict(MGACBAM_POOL_TX="16", MGACBAM_CHAN_TX="16"),
                                 dict(MGACBAM_POOL_TX="64", MGACBAM_CHAN_TX="64"), dict(MGACBAM_POOL_TX="128", MGACBAM_CHAN_TX="32"),
                                 dict(MGACBAM_POOL_TX="256", MGACBAM_CHAN_TX="8")], ids=["1_1", "16_16", "64_64", "128_32", "256_8"])
def test_the_restatement_follows_the_forced_geometries(built_lib, env, monkeypatch):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_env()
    try:
        _hold_against_library(lib, pool_tx=int(env["MGACBAM_POOL_TX"]), chan_tx=int(env["MGACBAM_CHAN_TX"]))
    finally:
        monkeypatch.undo()
        _lib.reload_env()


def _rows():
    rows = []
    for name, dt, B, C, H, W, k, hid, kind, mask3d, mask_grad, thr, want in NCHW_ROWS:
        gmask = kind != "none" and mask_grad
        g = cbam_nchw_geo(B, C, H, W, k, hid, dt, gmask)
        rows.append(dict(g, name=name, dt=dt, B=B, C=C, H=H, W=W, k=k, hid=hid, kind=kind, mask3d=mask3d, mask_grad=mask_grad, gmask=gmask, thr=thr,
                         want=want, env={}))
    return rows


def test_rows_have_the_geometry_their_comments_state():
    for r in _rows():
        assert r["want"] and {key: r[key] for key in r["want"]} == r["want"], (r["name"], {key: r[key] for key in r["want"]})
    assert len(set(ROW_IDS)) == len(NCHW_ROWS) == 32
    assert max(r[2] * r[3] * r[4] * r[5] * 4 for r in NCHW_ROWS if r[0] not in ("cpt2_tx256", "cpt2_c770_k5")) <= 10 << 20   # the size budget
    assert max(r[2] * r[3] * r[4] * r[5] * 4 for r in NCHW_ROWS) <= 56 << 20


def test_every_launch_form_is_reached_by_some_row():
    """Every branch the table is there for must be reached by some row, so a tuning change that moves a row off its branch fails here, on
    the CPU, instead of thinning what the GPU rows cover.  A branch that loses its row gets another shape, never a weaker predicate."""
    rows = _rows()
    for name, env in ENV_ROWS.items():                             # the rows that run again under a knob, with the geometry it gives them
        r0 = next(r for r in rows if r["name"] == name)
        g = cbam_nchw_geo(r0["B"], r0["C"], r0["H"], r0["W"], r0["k"], r0["hid"], r0["dt"], r0["gmask"],
                          gate_narrow=env.get("MGACBAM_GATE_NARROW") == "1", bwd_merge=env.get("MGACBAM_BWD_MERGE", "1") != "0")
        rows.append(dict(r0, **g, env=env))
    f32 = lambda r: r["dt"] == "f32"
    half = lambda r: r["dt"] != "f32"
    plain = lambda r: not r["env"]
    gated = lambda r: r["gate"]
    branches = {
        # lane width
        "vec 1, fp32": lambda r: f32(r) and r["vec"] == 1,
        "vec 4, fp32": lambda r: f32(r) and r["vec"] == 4,
        "vec 4, fp16": lambda r: r["dt"] == "f16" and r["vec"] == 4,
        "vec 1, fp16": lambda r: r["dt"] == "f16" and r["vec"] == 1,
        "vec 4, bf16": lambda r: r["dt"] == "bf16" and r["vec"] == 4,
        "vec 1, bf16": lambda r: r["dt"] == "bf16" and r["vec"] == 1,
        "gvec 8, fp16": lambda r: r["dt"] == "f16" and r["gvec"] == 8 and gated(r),
        "gvec 8, bf16": lambda r: r["dt"] == "bf16" and r["gvec"] == 8 and gated(r),
        "H*W % 8 = 4 in half precision: gvec 4": lambda r: half(r) and r["H"] * r["W"] % 8 == 4 and r["gvec"] == 4 and gated(r),
        # sweep kernels
        "pool_tx 1": lambda r: r["tx"] == 1,
        "pool_tx 2..32": lambda r: 2 <= r["tx"] <= 32,
        "pool_tx 64": lambda r: r["tx"] == 64,
        "pool_tx 128": lambda r: r["tx"] == 128,
        "pool_tx 256": lambda r: r["tx"] == 256,
        "ragged last sweep": lambda r: r["rem"] != 0 and r["nv"] > r["tx"],
        "ragged last sweep through the LDS row reduction": lambda r: r["tx"] > 64 and r["rem"] != 0,
        "clamped channels in the last workgroup": lambda r: r["crem_f"] != 0 and r["C"] > r["cpb_f"],
        "B not a multiple of 8": lambda r: r["B"] > 1 and r["B"] % 8 != 0,
        "B = 1": lambda r: r["B"] == 1,
        "cpt 2 by the rule, forward and backward, tx 256": lambda r: r["cpt_f"] == 2 and r["cpt_b"] == 2 and r["tx"] == 256 and r["C"] % 2,
        "cpt 2 by the rule, tx < 256, clamped channels": lambda r: r["cpt_f"] == 2 and r["cpt_b"] == 2 and r["tx"] < 256 and r["crem_b"],
        # chan_tx
        "ctx 64 by the channels-per-row widening": lambda r: r["ctx"] == 64 and r["B"] * r["tiles"] < 768 and r["nv"] >= 64,
        "ctx 32": lambda r: r["ctx"] == 32,
        "ctx 16": lambda r: r["ctx"] == 16 and r["nv"] >= 16,
        "ctx below 16": lambda r: r["ctx"] < 16 and r["nv"] < 16,
        "last tile of one lane": lambda r: r["tiles"] > 1 and r["last"] == 1,
        "last tile partly active": lambda r: r["tiles"] > 1 and 1 < r["last"] < r["ctx"],
        "C < TY: both prefetched slices clamped": lambda r: r["C"] < r["ty"],
        "TY < C < 2 TY": lambda r: r["ty"] < r["C"] < 2 * r["ty"],
        # k_gate eligible
        "k_gate, one tile per sample": lambda r: gated(r) and r["gtiles"] == 1,
        "k_gate, several tiles, span >= 3": lambda r: gated(r) and r["gtiles"] > 1 and r["span"] >= 3,
        "k_gate, a tile spans several image rows": lambda r: gated(r) and r["gtiles"] > 1 and r["gtp"] >= 2 * r["W"],
        "k_gate, a tile is exactly one image row": lambda r: gated(r) and r["gtiles"] > 1 and r["gtp"] == r["W"],
        "k_gate, last tile partial": lambda r: gated(r) and r["gtiles"] > 1 and (r["H"] * r["W"]) % r["gtp"] != 0,
        "gate_tx 256": lambda r: gated(r) and r["gtx"] == 256,
        "gate_tx 64": lambda r: gated(r) and r["gtx"] == 64,
        "gate_tx 16": lambda r: gated(r) and r["gtx"] == 16,
        "gate_tx 8": lambda r: gated(r) and r["gtx"] == 8,
        "k_gate, k = 7": lambda r: gated(r) and r["k"] == 7,
        "k_gate, generic k": lambda r: gated(r) and r["k"] != 7,
        "k_gate narrower than a row (MGACBAM_GATE_NARROW)": lambda r: gated(r) and not r["tp_w"] and r["env"],
        # k_gate refused, each reason alone
        "refused: TP < W alone": lambda r: plain(r) and not r["gate"] and r["gty"] <= 256 and not r["tp_w"] and r["tp_sync"] and r["lds_ok"],
        "refused: the LDS bound alone": lambda r: not r["gate"] and r["gty"] <= 256 and r["tp_w"] and r["tp_sync"] and not r["lds_ok"],
        "refused: TP < kSyncPx alone": lambda r: not r["gate"] and r["gty"] <= 256 and r["tp_w"] and not r["tp_sync"] and r["lds_ok"],
        "refused: gty > 256": lambda r: not r["gate"] and r["gty"] > 256 and r["C"] > 4096,
        # MLP
        "MLP streamed": lambda r: r["stream"],
        "MLP staged: C % 4 != 0 alone": lambda r: r["C"] % 4 != 0 and r["hid"] % 4 == 0 and r["C"] <= 2048,
        "MLP staged: hidden % 4 != 0 alone": lambda r: r["C"] % 4 == 0 and r["hid"] % 4 != 0 and r["C"] <= 2048,
        "MLP staged: C > 2048 alone": lambda r: r["C"] % 4 == 0 and r["hid"] % 4 == 0 and r["C"] > 2048 and not r["stream"],
        "split_mlp inside k_gate": lambda r: r["split_mlp"] and gated(r),
        "split_mlp as a launch": lambda r: r["split_mlp"] and not r["gate"],
        "hidden = 1": lambda r: r["hid"] == 1,
        "hidden = C": lambda r: r["hid"] == r["C"] and r["C"] > 1,
        # k_pool forms ca
        "pool_ca, fp32, exactly 1 MiB, B = 1": lambda r: r["pool_ca"] and f32(r) and r["x_bytes"] == ONE_MIB and r["B"] == 1,
        "pool_ca, fp32, exactly 1 MiB, B = 9": lambda r: r["pool_ca"] and f32(r) and r["x_bytes"] == ONE_MIB and r["B"] == 9,
        "pool_ca, fp16, 2-byte elements": lambda r: r["pool_ca"] and r["dt"] == "f16" and r["x_bytes"] == r["C"] * r["H"] * r["W"] * 2,
        "pool_ca, bf16, 2-byte elements": lambda r: r["pool_ca"] and r["dt"] == "bf16" and r["x_bytes"] == r["C"] * r["H"] * r["W"] * 2,
        "not formed just below 1 MiB": lambda r: (not r["pool_ca"] and r["stream"] and not r["split_mlp"] and gated(r)
                                                   and ONE_MIB - 32768 <= r["x_bytes"] < ONE_MIB),
        # convolution
        "W = 1": lambda r: r["W"] == 1,
        "two column strips, the last narrower": lambda r: r["strips"] == 2 and r["last_strip"] < r["tw"],
        "three or more column strips, the last narrower": lambda r: r["strips"] >= 3 and r["last_strip"] < r["tw"],
        "conv_th limited by its cap": lambda r: r["th_by"] == "cap" and r["conv_tiles"] > r["strips"],
        "conv_th limited by H": lambda r: r["th_by"] == "H",
        "wsa_th < conv_th, several dWsa tiles": lambda r: r["wth"] < r["th"] and r["wsa_tiles"] > r["strips"],
        # backward form
        "merged": lambda r: r["merge"],
        "folded, not merged: k != 7": lambda r: r["fold"] and not r["merge"] and r["k"] != 7,
        "folded, not merged: MGACBAM_BWD_MERGE=0 at k = 7": lambda r: r["fold"] and not r["merge"] and r["k"] == 7 and r["env"],
        "unfolded: TP < W": lambda r: not r["fold"] and r["ctx"] * r["vec"] < r["W"] <= 128,
        "unfolded: W > 128": lambda r: not r["fold"] and r["W"] > 128,
        "merged with cpt 2": lambda r: r["merge"] and r["cpt_b"] == 2,
        # projection planes
        "no planes: hidden > 16": lambda r: r["gmask"] and f32(r) and r["hid"] > 16 and r["make_proj"] == 0,
        "VALU planes": lambda r: r["make_proj"] == 1 and r["hid"] <= 4,
        "MFMA planes, hidden 8": lambda r: r["make_proj"] == 2 and r["hid"] == 8,
        "MFMA planes, hidden 12": lambda r: r["make_proj"] == 2 and r["hid"] == 12,
        "MFMA planes, hidden 16": lambda r: r["make_proj"] == 2 and r["hid"] == 16,
        "MFMA planes at exactly 1 MiB": lambda r: r["make_proj"] == 2 and r["B"] * r["C"] * r["H"] * r["W"] * 4 == ONE_MIB,
        "hidden 5..16 below 1 MiB: x is read": lambda r: (r["gmask"] and f32(r) and 4 < r["hid"] <= 16 and r["vec"] == 4 and r["ctx"] in (16, 32)
                                                           and r["make_proj"] == 0),
        "the no-x k_bwd_apply": lambda r: r["nox"],
        "its NEEDX twin (fp32, vec 4, gmask, no planes)": lambda r: r["gmask"] and f32(r) and r["vec"] == 4 and not r["nox"],
        "VALU planes at vec 1 (x-reading instantiation)": lambda r: r["make_proj"] == 1 and r["vec"] == 1,
        "half precision never makes planes": lambda r: half(r) and r["gmask"] and r["hid"] <= 16 and r["make_proj"] == 0,
        "early prologue loads (C <= 256, hidden <= 8)": lambda r: r["C"] <= 256 and r["hid"] <= 8,
        "late prologue: C > 256": lambda r: r["C"] > 256,
        "late prologue: hidden > 8": lambda r: r["C"] <= 256 and r["hid"] > 8,
        "chunked hidden partials at pool_tx 1": lambda r: r["chunked_pgh"] and r["tx"] == 1,
        # mask
        "no mask": lambda r: r["kind"] == "none",
        "mask without grad": lambda r: r["kind"] != "none" and not r["mask_grad"],
        "3-D mask": lambda r: r["mask3d"],
        "raw-probability mask, fp32": lambda r: r["kind"] == "prob" and f32(r),
        "raw-probability mask, half": lambda r: r["kind"] == "prob" and half(r),
        "a tiny sample inside a mixed batch": lambda r: r["kind"] == "mixed" and r["B"] > 2 and r["thr"] > 0,
        "every sample tiny (use = 0)": lambda r: r["kind"] == "tiny" and r["thr"] > 0,
        "all_negative": lambda r: r["kind"] == "all_negative",
        "use = 1 with S < eps": lambda r: r["kind"] == "tiny" and r["thr"] == 0.0,
    }
    missed = [b for b, hit in branches.items() if not any(hit(r) for r in rows)]
    assert not missed, missed
    assert {r["k"] for r in rows} == {1, 3, 5, 7, 9, 15}
    assert {"none", "tiny", "all_negative", "prob", "mixed", "sparse", "randn"} <= {r["kind"] for r in rows}
    by = {r["name"]: r for r in rows if not r["env"]}
    assert {by[n]["dt"] for n in KNOB_ROWS} == {"f32", "f16", "bf16"} and {by[n]["vec"] for n in KNOB_ROWS} == {1, 4}
    assert max(by[n]["B"] * by[n]["C"] * by[n]["H"] * by[n]["W"] for n in KNOB_ROWS) <= 1 << 16


@pytest.mark.parametrize("name", ROW_IDS)
def test_the_oracle_alone_stays_inside_the_guards(name):
    """row_case asserts on the host that no sample's S / N is within 1e-3 of tiny_thr and no S within 1e-3 of eps, that at most 4 pixels have
    a channel arg-max decided by < 1e-6 relative and at most 2 channels a masked maximum with such a runner-up, and, for the tiny_thr = 0
    row, that the fp64 autograd oracle and the hand-derived one agree to 1e-9; and that plain fp32 torch ops hold the element-wise bars with a
    factor of two to spare (assert_fp32_holds_the_bars).  A row that cannot gets another seed or milder parameters, not a larger cap."""
    c = row_case(name, fp32_guard=True)
    assert MAX_TIE_PIXELS == 4 and MAX_TIE_CHANNELS == 2
    assert int(c.skip_px.sum()) <= 4 and int(c.skip_ch.sum()) <= 2
    assert c.y_o.dtype == torch.float64 and c.g_o["gx"].shape == c.x.shape and c.g_o["gw1"].shape == (c.hidden, c.C)
    assert (c.g_o["gmask"] is None) == (c.mask is None)
    for key, t in c.g_o.items():
        assert t is None or bool(torch.isfinite(t).all()), key
