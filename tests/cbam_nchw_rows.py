"""What tests/test_gpu_cbam_nchw.py and tests/test_abi_cbam_nchw.py share.  Not a test.

  1. NCHW_ROWS: the shapes at which the NCHW MaskCBAM kernels (csrc/fwd.cuh, csrc/bwd.cuh) are compared element-wise with the fp64 oracle,
     each with the launch form it is there for -- in words in its comment and as numbers in its last column.
  2. cbam_nchw_geo: a restatement BY HAND of host.cuh's vec_of, choose_tune, gate_geometry, pool_forms_ca, group_cpt, wide_proj_shape,
     the tile counts and sync_layout, of api_fwd.hip's gvec and split_mlp rules and of api_bwd.hip's fold / merge / projection-plane / no-x
     rules, for ONE level called alone.  scratch_total / ctx_fields restate scratch_layout / ctx_layout on top of it, and
     tests/test_abi_cbam_nchw.py holds those against the library's own size queries, so the restatement cannot drift from host.cuh
     unnoticed; it has to be brought along with host.cuh by hand.
  3. row_case: a row's inputs, parameters and fp64 oracle outputs, with the host-side guards (branch thresholds, near ties, and that
     plain fp32 arithmetic can hold the bars at the row's inputs).
"""
from types import SimpleNamespace

import torch

from conftest import rel_err, synth
from oracle import maskcbam_oracle as O

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
K_BLOCK = 256                        # common.cuh: kBlock
K_WAVE = 64                          # common.cuh: kWave
K_GATE_R = 16                        # args.cuh: kGateR
K_SYNC_PX = 16                       # args.cuh: kSyncPx
K_ARRIVE_STRIDE = 64                 # args.cuh: kArriveStride
K_PROJ_MAX = 4                       # args.cuh: kProjMax (MGACBAM_PROJ_MAX_HIDDEN)
K_PROJ_WIDE = 16                     # args.cuh: kProjWide
K_PGH_LDS = 2048                     # bwd.cuh: kPghLds
GATE_LDS_BOUND = 48 * 1024           # host.cuh: gate_geometry
ONE_MIB = 1 << 20                    # host.cuh: pool_forms_ca, wide_proj_shape
SPLIT_MLP = 8192                     # api_fwd.hip: split_mlp; host.cuh: pool_forms_ca
MLP_STREAM_MAX_C = 8 * 4 * K_WAVE    # common.cuh: mlp_stream_ok
CHAN_GRID_MIN = 768                  # host.cuh: choose_tune, chan_tx
CPT_BLOCKS_MIN = 1536                # host.cuh: group_cpt
CONV_LOADS = 24 * 256                # host.cuh: choose_tune, conv_th's cap
WSA_LDS_FLOATS = 3500                # host.cuh: choose_tune, wsa_th
FOLD_SPAN_MAX = 512                  # api_bwd.hip: backward_group, fold


def G(**kw):
    return kw


def _pow2_floor(v):
    return 1 << (v.bit_length() - 1)


def _pow2_ceil(v):
    return 1 << (v - 1).bit_length() if v > 1 else 1


def _cdiv(a, b):
    return -(-a // b)


def _gate_geometry(C, H, W, k, vec, narrow):
    """host.cuh's gate_geometry -> dict(gty, gtx, tp, rows, span, lds, the three conditions, ok)."""
    gty = _pow2_ceil(_cdiv(C, K_GATE_R))
    if gty > K_BLOCK:
        return dict(gty=gty, gtx=0, tp=0, rows=0, span=0, lds=0, tp_sync=False, tp_w=False, lds_ok=False, ok=False)
    gtx = K_BLOCK // gty
    tp = gtx * vec
    rows = min((tp - 1) // W + 2, H) + k - 1
    span = ((k // 2) * W + tp - 1) // tp + 1
    lds = (3 * rows * (W + k - 1) + tp + 3 * k * k + 3 * C + 64) * 4
    tp_sync, tp_w, lds_ok = tp >= K_SYNC_PX, tp >= W, lds <= GATE_LDS_BOUND
    return dict(gty=gty, gtx=gtx, tp=tp, rows=rows, span=span, lds=lds, tp_sync=tp_sync, tp_w=tp_w, lds_ok=lds_ok,
                ok=tp_sync and (tp_w or narrow) and lds_ok)


def cbam_nchw_geo(B, C, H, W, k, hidden, dtype="f32", gmask=True, *, pool_tx=0, chan_tx=0, gate_narrow=False, bwd_merge=True):
    """The launch form of one NCHW MaskCBAM level called alone through the autograd path (no SAVE_PROJ / HAVE_PROJ), restated by hand.
    The keywords are the knobs tests/test_abi_cbam_nchw.py forces (MGACBAM_POOL_TX, _CHAN_TX, _GATE_NARROW, _BWD_MERGE); without them, no
    knob is set."""
    HW = H * W
    f32 = dtype == "f32"
    vec = 4 if HW % 4 == 0 else 1                                                 # vec_of
    nv = HW // vec
    # choose_tune: the sweep kernels
    tx = min(_pow2_floor(max(nv // 4, 1)), 256)
    # choose_tune: the tile kernels
    ctx = min(_pow2_ceil(nv), 64)
    while ctx > 16 and B * _cdiv(nv, ctx) < CHAN_GRID_MIN:
        ctx //= 2
    while ctx < 64 and (K_BLOCK // ctx) * 4 > C:
        ctx *= 2
    # choose_tune: the conv tiles
    ntx = _cdiv(W, 128)
    tw = _cdiv(_cdiv(W, ntx), 4) * 4
    twq = tw // 4
    cap = CONV_LOADS // (4 * (tw + k - 1)) - (k - 1)
    th_free = min(K_BLOCK // twq, 64)
    th = max(min(th_free, H, cap), 1)
    wth = max(min(WSA_LDS_FLOATS // (4 * (tw + k - 1)) - (k - 1), H, 64), 1)
    if pool_tx:
        tx = pool_tx
    if chan_tx:
        ctx = chan_tx
    apply_rows = min((ctx * vec - 1) // W + 2, H) + k - 1
    # gate_geometry at the level's vec, then forward_args' gvec 8 rule
    gate = _gate_geometry(C, H, W, k, vec, gate_narrow)
    gvec = vec
    if not f32 and vec == 4 and HW % 8 == 0:
        g8 = _gate_geometry(C, H, W, k, 8, gate_narrow)
        if g8["ok"]:
            gate, gvec = g8, 8
    gtiles = _cdiv(HW // gvec, gate["gtx"]) if gate["ok"] else 0
    # the MLP
    stream = C % 4 == 0 and hidden % 4 == 0 and C <= MLP_STREAM_MAX_C             # mlp_stream_ok
    split_mlp = C * hidden >= SPLIT_MLP
    x_bytes = C * HW * (4 if f32 else 2)
    pool_ca = stream and not split_mlp and gate["ok"] and x_bytes >= ONE_MIB      # pool_forms_ca
    # group_cpt: max_cpt 2 in the forward, 4 in the backward
    def cpt_of(max_cpt):
        c = max_cpt
        while c > 1:
            if B * _cdiv(C, (K_BLOCK // tx) * c) >= CPT_BLOCKS_MIN:
                return c
            c //= 2
        return 1
    cpt_f, cpt_b = cpt_of(2), cpt_of(4)
    cpb_f, cpb_b = (K_BLOCK // tx) * cpt_f, (K_BLOCK // tx) * cpt_b
    # tile counts and flags
    tiles = _cdiv(nv, ctx)
    strips = _cdiv(W, tw)
    conv_tiles = strips * _cdiv(H, th)
    wsa_tiles = strips * _cdiv(H, wth)
    nflag = _cdiv(HW, K_SYNC_PX) + 1
    # backward_group: fold and merge
    tp = ctx * vec
    fold = tp >= K_SYNC_PX and tp >= W and 8 * (((th + k) * W + tp - 1) // tp + 1) <= FOLD_SPAN_MAX and conv_tiles <= nflag
    ncg = _cdiv(C, cpb_b)
    merge = fold and k == 7 and bwd_merge and wsa_tiles <= nflag and ncg <= C
    # backward_args: projection planes
    valu_lds = (((3 * C + 3) & ~3) + C * K_PROJ_MAX + 4 * K_BLOCK * vec) * 4      # reduce1_smem(g, vec, 1)
    wide_shape = K_PROJ_MAX < hidden <= K_PROJ_WIDE and vec == 4 and ctx == 16 and B * C * HW * 4 >= ONE_MIB   # wide_proj_shape
    make_proj = 0
    if gmask and f32 and hidden <= K_PROJ_MAX and valu_lds <= 64 * 1024:
        make_proj = 1
    if gmask and f32 and wide_shape:
        make_proj = 2
    nox = bool(gmask and f32 and vec == 4 and make_proj)
    return dict(vec=vec, nv=nv, tx=tx, rem=nv % tx, ctx=ctx, ty=K_BLOCK // ctx, tiles=tiles, last=nv - (tiles - 1) * ctx,
                twq=twq, tw=tw, strips=strips, last_strip=W - (strips - 1) * tw, th=th, th_by=("cap" if cap < min(th_free, H) else
                                                                                             "H" if H < th_free else "free"),
                wth=wth, apply_rows=apply_rows, conv_tiles=conv_tiles, wsa_tiles=wsa_tiles, nflag=nflag,
                gate=gate["ok"], gty=gate["gty"], gtx=gate["gtx"] if gate["ok"] else 0, gtp=gate["tp"], grows=gate["rows"],
                span=gate["span"] if gate["ok"] else 0, gate_lds=gate["lds"], tp_sync=gate["tp_sync"], tp_w=gate["tp_w"],
                lds_ok=gate["lds_ok"], gvec=gvec, gtiles=gtiles,
                stream=stream, split_mlp=split_mlp, pool_ca=pool_ca, x_bytes=x_bytes,
                cpt_f=cpt_f, cpt_b=cpt_b, cpb_f=cpb_f, cpb_b=cpb_b, crem_f=C % cpb_f, crem_b=C % cpb_b, ncg=ncg,
                fold=fold, merge=merge, make_proj=make_proj, wide_shape=wide_shape, nox=nox,
                chunked_pgh=hidden > K_PGH_LDS // (K_BLOCK // tx))


class _Carver:
    """host.cuh's Carver: 16-byte aligned fields of 4-byte elements, in the order they are taken."""

    def __init__(self):
        self.total = 0

    def take(self, n):
        off = self.total
        self.total = (self.total + 4 * n + 15) // 16 * 16
        return off


def sync_len(B, C, H, W):
    """host.cuh's sync_layout: six (B, nflag) flag classes, 4 status words, (B) ca flags, (B, C) sweep flags, the arrival words."""
    per = B * (_cdiv(H * W, K_SYNC_PX) + 1)
    return 6 * per + 4 + B + B * C + B * K_ARRIVE_STRIDE


def ctx_fields(B, C, H, W, hidden):
    """host.cuh's ctx_layout -> {field: byte offset} and total."""
    HW, BC = H * W, B * C
    cv = _Carver()
    out = {}
    for name, n in (("S", B), ("use", B), ("den", B), ("avg", BC), ("mx", BC), ("mavg", BC), ("valid", BC), ("amax", BC),
                    ("h_avg", B * hidden), ("h_mx", B * hidden), ("ca", BC), ("planes", B * 3 * HW), ("cidx", B * HW), ("sa", B * HW),
                    ("proj", B * hidden * HW if hidden <= K_PROJ_MAX else 0), ("sync", sync_len(B, C, H, W))):
        out[name] = cv.take(n)
    out["status"] = out["sync"] + 4 * B * (_cdiv(HW, K_SYNC_PX) + 1)
    out["total"] = cv.total
    return out


def scratch_total(B, C, H, W, hidden, k, g):
    """host.cuh's scratch_layout of an NCHW level from a restated geometry g (the layout does not depend on the element type)."""
    HW, BC = H * W, B * C
    cv = _Carver()
    cv.take(2 * BC * g["tiles"])                       # A_part
    cv.take(B * HW)                                    # gpre
    cv.take(B * 3 * HW)                                # gplanes
    cv.take(B * g["wsa_tiles"] * 3 * k * k)            # gwsa_part
    cv.take(BC); cv.take(BC)                           # gz, gbq
    cv.take(B * hidden); cv.take(B * hidden)           # gh_avg, gh_mx
    cv.take(B * _cdiv(C, K_BLOCK // g["tx"]) * hidden)  # pgh
    cv.take(B * hidden * HW if g["wide_shape"] else 0)  # proj
    return cv.total


# Columns: name, dtype, B, C, H, W, k, hidden, mask kind, 3-D mask, mask requires grad, tiny_thr, geometry.
# In the comments and the geometry column: vec = elements per lane access (vec_of); tx = pool_tx, rem = (H*W / vec) % tx (a ragged last sweep
# when non-zero), cpt_f / cpt_b = channels per thread of k_pool / the backward sweeps, crem = C % CPB (the last workgroup's clamped channels);
# ctx = chan_tx, ty = 256 / ctx channel slices, tiles per sample with `last` active lanes in the last one; gate = k_gate eligible, gtx its lanes
# along H*W, gvec its elements per lane, gtiles its tiles per sample, span the tiles a window reaches; strips = column strips of the conv
# tiles, th / wth = rows of a conv / dWsa tile; fold / merge = the backward form; make_proj 1 = VALU planes, 2 = MFMA planes; nox = the
# k_bwd_apply that cannot read x; pool_ca = k_pool's last arriver forms ca.
NCHW_ROWS = [
    # vec 1, tx 64 ragged (391 % 64 = 7), CPB 4 with C % 4 = 2 (clamped channels), ctx 16 with 7 lanes in the last of 25 tiles; k_gate refused
    # because a 16-pixel tile is narrower than the 17-pixel row, and for the same reason the backward is unfolded; MLP staged (C % 4 != 0);
    # sample 2 of the mixed batch is tiny (use = 0, GAP fallback); hidden 8 but vec 1: x is read for dL/dmask
    ("v1_tx64_c130", "f32", 3, 130, 23, 17, 3, 8, "mixed", False, True, 1e-4,
     G(vec=1, tx=64, rem=7, cpb_f=4, crem_f=2, ctx=16, tiles=25, last=7, gate=False, tp_w=False, tp_sync=True, lds_ok=True, fold=False, stream=False,
       make_proj=0, nox=False)),
    # vec 1 WITH k_gate (one 64-pixel tile per sample, generic k), ctx 32, folded but not merged (k = 5), MLP staged because hidden % 4 != 0,
    # VALU planes at vec 1 (k_bwd_apply keeps the instantiation that can read x)
    ("v1_gate_k5", "f32", 2, 48, 9, 7, 5, 3, "randn", False, True, 1e-4,
     G(vec=1, tx=8, rem=7, ctx=32, tiles=2, last=31, gate=True, gtx=64, gtiles=1, fold=True, merge=False, stream=False, make_proj=1, nox=False)),
    # one k_gate tile per sample spanning every image row, merged backward, VALU planes, the no-x k_bwd_apply, streamed MLP, early prologue
    ("one_tile_merged", "f32", 2, 64, 16, 16, 7, 4, "sparse", False, True, 1e-4,
     G(vec=4, tx=16, ctx=16, tiles=4, gate=True, gtx=64, gtiles=1, span=2, fold=True, merge=True, stream=True, make_proj=1, nox=True, pool_ca=False)),
    # x of a sample is exactly 1 MiB: k_pool's last arriver forms ca, with B = 1; tx 256, 16 k_gate tiles, conv_th 15 by its cap, 11 dWsa tiles
    ("pool_ca_b1", "f32", 1, 64, 64, 64, 7, 4, "randn", False, True, 1e-4,
     G(vec=4, tx=256, rem=0, ctx=16, tiles=64, gate=True, gtx=64, gtiles=16, pool_ca=True, x_bytes=1 << 20, th=15, th_by="cap", wth=6, conv_tiles=5,
       wsa_tiles=11, merge=True, make_proj=1, nox=True)),
    # the same level with B = 9: nine arrival words, XCD padding ids
    ("pool_ca_b9", "f32", 9, 64, 64, 64, 7, 4, "mixed", False, True, 1e-4,
     G(vec=4, tx=256, gate=True, gtiles=16, pool_ca=True, x_bytes=1 << 20, merge=True, make_proj=1, nox=True)),
    # 4 032 pixels: 16 128 bytes short of 1 MiB, so k_gate's role workgroups form ca; tx 128 ragged (1008 % 128 = 112); mask without grad
    # (the GMASK = false instantiations, no planes)
    ("below_1mib_nograd", "f32", 1, 64, 63, 64, 7, 4, "randn", False, False, 1e-4,
     G(vec=4, tx=128, rem=112, gate=True, gtiles=16, stream=True, split_mlp=False, pool_ca=False, x_bytes=1032192, merge=True, make_proj=0, nox=False)),
    # bf16 and fp16: 16-byte k_gate lanes (gvec 8) with k_pool forming ca under the 2-byte bytes rule (128 x 4096 x 2 = 1 MiB); no planes
    ("bf16_gvec8_pool_ca", "bf16", 2, 128, 64, 64, 7, 8, "randn", False, True, 1e-4,
     G(vec=4, gvec=8, gate=True, gtx=32, gtiles=16, pool_ca=True, x_bytes=1 << 20, merge=True, make_proj=0, nox=False)),
    ("f16_gvec8_pool_ca", "f16", 2, 128, 64, 64, 7, 8, "sparse", False, True, 1e-4,
     G(vec=4, gvec=8, gate=True, gtx=32, gtiles=16, pool_ca=True, x_bytes=1 << 20, merge=True, make_proj=0, nox=False)),
    # MFMA planes, hidden 8 at 1.6 MB; tx 64 ragged (400 % 64 = 16), 13 k_gate tiles of 128 pixels, the last partial
    ("mfma_h8", "f32", 2, 128, 40, 40, 7, 8, "randn", False, True, 1e-4,
     G(vec=4, tx=64, rem=16, ctx=16, tiles=25, gate=True, gtx=32, gtiles=13, merge=True, make_proj=2, nox=True, th_by="free", wsa_tiles=4)),
    # MFMA planes, hidden 12 (rows 12..15 of the MFMA's A operand are padding), B = 8
    ("mfma_h12", "f32", 8, 64, 32, 32, 7, 12, "mixed", False, True, 1e-4, G(vec=4, tx=64, ctx=16, merge=True, make_proj=2, nox=True, gtiles=4)),
    # MFMA planes, hidden 16, at exactly 1 MiB
    ("mfma_h16", "f32", 4, 64, 32, 32, 7, 16, "sparse", False, True, 1e-4, G(vec=4, ctx=16, merge=True, make_proj=2, nox=True)),
    # hidden 8 below 1 MiB: no planes, k_bwd_apply reads x (the NEEDX twin of the no-x rows); ctx 32; streamed MLP with C = 40
    ("h8_needx_ctx32", "f32", 2, 40, 24, 24, 7, 8, "randn", False, True, 1e-4,
     G(vec=4, tx=32, rem=16, ctx=32, tiles=5, last=16, gate=True, gtx=64, gtiles=3, merge=True, make_proj=0, nox=False, wide_shape=False)),
    # split_mlp (512 x 32 >= 8192: k_gate's role workgroups run the MLP, never k_pool), gate_tx 8, 13 tiles of 32 pixels with span 3; hidden > 16:
    # no planes; C > 256: the late prologue of k_bwd_apply; last chan tile 4 lanes
    ("split_mlp_gtx8", "f32", 2, 512, 20, 20, 7, 32, "randn", False, True, 1e-4,
     G(vec=4, tx=16, rem=4, ctx=16, tiles=7, last=4, gate=True, gtx=8, gtiles=13, span=3, split_mlp=True, pool_ca=False, merge=True, make_proj=0)),
    # W = 260: three column strips of 88, the last 84 wide; ctx 64 through the ">= 4 channels per row" widening; k_gate with 1024-pixel tiles
    # (gate_tx 256) at 40 244 B of LDS; unfolded because a 256-pixel tile is narrower than the row; tx 128 ragged
    ("w260_3strips", "f32", 1, 16, 8, 260, 7, 4, "randn", False, True, 1e-4,
     G(vec=4, tx=128, rem=8, ctx=64, tiles=9, last=8, strips=3, last_strip=84, th=8, th_by="H", wth=3, wsa_tiles=9, gate=True, gtx=256, gtiles=3,
       gate_lds=40244, fold=False, make_proj=1, nox=True)),
    # W = 400: four strips; k_gate refused by the LDS bound alone (53 852 B > 48 KB)
    ("w400_gate_lds", "f32", 1, 16, 8, 400, 7, 4, "sparse", False, True, 1e-4,
     G(vec=4, ctx=64, strips=4, wth=2, wsa_tiles=16, gate=False, tp_sync=True, tp_w=True, lds_ok=False, gate_lds=53852, fold=False, make_proj=1)),
    # W = 150: two strips of 76, the last 74 wide; k_gate refused because a 64-pixel tile is a fraction of a row (runs again under
    # MGACBAM_GATE_NARROW=1, ENV_ROWS); unfolded with W > 128; last chan tile 1 lane; hidden 16 below 1 MiB: no planes
    ("w150_narrow", "f32", 1, 256, 6, 150, 7, 16, "randn", False, True, 1e-4,
     G(vec=4, tx=32, rem=1, ctx=16, tiles=15, last=1, strips=2, last_strip=74, gate=False, tp_sync=True, tp_w=False, lds_ok=True, fold=False,
       make_proj=0, nox=False)),
    # a k_gate tile is exactly one image row (64 pixels, gate_tx 16), five tiles, span 4; hidden 16 with C <= 256
    ("gate_one_row", "f32", 1, 256, 5, 64, 7, 16, "sparse", False, True, 1e-4,
     G(vec=4, gate=True, gtx=16, gtp=64, gtiles=5, span=4, merge=True, make_proj=0)),
    # MLP staged because C > 2048 alone (C % 4 = 0, hidden % 4 = 0); k_gate refused because a tile (4 pixels) is below kSyncPx alone
    ("c2052_staged", "f32", 1, 2052, 4, 4, 7, 4, "randn", False, True, 1e-4,
     G(vec=4, nv=4, tx=1, ctx=4, tiles=1, last=4, gate=False, tp_sync=False, tp_w=True, lds_ok=True, stream=False, split_mlp=True, merge=True)),
    # C > 4096: gty 512 > 256 refuses k_gate; nv = 1, ctx 1
    ("c4100_gty", "f32", 1, 4100, 2, 2, 3, 4, "randn", False, True, 1e-4, G(vec=4, nv=1, tx=1, ctx=1, gty=512, gate=False, fold=False)),
    # W = 1, hidden = C = 256 (hidden > kPghLds / 256 rows: chunked hidden partials in k_bwd_reduce2), ctx 8 with 7 active lanes
    ("w1_hidden_eq_c", "f32", 3, 256, 28, 1, 7, 256, "mixed", False, True, 1e-4,
     G(vec=4, nv=7, tx=1, ctx=8, tiles=1, last=7, gate=True, gtx=16, split_mlp=True, merge=True, chunked_pgh=True)),
    # nv = 1: one lane of one tile; hidden 16 > 2048 / 256: chunked hidden partials at pool_tx 1
    ("nv1_chunked_pgh", "f32", 2, 64, 2, 2, 7, 16, "randn", False, True, 1e-4,
     G(vec=4, nv=1, tx=1, ctx=16, tiles=1, last=1, gate=True, merge=True, chunked_pgh=True, make_proj=0)),
    # k = 15 > C = 7, B = 11 (XCD padding ids), 3-D mask; vec 1 at tx 128 ragged, ctx 64 (TY 4 < C < 2 TY), gate_tx 256 at vec 1, conv_th 19 by its
    # cap, 6 dWsa tiles of 5 rows
    ("k15_b11_mask3d", "f32", 11, 7, 30, 31, 15, 2, "mixed", True, True, 1e-4,
     G(vec=1, tx=128, rem=34, ctx=64, tiles=15, last=34, gate=True, gtx=256, gtiles=4, th=19, th_by="cap", wth=5, wsa_tiles=6, fold=True, merge=False,
       make_proj=1, nox=False)),
    # W = 1 and C = 3 < TY = 4: both prefetched channel slices clamped; every sample tiny (use = 0); hidden 1, k = 3
    ("w1_c3_tiny", "f32", 2, 3, 9, 1, 3, 1, "tiny", False, True, 1e-4, G(vec=1, tx=2, rem=1, ctx=64, ty=4, tiles=1, last=9, gate=True, gtx=256)),
    # last chan tile of ONE lane (33 = 2 * 16 + 1); raw-probability mask in fp32
    ("last_lane_prob", "f32", 2, 64, 12, 11, 7, 4, "prob", False, True, 1e-4, G(vec=4, tx=8, rem=1, ctx=16, tiles=3, last=1, merge=True, nox=True)),
    # no mask (HAS_MASK false, gmask None), k = 9, hidden 6 (staged: hidden % 4 != 0), C % CPB = 8
    ("nomask_k9", "f32", 2, 72, 10, 10, 9, 6, "none", False, False, 1e-4, G(vec=4, tx=4, rem=1, ctx=16, tiles=2, last=9, crem_f=8, stream=False, fold=True,
                                                                             merge=False)),
    # tiny_thr = 0: use = 1 with S = 144 * sigmoid(-20) < eps, so live = 0 (no K_b term in dL/dmask) and den = eps; k = 3
    ("live0", "f32", 2, 40, 12, 12, 3, 4, "tiny", False, True, 0.0, G(vec=4, tx=8, rem=4, ctx=32, tiles=2, last=4, merge=False, make_proj=1, nox=True)),
    # all_negative mask: no pixel selected, every channel invalid (mx falls back to GAP); fp16 with H*W % 8 = 4: gvec stays 4
    ("f16_gvec4_allneg", "f16", 3, 64, 6, 6, 7, 4, "all_negative", False, True, 1e-4,
     G(vec=4, gvec=4, tx=2, rem=1, ctx=16, tiles=1, last=9, gate=True, merge=True, make_proj=0, nox=False)),
    # the scalar 2-byte path in fp16 (vec 1), k = 1, hidden = 1, all_negative
    ("f16_scalar_k1_h1", "f16", 3, 33, 5, 7, 1, 1, "all_negative", False, True, 1e-4,
     G(vec=1, gvec=1, tx=8, rem=3, ctx=32, tiles=2, last=3, crem_f=1, gate=True, span=1, merge=False)),
    # the scalar 2-byte path in bf16, k = 9, B = 13, mixed batch
    ("bf16_scalar_k9", "bf16", 13, 33, 5, 7, 9, 2, "mixed", False, True, 1e-4, G(vec=1, gvec=1, tx=8, rem=3, ctx=32, tiles=2, last=3, gate=True)),
    # bf16 gvec 8 at generic k (k_gate's K = 0 instantiation with 16-byte lanes), one tile; raw-probability mask in half precision
    ("bf16_gvec8_k5", "bf16", 2, 72, 8, 8, 5, 4, "prob", False, True, 1e-4, G(vec=4, gvec=8, gtx=32, gtiles=1, gate=True, fold=True, merge=False)),
    # cpt 2 by group_cpt at the forward's AND the backward's max_cpt (8 * ceil(401 / 2) = 1608 >= 1536 > 8 * ceil(401 / 4)), tx 256, C odd (the
    # last workgroup's second channel clamped); three-launch forward (a 32-pixel tile < W), merged backward with MFMA planes; 53 MB
    ("cpt2_tx256", "f32", 8, 401, 64, 64, 7, 8, "sparse", False, True, 1e-4,
     G(vec=4, tx=256, cpt_f=2, cpt_b=2, cpb_f=2, crem_f=1, crem_b=1, gate=False, tp_w=False, merge=True, make_proj=2, nox=True)),
    # cpt 2 at tx 64: CPB 8 with C % 8 = 2 (16 * ceil(770 / 8) = 1552 >= 1536); k = 5: folded, not merged; split_mlp as a launch (k_mlp); 50 MB
    ("cpt2_c770_k5", "f32", 16, 770, 32, 32, 5, 48, "randn", False, True, 1e-4,
     G(vec=4, tx=64, cpt_f=2, cpt_b=2, cpb_f=8, crem_f=2, gate=False, split_mlp=True, fold=True, merge=False, make_proj=0)),
]
ROW_IDS = [r[0] for r in NCHW_ROWS]
SEEDS = {}                            # rows whose default seed (300 + C + H) puts the oracle outside the guards' caps
# Amplitude of the parameter perturbation where 0.3 is too much for fp32: added to 770 x 48 weights it drives |z| to 150, the sums behind z
# then carry ~1e-5 of absolute rounding error in fp32, and plain fp32 torch ops on the host miss the element-wise bar themselves (gx 3.3e-3
# against the fp64 oracle at cpt2_c770_k5; 8.9e-4 at split_mlp_gtx8, 512 x 32; 5.1e-4 at cpt2_tx256, 401 x 8 over 32 768 pixels).  These
# three are the rows assert_fp32_holds_the_bars refuses at 0.3; every other row keeps 0.3.  0.03 is the default initialisation's own scale at
# C = 770
AMP = {"cpt2_c770_k5": 0.03, "split_mlp_gtx8": 0.1, "cpt2_tx256": 0.1}
# the rows the forced launch forms run: fp32 at vec 1 and vec 4, fp16, bf16 at vec 1 and with 16-byte k_gate lanes -- all small
KNOB_ROWS = ["v1_gate_k5", "one_tile_merged", "f16_gvec4_allneg", "bf16_scalar_k9", "bf16_gvec8_k5"]
# rows that run a second time under one knob, with the geometry the knob gives them
ENV_ROWS = {"w150_narrow": dict(MGACBAM_GATE_NARROW="1"), "one_tile_merged": dict(MGACBAM_BWD_MERGE="0")}


def cbam_params(C, k, hidden, seed, amp=0.3):
    """Default-initialised parameters at the row's hidden width, perturbed as test_gpu_channels_last_edges._params does (amp 0.3)."""
    p = O.Params.default_init(C, r=max(C // hidden, 1), k=k, seed=seed)
    if p.w1.shape[0] != hidden:                          # C // r does not hit every width: the same init at the width itself
        import torch.nn as nn
        torch.manual_seed(seed)
        l1, l2 = nn.Linear(C, hidden), nn.Linear(hidden, C)
        p = O.Params(l1.weight.detach().clone(), l1.bias.detach().clone(), l2.weight.detach().clone(), l2.bias.detach().clone(), p.wsa,
                     p.beta)
    with torch.no_grad():
        for t in (p.w1, p.b1, p.w2, p.b2):
            t.add_(amp * torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)))
        p.wsa.mul_(3.0)
        p.beta.fill_(0.4)
    return p


def assert_off_thresholds(name, mask, use_sig, tiny_thr, eps, N):
    """fp32 and fp64 must take the same branches: no sample's S / N within 1e-3 (relative) of tiny_thr, no S within 1e-3 of eps."""
    if mask is None:
        return
    m = mask.double().reshape(mask.shape[0], -1)
    S = (m.sigmoid() if use_sig else m).sum(dim=1)
    assert bool(((S / N - tiny_thr).abs() > 1e-3 * tiny_thr).all()), f"{name}: a sample's S/N sits on tiny_thr; change the seed"
    assert bool(((S - eps).abs() > 1e-3 * eps).all()), f"{name}: a sample's S sits on eps; change the seed"


def near_tie_pixels(x, c):
    """(B, H*W) pixels whose channel arg-max is decided by < 1e-6 relative (test_gpu_channels_last_edges._near_tie_pixels): the device's ca
    differs from the oracle's by ~1e-7, so there cidx and the routed sub-gradient may take either channel."""
    B, C = x.shape[:2]
    if C < 2:
        return torch.zeros(B, x.shape[2] * x.shape[3], dtype=torch.bool)
    u = x.double().reshape(B, C, -1) * c.ca.double().reshape(B, C, 1)
    top = u.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    return (gap > 0) & (gap <= 1e-6 * top[:, 0].abs())


def near_tie_channels(x, mask, use_sig, c):
    """(B, C) valid channels whose masked maximum has a runner-up at ANOTHER pixel within 1e-6 relative, not exactly equal: x is exact on the
    device, so only such a runner-up could move amax, and none of these rows has one in practice -- the cap is what says so."""
    B, C = x.shape[:2]
    xf = x.double().reshape(B, C, -1)
    if xf.shape[2] < 2:
        return torch.zeros(B, C, dtype=torch.bool)
    if mask is not None:
        m = mask.double().reshape(B, 1, -1)
        sel = (m.sigmoid() if use_sig else m) > 0.5
        xf = torch.where(sel, xf, torch.full_like(xf, -float("inf")))
    top = xf.topk(2, dim=2).values
    gap = top[..., 0] - top[..., 1]
    return c.valid & torch.isfinite(top[..., 1]) & (gap > 0) & (gap <= 1e-6 * top[..., 0].abs())


MAX_TIE_PIXELS, MAX_TIE_CHANNELS = 4, 2


def assert_fp32_holds_the_bars(name, x, mask, gy, p, cfg, y_o, g_o, skip_px):
    """The element-wise bars are fp32 bars: a row is only a fair test of fp32 kernels if the same arithmetic in plain fp32 torch ops on the
    host holds them, with a factor of two to spare (another order of summation moves the error by about that much).  A row that cannot is
    ill-conditioned as an input -- it gets milder parameters (AMP) or another seed, and no bar moves.  The figure depends on the host's
    order of summation (c4100_gty at 0.3: gx 1.1e-4 on one host, 1.1e-3 on another, with the same torch), so it is a property of the row
    that tests/test_abi_cbam_nchw.py checks on the CPU (row_case(name, fp32_guard=True)); the GPU tests do not evaluate it."""
    from conftest import elem_err
    y32, c32 = O.forward(x, mask, p, cfg)
    g32 = O.backward(gy, x, mask, p, cfg, c32)
    keep = (~skip_px).reshape(x.shape[0], 1, *x.shape[2:])
    for key, got, want in (("y", y32, y_o), ("gx", g32["gx"] * keep, g_o["gx"] * keep), ("gmask", g32["gmask"], g_o["gmask"])):
        if want is not None:
            e = elem_err(got, want)
            assert e < 0.5e-3, f"{name}: plain fp32 ops give {key} an element-wise error of {e:.2e}: the row is too ill-conditioned for the bars"


def oracle64(x, mask, gy, p, use_sig, tiny_thr=1e-4, eps=1e-6):
    """The hand-derived oracle in fp64 -> (y, grads, Ctx)."""
    cfg = O.Config(use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=eps)
    m = None if mask is None else mask.double()
    pp = p.to(torch.float64)
    y_o, c = O.forward(x.double(), m, pp, cfg)
    return y_o, O.backward(gy.double(), x.double(), m, pp, cfg, c), c


_cases = {}
GRADS = ("gx", "gmask", "gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta")


def row_case(name, fp32_guard=False):
    """-> the row's inputs (x / gy already rounded to its dtype, as fp32), parameters, fp64 oracle outputs and guards.  Rows that several
    tests run are computed once and shared: their tensors must not be written to."""
    if name in _cases:
        return _cases[name]
    row = NCHW_ROWS[ROW_IDS.index(name)]
    _, dt, B, C, H, W, k, hidden, kind, mask3d, mask_grad, tiny_thr, _ = row
    x, mask, gy = synth(B, C, H, W, seed=SEEDS.get(name, 300 + C + H), mask_kind=kind, mask3d=mask3d)
    use_sig = kind != "prob"
    p = cbam_params(C, k, hidden, seed=C, amp=AMP.get(name, 0.3))
    if dt != "f32":
        x, gy = x.to(DT[dt]).float(), gy.to(DT[dt]).float()
    assert_off_thresholds(name, mask, use_sig, tiny_thr, 1e-6, H * W)
    y_o, g_o, c = oracle64(x, mask, gy, p, use_sig, tiny_thr)
    if tiny_thr == 0.0:
        # use = 1 with S < eps: the hand-derived backward's `live` term shares its derivation with the kernel, so the oracle of this row is
        # fp64 autograd of the eager-op form, and the two oracles must agree (1e-9: fp64 rounding of these sums, with margin)
        assert bool((mask.double().sigmoid().reshape(B, -1).sum(dim=1) < 1e-6).all()), name
        y_a, g_a = O.reference_form_step(x.double(), mask.double(), p.to(torch.float64),
                                         O.Config(use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=1e-6), gy.double())
        assert rel_err(y_o, y_a) < 1e-9, name
        for key in GRADS:
            assert g_o[key].shape == g_a[key].shape and rel_err(g_o[key], g_a[key]) < 1e-9, (name, key)
        y_o, g_o = y_a, g_a
    skip_px = near_tie_pixels(x, c)
    skip_ch = near_tie_channels(x, mask, use_sig, c)
    assert int(skip_px.sum()) <= MAX_TIE_PIXELS, f"{name}: {int(skip_px.sum())} channel arg-max near-ties; change the seed"
    assert int(skip_ch.sum()) <= MAX_TIE_CHANNELS, f"{name}: {int(skip_ch.sum())} masked-max near-ties; change the seed"
    if fp32_guard:
        assert_fp32_holds_the_bars(name, x, mask, gy, p, O.Config(use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=1e-6), y_o, g_o, skip_px)
    case = SimpleNamespace(name=name, dt=dt, dtype=DT[dt], B=B, C=C, H=H, W=W, k=k, hidden=hidden, x=x, mask=mask, gy=gy, p=p, use_sig=use_sig,
                           mask_grad=mask_grad, tiny_thr=tiny_thr, eps=1e-6, y_o=y_o, g_o=g_o, c=c, skip_px=skip_px, skip_ch=skip_ch)
    if name in KNOB_ROWS or name in ENV_ROWS:
        _cases[name] = case
    return case
