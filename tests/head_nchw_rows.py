"""What tests/test_gpu_head_nchw.py and tests/test_abi_head_nchw.py share.  Not a test.

  1. HEAD_NCHW_ROWS: the shapes at which the NCHW mask-head kernels (csrc/head.cuh) are compared element-wise with the fp64 oracle, each
     with the launch geometry it is there for -- in words in its comment and as numbers in its last column.
  2. head_geo: a restatement BY HAND of api_head.hip's head_waves, head_tiling (NCHW branch), head_ctx_layout and head_scratch_layout, of
     head.cuh's head_out_shape, and of what head_gemm_body, k_head_bwd_gw and k_head_bwd_gw2 make of them (K steps and their split over
     the K waves, M blocks, the last tile's pixels, pixel shares).  tests/test_abi_head_nchw.py holds every row's numbers against it on
     the CPU, and its byte counts against the library's size queries; the rest has to be brought along with the sources by hand.
  3. row_case: a row's module state, inputs and oracle outputs with their term magnitudes (oracle/maskhead_oracle.py).
"""
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                 # (tests/conftest.py does the same; this keeps `python tests/head_nchw_rows.py` working)
    sys.path.insert(0, ROOT)
from abi_header import a16  # noqa: E402
from oracle import maskhead_oracle as HO  # noqa: E402

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
K_BLOCK = 256                        # common.cuh: kBlock
HEAD_CB = 64                         # head.cuh: kHeadCB, channels of x per k_head_bwd_gw[2] workgroup
HEAD_GW_PX = 64                      # head.cuh: kHeadGwPx, pixels per chunk of k_head_bwd_gw2
HEAD_GW_DIV = 5                      # api_head.hip: kHeadGwDiv, 64-pixel chunks per k_head_bwd_gw2 workgroup
HEAD_PAR = 16                        # head.cuh: kHeadPar
HEAD_NSTAT = 12                      # head.cuh: kHeadNStat
HEAD_OUT_PAR_CH = 128                # head.cuh: kHeadOutParCh
HEAD_JC = 4                          # head.cuh: kHeadJC
OUTPUTS = ("logits", "gx", "gw1", "ggamma", "gbeta", "gwh", "gbh", "running_mean", "running_var")
TOL = {"f32": 1e-4, "f16": 4e-3, "bf16": 3e-2}          # the project's tensor-scale bars (test_maskhead.py)
# u (oracle.maskhead_oracle.elem_u) of the fp32 oracle at one thread against the fp64 oracle, worst over every f32 case of the table below:
# measure_oracle_u() (python tests/head_nchw_rows.py prints it; test_abi_head_nchw.py holds the table to it within a factor of 4; DESIGN.md has the table with the case each figure is from)
U_ORACLE32 = dict(logits=3.2e-7, gx=5.3e-6, gw1=1.2e-6, ggamma=5.1e-7, gbeta=4.6e-7, gwh=5.2e-6, gbh=6.4e-8, running_mean=1.3e-7,
                  running_var=2.2e-7)
# the device sums in another order (MFMA K steps of 4, K-split waves, two-stage fixed-order partials), none of it worse than a small
# multiple of the serial fp32 sum: 8 x; and what passes through SiLU carries sigmoid_fast (common.cuh: ~1e-6 relative, up to three times in
# SiLU'): + 4e-6.  gbh = sum g and the running statistics never see a sigmoid.
SILU_OUTPUTS = ("logits", "gx", "gw1", "ggamma", "gbeta", "gwh")
U_BAR = {k: 8 * v + (4e-6 if k in SILU_OUTPUTS else 0.0) for k, v in U_ORACLE32.items()}
HALF_FLOOR = {"f32": 0.0, "f16": 2.0 ** -14, "bf16": 2.0 ** -126}   # smallest normal number of the element type (elem_u's floor)


def G(**kw):
    return kw


# Columns: name, dtype(s), B, C, hidden, H, W, also run in eval mode, geometry (keys of head_geo).
# In the comments and the geometry column: vec = pixels per lane access; hidp / cp = hidden / C rounded up to 16; forward GEMM (M = hidden,
# K = C): fw_mtw M tiles per wave, fw_mw waves along M (fw_mw3: 3 remapped to 4), fw_kw waves along K with fw_ksteps K steps, fw_kper per
# wave and fw_kempty waves left without a step, fw_pw waves along pixels, tile_px pixels per workgroup, tps tiles per sample of which the
# last holds last_px, fw_mblk passes of the M loop, fw_w the form the weights are read in ("perm": 16-byte loads, "guard": those with the
# kk0 < K guard live because C % 16 != 0, "gather": C % 4 != 0); gx GEMM (M = C, K = hidden): the same with gx_; k_head_out: out_ppt staged
# pixels per thread, out_mo outputs a run can hold, out_px outputs per run, out_per runs per sample, out_last outputs of the last run,
# out_chunks chunks of kHeadOutParCh channels; k_head_bwd_act: act_ppt, nwg1 runs; dW1: gw2 (the LDS-staged form), ncb channel blocks
# with clast channels in the last, nshare pixel shares over `chunks` pixel chunks, gw_empty shares that own no chunk, gw_uneven (shares
# with different chunk counts), gw_last pixels of a sample's last chunk, gw_passes passes of 64 hidden channels (k_head_bwd_gw).
HEAD_NCHW_ROWS = [
    # vec 1; weights as 16-byte loads with C % 16 = 4 (the kk0 < K guard); out ppt 4; k_head_bwd_gw: 32 shares for 18 chunks (empty shares)
    ("v1_guard", ("f32", "f16", "bf16"), 2, 20, 8, 7, 5, True,
     G(vec=1, fw_w="guard", fw_kw=1, fw_pw=4, tile_px=64, tps=1, last_px=35, out_ppt=4, gw2=0, nshare=32, chunks=18, gw_empty=27)),
    # C % 4 != 0: the gather form of the weights; 2 tiles per sample, the last with 35 pixels
    ("gather_c6", ("f32", "bf16"), 3, 6, 8, 9, 11, True, G(vec=1, fw_w="gather", fw_ksteps=2, tile_px=64, tps=2, last_px=35, gw2=0)),
    # forward kw 4 with 36 K steps of which a wave takes 12: the fourth is empty; ncb 3 with 4 channels in the last block; gx in 2 M
    # blocks (cp 144); gw2; last tile 16 px
    ("ksplit_c132", ("f32", "f16"), 2, 132, 24, 12, 12, True,
     G(vec=4, fw_w="guard", fw_mw=1, fw_kw=4, fw_ksteps=36, fw_kper=12, fw_kempty=1, fw_pw=1, tile_px=64, tps=3, last_px=16, cp=144,
       gx_mw=4, gx_mblk=2, gx_kw=1, gw2=1, ncb=3, clast=4, nshare=1)),
    # forward kw 2 (mw 2); gw2 at hidp 64, ncb 2
    ("kw2_h64", ("f32", "bf16"), 2, 128, 64, 8, 8, False,
     G(vec=4, fw_w="perm", fw_mw=2, fw_kw=2, fw_ksteps=32, fw_kper=16, fw_kempty=0, fw_pw=1, gw2=1, hidp=64, ncb=2, clast=64)),
    # forward mw 3 -> 4 at MTW 2 (hidp 80: 5 tiles); k_head_bwd_gw at vec 4 in 2 passes; last tile 60 px
    ("mw3_h80", ("f32", "f16"), 2, 64, 80, 6, 10, True,
     G(vec=4, hidp=80, fw_mtw=2, fw_mw=4, fw_mw3=True, fw_kw=1, fw_pw=1, tile_px=64, tps=1, last_px=60, gw2=0, gw_passes=2)),
    # the MTW 4 template with forward mw 3 -> 4 (hidp 144: 9 tiles); gx mw 3 -> 4 (cp 96: 6 tiles); ncb 2 with 32 channels in the last
    ("mtw4_h144", ("f32", "bf16"), 2, 96, 144, 5, 8, False,
     G(vec=4, hidp=144, fw_mtw=4, fw_mw=4, fw_mw3=True, gx_mw=4, gx_mw3=True, gx_kw=1, ncb=2, clast=32, gw2=0, gw_passes=3, out_chunks=2)),
    # gx kw 4 with K = 130 (half precision: the half_gx grouping, 36 steps, 12 per wave, one wave empty); hidden > 128: two chunks of
    # kHeadOutParCh; hidp 144 with 14 padded M rows
    ("gxk4_h130", ("f32", "f16", "bf16"), 2, 32, 130, 4, 6, True,
     G(vec=4, hidp=144, gx_mw=1, gx_kw=4, gx_pw=1, gx_ksteps=33, gx_kper=9, gx_kempty=0, gx_ksteps_half=36, gx_kper_half=12,
       gx_kempty_half=1, out_chunks=2, fw_mtw=4, fw_mw=3 + 1, fw_mw3=True)),
    # forward in 2 M blocks (24 tiles > 4 waves x 4); gx kw 2; 12 pixels in all
    ("mblk2_h384", ("f32", "bf16"), 1, 48, 384, 3, 4, True,
     G(vec=4, hidp=384, fw_mtw=4, fw_mw=4, fw_mblk=2, gx_mw=2, gx_kw=2, gx_pw=1, tps=1, last_px=12, out_chunks=3, gw_passes=6)),
    # hidp 256 = exactly one full M block; gx 2 M blocks; ncb 3 with 8 channels in the last block
    ("mfull_h256", ("f32",), 2, 136, 256, 4, 4, False,
     G(vec=4, hidp=256, fw_mtw=4, fw_mw=4, fw_mw3=False, fw_mblk=1, fw_kw=1, cp=144, gx_mblk=2, ncb=3, clast=8, fw_w="guard")),
    # vec 1 with kw 2, 68 K steps (kper 36: the second wave takes 32); tile 16 px, 8 tiles, last 5 px; gx 3 M blocks; ncb 5
    ("v1_kw2_c260", ("f32", "f16"), 2, 260, 48, 9, 13, False,
     G(vec=1, fw_w="guard", fw_mw=2, fw_kw=2, fw_ksteps=68, fw_kper=36, fw_kempty=0, fw_pw=1, tile_px=16, tps=8, last_px=5, cp=272,
       gx_mblk=3, ncb=5, clast=4, gw2=0)),
    # k_head_out in 2 runs per sample (208 outputs at most, 200 taken); pw 2; gw2 with 2 shares over 14 chunks
    ("out2_h40", ("f32", "f16"), 2, 16, 40, 20, 20, False,
     G(vec=4, out_ppt=1, out_mo=208, out_px=200, out_per=2, out_last=200, fw_pw=2, tile_px=128, gw2=1, nshare=2, chunks=14)),
    # the widest row: ppt escalated to 4, 16 outputs per run, 32 runs
    ("w500", ("f32",), 1, 8, 40, 1, 500, False, G(vec=4, out_ppt=4, out_mo=16, out_px=16, out_per=32, out_last=4, gw2=1)),
    # vec 1, act_ppt 2, out in 2 runs, 11 tiles
    ("v1_w333", ("f32", "bf16"), 1, 8, 8, 2, 333, True, G(vec=1, act_ppt=2, nwg1=2, out_ppt=4, out_per=2, tps=11, last_px=26)),
    # vec 1, hidden 33 -> hidp 48, ppt escalated 1 -> 2, C % 4 != 0
    ("v1_h33_w101", ("f32",), 2, 30, 33, 5, 101, False, G(vec=1, hidp=48, out_ppt=2, out_mo=304, fw_w="gather", act_ppt=1)),
    # H*W = 512: act_ppt 2 exactly at the step
    ("hw512", ("f32",), 1, 8, 8, 16, 32, True, G(vec=4, act_ppt=2, nwg1=1, out_ppt=4, out_per=1)),
    # H*W = 508: act_ppt 1, two runs, last tile 252 px
    ("hw508", ("f32",), 1, 4, 4, 4, 127, False, G(vec=4, act_ppt=1, nwg1=2, tile_px=256, tps=2, last_px=252)),
    # H*W = 2048: act_ppt 4; out in 3 runs; gw2 6 shares over 32 chunks (uneven)
    ("hw2048", ("f32", "f16"), 1, 8, 8, 32, 64, True, G(vec=4, act_ppt=4, nwg1=2, out_per=3, gw2=1, nshare=6, chunks=32, gw_uneven=True)),
    # gw2: 21 chunks in 4 uneven shares, ragged last chunk (16 px)
    ("gw2_ragged", ("f32", "bf16"), 3, 64, 16, 20, 20, False, G(vec=4, gw2=1, nshare=4, chunks=21, gw_uneven=True, gw_last=16, ncb=1)),
    # gw2 with 25 shares; act_ppt 2; out in 2 runs; gx 13 tiles per sample
    ("gw2_s25", ("f32",), 5, 64, 16, 40, 40, False, G(vec=4, gw2=1, nshare=25, chunks=125, act_ppt=2, out_per=2, gx_tps=13)),
    # k_head_stats: 1028 tile partials per channel, so its loop of 4 x 256 loads in flight runs once (vec 1, tile 16 px, 257 tiles per sample)
    ("stats_u4", ("f32",), 4, 4, 72, 17, 241, False, G(vec=1, fw_mw=4, fw_pw=1, tile_px=16, tps=257, nwg=1028, last_px=1, act_ppt=4)),
    # k_head_bwd_fin: 128 run partials per channel, so its loop of 8 x 16 loads in flight runs once (B = 64, two runs per sample)
    ("fin_u8", ("f32",), 64, 4, 4, 7, 73, False, G(vec=1, act_ppt=1, nwg1=128, out_per=1)),
    # C = hidden = 1
    ("c1_h1", ("f32",), 2, 1, 1, 3, 3, False, G(vec=1, hidp=16, cp=16, fw_w="gather", fw_ksteps=1, gx_ksteps=1, ncb=1, clast=1)),
]
SHAPES = {r[0]: r for r in HEAD_NCHW_ROWS}
# (row, dtype, training): every row in training mode in each of its dtypes, then the eval-mode rows
# (row, dtype, training, dL/dlogits): every row in training mode in each of its dtypes, then the eval-mode rows, all under a dL/dlogits
# of uniform size ("flat": every pixel -- the ragged last tile, the short last run, the ragged last chunk -- carries its weight in the
# reductions), and the eval-mode rows once more under the envelope of row_inputs ("env": gx gets elements far below its largest)
CASES = ([(r[0], dt, True, "flat") for r in HEAD_NCHW_ROWS for dt in r[1]] +
         [(r[0], dt, False, g) for g in ("flat", "env") for r in HEAD_NCHW_ROWS if r[7] for dt in r[1]])
CASE_IDS = [f"{n}-{dt}-{'train' if tr else 'eval'}-{g}" for n, dt, tr, g in CASES]


def _waves(mtiles, mtw, K):
    """api_head.hip: head_waves -> (mw as the kernel uses it, remapped from 3, kw, pw)."""
    mw = min(4, -(-mtiles // mtw))
    remap = mw == 3
    if remap:
        mw = 4
    rest = 4 // mw
    kw = rest if K >= 128 else 1
    return mw, remap, kw, rest // kw


def _ksplit(K, kw, grouped):
    """head_gemm_body: K steps of 4 channels (whole groups of 16 in the grouped forms), a wave's share, waves left without a step."""
    ksteps = -(-K // 16) * 4 if grouped else -(-K // 4)
    kper = -(-ksteps // kw)
    if grouped:
        kper = (kper + 3) & ~3
    return ksteps, kper, sum(1 for w in range(kw) if w * kper >= ksteps)


def head_out_max(ppt, W):
    return (K_BLOCK * ppt - 2 * (W + 1) - 3) & ~3


def head_geo(B, C, hid, H, W):
    """One NCHW level called alone, no knobs set; restated by hand (see the module's docstring)."""
    HW = H * W
    g = dict(vec=4 if HW % 4 == 0 else 1, hidp=a16(hid), cp=a16(C))
    vec, hidp, cp = g["vec"], g["hidp"], g["cp"]
    # forward GEMM
    g["fw_mtw"] = 4 if hidp // 16 > 8 else 2
    g["fw_mw"], g["fw_mw3"], g["fw_kw"], g["fw_pw"] = _waves(hidp // 16, g["fw_mtw"], C)
    g["tile_px"] = g["fw_pw"] * 16 * vec
    g["tps"] = -(-HW // g["tile_px"])
    g["nwg"] = B * g["tps"]
    g["last_px"] = HW - (g["tps"] - 1) * g["tile_px"]
    g["fw_mblk"] = -(-(hidp // 16) // (g["fw_mtw"] * g["fw_mw"]))
    g["fw_w"] = "gather" if C % 4 else ("guard" if C % 16 else "perm")
    g["fw_ksteps"], g["fw_kper"], g["fw_kempty"] = _ksplit(C, g["fw_kw"], C % 4 == 0)
    # gx GEMM (MTW 2 always)
    g["gx_mw"], g["gx_mw3"], g["gx_kw"], g["gx_pw"] = _waves(cp // 16, 2, hid)
    g["gx_tile_px"] = g["gx_pw"] * 16 * vec
    g["gx_tps"] = -(-HW // g["gx_tile_px"])
    g["gx_mblk"] = -(-(cp // 16) // (2 * g["gx_mw"]))
    g["gx_ksteps"], g["gx_kper"], g["gx_kempty"] = _ksplit(hid, g["gx_kw"], False)
    g["gx_ksteps_half"], g["gx_kper_half"], g["gx_kempty_half"] = _ksplit(hid, g["gx_kw"], True)
    # k_head_out (head.cuh: head_out_shape)
    ppt = 4 if hid <= 16 else (2 if hid <= 32 else 1)
    while ppt < 4 and head_out_max(ppt, W) < 64:
        ppt *= 2
    mo = head_out_max(ppt, W)
    assert mo >= 4, "rows too wide for k_head_out"
    per = -(-HW // mo)
    opx = (-(-HW // per) + 3) & ~3
    g.update(out_ppt=ppt, out_mo=mo, out_per=per, out_px=opx, out_last=HW - (per - 1) * opx, out_chunks=-(-hid // HEAD_OUT_PAR_CH))
    # k_head_bwd_act
    g["act_ppt"] = 4 if HW >= 2048 else (2 if HW >= 512 else 1)
    g["nwg1"] = B * -(-HW // (K_BLOCK * g["act_ppt"]))
    g["act_hl"] = K_BLOCK * g["act_ppt"] + 2 * (W + 1)
    # dW1
    ncb = -(-C // HEAD_CB)
    per_share = ncb * hidp * HEAD_CB * 4
    gw2 = 1 if vec == 4 and hidp <= 64 else 0
    if gw2:
        nch = -(-HW // HEAD_GW_PX)
        chunks = B * nch
        nshare = max(1, min(max(1, min(512, (4 << 20) // per_share)), chunks // HEAD_GW_DIV))
        empty = 0                                                # share s takes chunks s, s + nshare, ...; nshare <= chunks
        last = HW - (nch - 1) * HEAD_GW_PX
    else:
        nch = -(-HW // (4 * vec))
        chunks = B * nch
        nshare = max(32, min(256, min((4 << 20) // per_share, (chunks + 7) // 8)))
        empty = sum(1 for s in range(nshare) if s * 4 >= chunks)  # share s starts at chunk 4 s + wave
        last = HW - (nch - 1) * 4 * vec
    g.update(ncb=ncb, clast=C - (ncb - 1) * HEAD_CB, gw2=gw2, nshare=nshare, chunks=chunks, gw_empty=empty, gw_uneven=chunks % nshare != 0,
             gw_last=last, gw_passes=-(-(hidp // 16) // 4))
    # head_ctx_layout / head_scratch_layout: floats, each region rounded up to 16 bytes
    ctx = [B * hid * HW, hidp, hidp, hidp * HEAD_PAR, g["nwg"] * 2 * hidp]
    scr = [B * hid * HW, g["nwg1"] * hidp * HEAD_NSTAT, 5 * hidp, ncb * nshare * hidp * HEAD_CB]
    g["ctx_bytes"] = sum(a16(4 * n) for n in ctx)
    g["scratch_bytes"] = sum(a16(4 * n) for n in scr)
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# a row's data
# ---------------------------------------------------------------------------------------------------------------------------
def head_module(C, hid, seed, training=True):
    """A module perturbed as in test_maskhead.test_device_wide_rows_vs_live_oracle (parameters += 0.3 randn), the running statistics
    perturbed too, and the LAST hidden channel nearly dead (BatchNorm weight and bias x 1e-4) when there are several: its activation,
    its row of dW1 and its taps of dW_h are four decades below their neighbours', which a tensor-scale comparison does not see."""
    from mga_yolo_amd import MGAMaskHead
    torch.manual_seed(seed)
    m = MGAMaskHead(C, hid).train()
    g = torch.Generator().manual_seed(seed + 2)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.add_(0.3 * torch.randn(p_.shape, generator=g))
        bn = m.proj[1]
        bn.running_mean.add_(0.2 * torch.randn(hid, generator=g))
        bn.running_var.mul_(0.5 + torch.rand(hid, generator=g))
        if hid > 1:
            bn.weight[-1] *= 1e-4
            bn.bias[-1] *= 1e-4
    return m.train(training)


def row_inputs(B, C, H, W, dt, seed, gkind="flat"):
    """x ~ N(0,1) and dL/dlogits ~ N(0,1), rounded to the row's dtype and returned as fp32.  gkind "env": dL/dlogits under an envelope that
    falls by five decades along each sample's pixels (a loss gradient is nothing like uniform in size): in eval mode gx follows it, so its
    small elements are not hidden behind the large ones; two decades in fp16, which holds nothing below 6e-5 to relative accuracy, as
    gradient or as MFMA operand.  The envelope takes the weight of a sample's last pixels out of every reduction, so no row runs under
    it alone."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    gl = torch.randn(B, 1, H, W, generator=g)
    if gkind == "env":
        decades = 2.0 if dt == "f16" else 5.0
        gl = gl * torch.pow(10.0, -decades * torch.arange(H * W, dtype=torch.float32) / (H * W)).view(1, 1, H, W)
    else:
        assert gkind == "flat", gkind
    return x.to(DT[dt]).float(), gl.to(DT[dt]).float()


def params_of(m):
    bn = m.proj[1]
    return HO.HeadParams.from_state_dict({k: v.detach().clone().float().cpu() for k, v in m.state_dict().items()}, eps=bn.eps, momentum=bn.momentum)


def oracle64(x, gl, p, training):
    """-> (outputs, term magnitudes, forward ctx, g_z), everything fp64."""
    lo, c, mf = HO.forward(x, p, training, double=True)
    go, mb = HO.backward(gl, x, p, c, training, double=True)
    out = dict(logits=lo, running_mean=c.new_running_mean, running_var=c.new_running_var, **{k: go[k] for k in HO_GRADS})
    return out, dict(mf, **mb), c, go["g_z"]


def oracle32(x, gl, p, training):
    lo, c = HO.forward(x, p, training)
    go = HO.backward(gl, x, p, c, training)
    return dict(logits=lo, running_mean=c.new_running_mean, running_var=c.new_running_var, **go)


def oracle_fmt(x, gl, p, training, dt):
    """The fp32 oracle with the roundings the ELEMENT TYPE imposes on a half-precision level, placed where csrc/head.cuh places them: W1
    rounded to the type as operand of the forward MFMA (C % 4 == 0: the 16-byte weight form; the gather form runs fp32 MFMAs), W1 and g_z
    as operands of gx, g_z as operand of dW1 (H*W % 4 == 0: both dW1 kernels; k_head_bwd_gw at vec 1 runs fp32 MFMAs), logits and gx
    stored in the type.  Rounding W1 alone moves z by 2^-9 (bf16) of its terms, and what follows (zhat, SiLU, SiLU') is not bounded by
    that in units of ITS terms -- so the half-precision rows are compared element-wise with this, where the device may differ by
    summation order and by a rounding that falls the other way, and at the tensor scale with the plain fp32 oracle."""
    _, _, H, W = x.shape
    C = x.shape[1]
    lo, c = HO.forward(x, p, training, mma_dtype=DT[dt] if C % 4 == 0 else None)
    go = HO.backward(gl, x, p, c, training, mma_dtype=DT[dt], mma_gw1=(H * W) % 4 == 0)
    go["gx"] = go["gx"].to(DT[dt]).float()
    return dict(logits=lo.to(DT[dt]).float(), running_mean=c.new_running_mean, running_var=c.new_running_var, **go)


# half-precision rows against oracle_fmt: the device sums in another order, so a rounding to the type may fall the other way -- of the
# result, off by one ulp then (at most 2^-10 / 2^-7 of its value in fp16 / bf16), and of MFMA operands, each off by one ulp of its term; value and
# terms are bounded by the magnitude, so two ulps of it
U_BAR_HALF = {"f16": 2.0 ** -9, "bf16": 2.0 ** -6}
HO_GRADS = ("gx", "gw1", "ggamma", "gbeta", "gwh", "gbh")
_cases = {}


def row_case(name, dt="f32", training=True, gkind="flat"):
    """-> the row's module state (a state_dict to load into a fresh MGAMaskHead), inputs (rounded to dt, as fp32), the oracle's outputs
    `want` (fp64 for f32 rows; the fp32 oracle on the rounded inputs for half rows, as everywhere in this suite), for half rows
    `want_fmt` (oracle_fmt) too, and the fp64 term magnitudes `mag` of every output.  Computed once per (row, dtype, mode) and shared: the tensors must not be written to."""
    key = (name, dt, training, gkind)
    if key in _cases:
        return _cases[key]
    _, _, B, C, hid, H, W, _, _ = SHAPES[name]
    m = head_module(C, hid, seed=1000 + C + hid, training=training)
    x, gl = row_inputs(B, C, H, W, dt, 2000 + 7 * C + H, gkind)
    p = params_of(m)
    want, mag, c64, g_z = oracle64(x, gl, p, training)
    want_fmt = None
    if dt != "f32":
        want, want_fmt = oracle32(x, gl, p, training), oracle_fmt(x, gl, p, training, dt)
    case = SimpleNamespace(want_fmt=want_fmt, name=name, dt=dt, dtype=DT[dt], training=training, B=B, C=C, hid=hid, H=H, W=W, x=x, gl=gl, p=p,
                           state={k: v.detach().clone() for k, v in m.state_dict().items()}, want=want, mag=mag, c64=c64, g_z=g_z)
    _cases[key] = case
    return case


def measure_oracle_u():
    """-> {output: (worst u, case id)} of the fp32 oracle at ONE thread against the fp64 oracle over every f32 case of the table: what
    a serial fp32 evaluation of the same sums is off by, in units of the term magnitudes.  DESIGN.md's table and U_ORACLE32 come from it."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    worst = {k: (0.0, "") for k in OUTPUTS}
    try:
        for (name, dt, training, gkind), cid in zip(CASES, CASE_IDS):
            if dt != "f32":
                continue
            c = row_case(name, dt, training, gkind)
            got = oracle32(c.x, c.gl, c.p, training)
            for k in OUTPUTS:
                u = HO.elem_u(got[k], c.want[k], c.mag[k])
                if u > worst[k][0]:
                    worst[k] = (u, cid)
    finally:
        torch.set_num_threads(threads)
    return worst


if __name__ == "__main__":
    for k, (u, cid) in measure_oracle_u().items():
        print(f"{k:13s} {u:.2e}  {cid}")
