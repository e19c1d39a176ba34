"""What tests/test_gpu_eca_nchw.py and tests/test_abi_eca_nchw.py share.  Not a test.

  1. NCHW_ROWS: the shapes at which the NCHW MaskECA kernels (csrc/eca.cuh) are compared element-wise with the fp64 oracle, each with the
     launch geometry it is there for -- in words in its comment and as numbers in its last column.
  2. nchw_geo: a restatement BY HAND of host.cuh's vec_of, choose_tune (pool_tx and chan_tx only) and group_cpt, plus api_eca.hip's
     eca_bwd_smem.  tests/test_abi_eca_nchw.py holds every row's numbers against it on the CPU, so a row that stops covering its branch
     after a tuning change fails there; the restatement itself has to be brought along with host.cuh by hand.
  3. row_case: a row's inputs and its oracle outputs, with the host-side guard that no sample sits on a branch threshold.
"""
from types import SimpleNamespace

import torch

from conftest import rel_err, synth
from oracle import maskeca_oracle as E

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
K_BLOCK = 256                        # common.cuh: kBlock
LDS_PER_WORKGROUP = 64 * 1024
ECA_BWD_STATIC_LDS = 8 * 4           # eca.cuh: k_eca_bwd's red[kEcaBwdRed]


def G(**kw):
    return kw


# Columns: name, dtype, B, C, H, W, k, mask kind, 3-D mask, mask requires grad, tiny_thr, geometry.
# In the comments and the geometry column: vec = elements per lane access (vec_of), TX = pool_tx with rem = (H*W / vec) % TX (a ragged last
# sweep when non-zero), cpt = channels per thread of the sweep kernels (group_cpt), CPB = channels per workgroup = (256 / TX) * cpt with
# crem = C % CPB (the last workgroup's clamped channels), ctx = chan_tx, TY = 256 / ctx channel slices of k_eca_bwd, tiles = ceil(nv / ctx)
# per sample with `last` active lanes in the last one.
NCHW_ROWS = [
    # vec 1, TX 64 ragged (391 % 64 = 7), CPB 4 with C % 4 = 2 (clamped channels), ctx 16, 25 tiles, last tile 7 lanes
    ("v1_tx64_c130", "f32", 3, 130, 23, 17, 3, "mixed", False, True, 1e-4, G(vec=1, tx=64, rem=7, cpt=1, cpb=4, crem=2, ctx=16, tiles=25, last=7)),
    # vec 4, TX 128 ragged (564 % 128 = 52), ctx 16, 36 tiles, last tile 4 lanes
    ("v4_tx128", "f32", 2, 130, 48, 47, 5, "sparse", False, True, 1e-4, G(vec=4, tx=128, rem=52, cpb=2, ctx=16, tiles=36, last=4)),
    # TX 256 ragged (9025 % 256 = 65), CPB 1, ctx 64 through the ">= 4 channels per row" widening (TY 4), 142 tiles, last tile 1 lane, B = 1
    ("v4_tx256_b1", "f32", 1, 16, 190, 190, 5, "randn", False, True, 1e-4, G(vec=4, tx=256, rem=65, cpb=1, ctx=64, ty=4, tiles=142, last=1)),
    # k = 15: all 15 tap roles plus role 15 (dbeta); ctx 16, 33 tiles, last tile 8 lanes
    ("k15_roles", "f32", 2, 256, 40, 52, 15, "mixed", False, True, 1e-4, G(vec=4, tx=128, ctx=16, tiles=33, last=8)),
    # 8-byte half vectors (vec 4 in fp16), raw-probability mask, TX 16, CPB 16 with C % 16 = 4
    ("h4_cpb16", "f16", 2, 260, 20, 13, 5, "prob", False, True, 1e-4, G(vec=4, tx=16, rem=1, cpb=16, crem=4, ctx=16, tiles=5, last=1)),
    # no mask (HAS_MASK false, gmask None), k = 1, TX 8, CPB 32 with C % 32 = 8
    ("nomask_k1", "bf16", 2, 520, 12, 12, 1, "none", False, False, 1e-4, G(vec=4, tx=8, rem=4, cpb=32, crem=8, ctx=16, tiles=3, last=4)),
    # TX 256 ragged (4200 % 256 = 104), 263 tiles, last tile 8 lanes; 3-D mask
    ("bf16_263_tiles", "bf16", 1, 72, 140, 120, 3, "sparse", True, True, 1e-4, G(vec=4, tx=256, rem=104, cpb=1, ctx=16, tiles=263, last=8)),
    # mask without grad: GMASK false; TX 256 ragged (2500 % 256 = 196), 157 tiles, last tile 4 lanes
    ("f16_nograd", "f16", 3, 64, 100, 100, 3, "randn", False, False, 1e-4, G(vec=4, tx=256, rem=196, ctx=16, tiles=157, last=4)),
    # W = 1, vec 1, TX 2, ctx 64 with 9 of its lanes active, C = 3 < TY = 4 (both prefetched slices clamped), use = 0
    ("w1_c3", "f32", 2, 3, 9, 1, 3, "tiny", False, True, 1e-4, G(vec=1, tx=2, rem=1, ctx=64, ty=4, tiles=1, last=9)),
    # ctx 64, TY 4, C = 12 = 3 * TY: one pass of the channel loop after the two prefetched slices; 9 tiles, last tile 13 lanes
    ("w3_ty4", "f32", 5, 12, 700, 3, 5, "all_negative", False, True, 1e-4, G(vec=4, tx=128, rem=13, ctx=64, ty=4, tiles=9, last=13)),
    # k = 15 > C = 7; TY 4 < C < 2 * TY: the second prefetched slice is clamped for ty = 3; B = 11 (XCD padding ids); 3-D mask
    ("k_gt_c_b11", "f32", 11, 7, 30, 31, 15, "mixed", True, True, 1e-4, G(vec=1, tx=128, rem=34, cpb=2, crem=1, ctx=64, ty=4, tiles=15, last=34)),
    # vec 1 with TX 256, ragged (1517 % 256 = 237); raw-probability mask in fp32
    ("v1_tx256_prob", "f32", 9, 20, 37, 41, 15, "prob", False, True, 1e-4, G(vec=1, tx=256, rem=237, cpb=1, ctx=64, ty=4, tiles=24, last=45)),
    # the scalar 2-byte path (vec 1 in bf16), ctx 32 (TY 8), TX 8, CPB 32 with C % 32 = 1, 2 tiles, last tile 3 lanes
    ("bf16_scalar_k9", "bf16", 13, 33, 5, 7, 9, "mixed", False, True, 1e-4, G(vec=1, tx=8, rem=3, cpb=32, crem=1, ctx=32, ty=8, tiles=2, last=3)),
    # the same geometry in fp16
    ("f16_scalar_k7", "f16", 13, 33, 5, 7, 7, "randn", False, True, 1e-4, G(vec=1, tx=8, rem=3, cpb=32, crem=1, ctx=32, ty=8, tiles=2, last=3)),
    # cpt 2 chosen by group_cpt (16 * ceil(770 / 8) = 1552 >= 1536), CPB 8 with C % 8 = 2; 50 MB
    ("cpt2_c770", "f32", 16, 770, 32, 32, 5, "randn", False, True, 1e-4, G(vec=4, tx=64, rem=0, cpt=2, cpb=8, crem=2, ctx=16, tiles=16)),
    # cpt 2 at TX 256: CPB 2 with C odd (8 * ceil(401 / 2) = 1608 >= 1536); 53 MB
    ("cpt2_tx256", "f32", 8, 401, 64, 64, 5, "sparse", False, True, 1e-4, G(vec=4, tx=256, rem=0, cpt=2, cpb=2, crem=1, ctx=16, tiles=64)),
    # ctx 64 kept by the grid size (32 * 25 tiles = 800 >= 768), TY 4, C = 10 * TY; 33 MB
    ("ctx64_by_grid", "f32", 32, 40, 80, 80, 3, "randn", False, True, 1e-4, G(vec=4, tx=256, rem=64, cpt=1, cpb=1, ctx=64, ty=4, tiles=25, last=64)),
    # nv = 1, TX 1, ctx 1, TY 256, k_eca_bwd's LDS 64 096 B: near the widest C the backward's LDS takes (test_abi_eca_nchw.py: the limit)
    ("c5000_lds", "f32", 1, 5000, 2, 2, 7, "randn", False, True, 1e-4, G(vec=4, nv=1, tx=1, ctx=1, ty=256, tiles=1, last=1, lds=64096)),
    # one element
    ("one_element", "f32", 1, 1, 1, 1, 3, "randn", False, True, 1e-4, G(vec=1, nv=1, tx=1, cpb=256, ctx=64, ty=4, tiles=1, last=1)),
    # two channels of three pixels
    ("c2_w3", "f32", 4, 2, 1, 3, 3, "randn", False, True, 1e-4, G(vec=1, nv=3, tx=1, cpb=256, ctx=64, ty=4, tiles=1, last=3)),
    # tiny_thr = 0: use = 1 with S = 144 * sigmoid(-20) < eps, so live = 0 (no K_b term in dL/dmask) and den = eps
    ("live0", "f32", 2, 40, 12, 12, 3, "tiny", False, True, 0.0, G(vec=4, tx=8, rem=4, cpb=32, crem=8, ctx=32, ty=8, tiles=2, last=4)),
]
ROW_IDS = [r[0] for r in NCHW_ROWS]
KNOB_ROWS = [NCHW_ROWS[i - 1][0] for i in (1, 5, 9, 11, 13)]        # the rows the forced launch geometries run: fp32, fp16 and bf16


def _pow2_floor(v):
    return 1 << (v.bit_length() - 1)


def _pow2_ceil(v):
    return 1 << (v - 1).bit_length() if v > 1 else 1


def nchw_geo(B, C, H, W):
    """host.cuh's vec_of, choose_tune (pool_tx, chan_tx) and group_cpt for one NCHW level called alone, no knobs set; restated by hand."""
    HW = H * W
    vec = 4 if HW % 4 == 0 else 1                                    # vec_of
    nv = HW // vec
    tx = min(_pow2_floor(max(nv // 4, 1)), 256)                      # choose_tune: pool_tx
    ctx = min(_pow2_ceil(nv), 64)                                    # choose_tune: chan_tx
    while ctx > 16 and B * -(-nv // ctx) < 768:
        ctx //= 2
    while ctx < 64 and (K_BLOCK // ctx) * 4 > C:
        ctx *= 2
    cpt = 2 if B * -(-C // ((K_BLOCK // tx) * 2)) >= 1536 else 1     # group_cpt (max_cpt = 2)
    cpb = (K_BLOCK // tx) * cpt
    tiles = -(-nv // ctx)                                            # chan_tiles
    return dict(vec=vec, nv=nv, tx=tx, rem=nv % tx, cpt=cpt, cpb=cpb, crem=C % cpb, ctx=ctx, ty=K_BLOCK // ctx, tiles=tiles,
                last=nv - (tiles - 1) * ctx, lds=(3 * C + K_BLOCK * vec) * 4)           # eca_bwd_smem


def nchw_max_c():
    """api_eca.hip's kEcaNchwMaxC: the widest C whose eca_bwd_smem at vec 4 plus k_eca_bwd's static LDS is at most 64 KB."""
    return (LDS_PER_WORKGROUP - ECA_BWD_STATIC_LDS - K_BLOCK * 4 * 4) // (3 * 4)


def eca_params(k, seed):
    g = torch.Generator().manual_seed(seed)
    return E.EcaParams(0.6 * torch.randn(1, 1, k, generator=g), torch.tensor(0.4))


def assert_off_thresholds(name, mask, use_sig, tiny_thr, eps, N):
    """fp32 and fp64 must take the same branches: no sample's S / N within 1e-3 (relative) of tiny_thr, no S within 1e-3 of eps."""
    if mask is None:
        return
    m = mask.double().reshape(mask.shape[0], -1)
    S = (m.sigmoid() if use_sig else m).sum(dim=1)
    assert bool(((S / N - tiny_thr).abs() > 1e-3 * tiny_thr).all()), f"{name}: a sample's S/N sits on tiny_thr; change the seed"
    assert bool(((S - eps).abs() > 1e-3 * eps).all()), f"{name}: a sample's S sits on eps; change the seed"


def oracle(x, mask, gy, p, use_sig, double, tiny_thr=1e-4, eps=1e-6):
    """The hand-derived oracle (forward + backward) in fp64, or in fp32 (the half-precision rows: on the rounded inputs)."""
    cast = (lambda t: None if t is None else t.double()) if double else (lambda t: t)
    pp = E.EcaParams(cast(p.w), cast(p.beta))
    cfg = E.EcaConfig(use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=eps)
    y_o, t = E.forward(cast(x), cast(mask), pp, cfg)
    return y_o, E.backward(cast(gy), cast(x), cast(mask), pp, cfg, t)


def autograd_oracle(x, mask, gy, p, use_sig, tiny_thr=1e-4, eps=1e-6):
    """fp64 autograd of the eager-op form: shares no derivation with the kernels."""
    pp = E.EcaParams(p.w.double(), p.beta.double())
    cfg = E.EcaConfig(use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=eps)
    return E.reference_form_step(x.double(), None if mask is None else mask.double(), pp, cfg, gy.double())


_cases = {}


def row_case(name):
    """-> the row's inputs (x / gy already rounded to its dtype, as fp32), parameters and oracle outputs.  The rows that several tests run
    (KNOB_ROWS, all small) are computed once and shared: their tensors must not be written to."""
    if name in _cases:
        return _cases[name]
    row = NCHW_ROWS[ROW_IDS.index(name)]
    _, dt, B, C, H, W, k, kind, mask3d, mask_grad, tiny_thr, _ = row
    x, mask, gy = synth(B, C, H, W, seed=300 + C + H, mask_kind=kind, mask3d=mask3d)
    use_sig = kind != "prob"
    p = eca_params(k, seed=C)
    if dt != "f32":
        x, gy = x.to(DT[dt]).float(), gy.to(DT[dt]).float()
    assert_off_thresholds(name, mask, use_sig, tiny_thr, 1e-6, H * W)
    y_o, g_o = oracle(x, mask, gy, p, use_sig, dt == "f32", tiny_thr)
    if tiny_thr == 0.0:
        # use = 1 with S < eps: the hand-derived backward's `live` term shares its derivation with the kernel, so the oracle of this row is
        # fp64 autograd of the eager-op form, and the two oracles must agree (1e-9: fp64 rounding of sums of 144 * 40 terms, with margin)
        assert dt == "f32" and bool((mask.double().sigmoid().reshape(B, -1).sum(dim=1) < 1e-6).all()), name
        y_a, g_a = autograd_oracle(x, mask, gy, p, use_sig, tiny_thr)
        assert rel_err(y_o, y_a) < 1e-9, name
        for key in ("gx", "gmask", "gw", "gbeta"):
            assert g_o[key].shape == g_a[key].shape and rel_err(g_o[key], g_a[key]) < 1e-9, (name, key)
        y_o, g_o = y_a, g_a
    case = SimpleNamespace(name=name, dt=dt, dtype=DT[dt], x=x, mask=mask, gy=gy, p=p, use_sig=use_sig, mask_grad=mask_grad, tiny_thr=tiny_thr,
                           eps=1e-6, y_o=y_o, g_o=g_o)
    if name in KNOB_ROWS:
        _cases[name] = case
    return case
