"""GPU tests (-m gpu) of the channels-last MaskCBAM kernels at the corners of their tiling (host.cuh nhwc_geo): lanes of 1 / 4 / 8
channels, 4..64 lanes per pixel with several channel-group passes (nj), several tiles per chunk (rp) with a ragged last chunk, partial
64-channel fold blocks, tiles that span many image rows or sit inside one, every mask kind and run-time conv sizes -- against the fp64
oracle element by element.  Then exact ties of both arg-maxes (masked max over pixels, channel max over lanes), which must go to the
first index, and two layout rows.  tests/test_abi_nhwc.py checks on the CPU that EDGE_ROWS reach every branch they claim to."""
import pytest
import torch

from conftest import elem_err, rel_err, synth
from oracle import maskcbam_oracle as O

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_TOL = {"f16": 4e-3, "bf16": 3e-2}

# name, dtype, B, C, H, W, k, mask kind, 3-D mask, mask requires grad        geometry (nhwc_geo) in the comment
EDGE_ROWS = [
    ("v1_nj3_fold", "f32", 3, 130, 23, 17, 3, "mixed", False, True),          # vec 1, cs 64, nj 3, ncb 3 (last block 2 channels)
    ("v1_rp2", "f32", 2, 130, 48, 47, 9, "sparse", False, True),              # vec 1, 71 tiles of 32 px, rp 2, 36 chunks (ragged)
    ("v4_cs4_rp2", "f32", 1, 16, 190, 190, 5, "randn", False, True),          # vec 4, cs 4, tiles of 512 px, 71 tiles, rp 2 (ragged)
    ("v4_cs64_rp2", "f32", 2, 256, 40, 52, 15, "mixed", False, True),         # vec 4, cs 64, 65 tiles, rp 2, 33 chunks (ragged)
    ("h4_nj2", "f16", 2, 260, 20, 13, 7, "prob", False, True),                # vec 4 in half precision, cs 64, nj 2; raw-probability mask
    ("v8_nj2_fold", "bf16", 2, 520, 12, 12, 1, "none", False, False),         # vec 8, cs 64, nj 2, ncb 9 (last block 8 channels); k = 1
    ("v8_rp5", "bf16", 1, 72, 140, 120, 9, "sparse", True, True),             # vec 8, cs 16, 263 tiles of 64 px, rp 5 (ragged); 3-D mask
    ("v8_rp2_nograd", "f16", 3, 64, 100, 100, 3, "randn", False, False),      # vec 8, cs 8, 79 tiles, rp 2 (ragged); mask without grad
    ("w1", "f32", 2, 3, 9, 1, 3, "tiny", False, True),                        # W = 1, vec 1, cs 4; use = 0
    ("w3_cs4", "f32", 5, 12, 700, 3, 5, "all_negative", False, True),        # vec 4, cs 4: a 512-pixel tile spans ~170 rows; GAP fallback
    ("w100", "f32", 2, 256, 3, 100, 9, "randn", False, False),                # W = 100 > 32-pixel tiles; mask without grad
    ("v1_b11", "f32", 11, 7, 30, 31, 15, "mixed", True, True),               # vec 1, cs 4, B = 11; 3-D mask, mixed batch
    ("h1_f16", "f16", 3, 7, 33, 35, 1, "all_negative", False, True),         # vec 1 in half precision
    ("prob_f32", "f32", 9, 20, 37, 41, 15, "prob", False, True),             # vec 4, cs 8; raw-probability mask in fp32
]


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


def _is_cl(t):
    return t.is_contiguous(memory_format=CL) and not t.is_contiguous()


def _params(C, k, seed):
    p = O.Params.default_init(C, k=k, seed=seed)
    with torch.no_grad():
        for t in (p.w1, p.b1, p.w2, p.b2):
            t.add_(0.3 * torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)))
        p.wsa.mul_(3.0)
        p.beta.fill_(0.4)
    return p


def _run(F, x, mask, gy, p, k, use_sig, dtype, mask_grad=True, fmt=CL):
    xd = x.cuda().to(dtype).to(memory_format=fmt).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(mask_grad)
    ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    y = F.mask_cbam(xd, md, *ps, F.BlockConfig(hidden=p.w1.shape[0], k=k, use_sigmoid_mask=use_sig))
    y.backward(gy.cuda().to(dtype).to(memory_format=fmt))
    torch.cuda.synchronize()
    g = dict(gx=xd.grad, gmask=md.grad if (md is not None and mask_grad) else None, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad,
             gb2=ps[3].grad, gwsa=ps[4].grad, gbeta=ps[5].grad)
    return y.detach(), g


def _oracle(x, mask, gy, p, use_sig, double):
    """(y, grads, ctx) of the oracle, in fp64 when `double` (inputs and parameters promoted), else in fp32."""
    cast = (lambda t: None if t is None else t.double()) if double else (lambda t: t)
    pp = p.to(torch.float64) if double else p
    cfg = O.Config(use_sigmoid_mask=use_sig)
    y_o, c = O.forward(cast(x), cast(mask), pp, cfg)
    return y_o, O.backward(cast(gy), cast(x), cast(mask), pp, cfg, c), c


def _near_tie_pixels(x, c, B, C, H, W):
    """(B, H*W) pixels whose channel arg-max is decided by less than fp32 rounding of ca (top-2 of x_c ca_c within 1e-6 relative, not
    exactly equal): the device's ca differs from the oracle's by ~1e-7, so there the routed sub-gradient may take either channel."""
    if C < 2:
        return torch.zeros(B, H * W, dtype=torch.bool)
    u = (x.double().reshape(B, C, H * W) * c.ca.double().reshape(B, C, 1))
    top = u.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    return (gap > 0) & (gap <= 1e-6 * top[:, 0].abs())


def _check(name, dtype, y, g, y_o, g_o, gy, x, skip_px):
    """fp32: 1e-4 relative on every output, 1e-3 element-wise on y / gx / gmask, parameter gradients 1e-4 of their scale plus the fuzzers'
    absolute floor (1e-7 |gy| |x|: fp32 rounding of a cancelling sum's terms).  Half precision: the same forms at 4e-3 / 3e-2."""
    tol = 1e-4 if dtype == "f32" else HALF_TOL[dtype]
    floor = 1e-7 * float(gy.double().norm() * x.double().norm())
    report = []
    gx_got, gx_want = g["gx"].float().cpu().double(), g_o["gx"].double()
    if skip_px is not None and bool(skip_px.any()):
        keep = ~skip_px.reshape(skip_px.shape[0], 1, *gx_want.shape[2:])
        gx_got, gx_want = gx_got * keep, gx_want * keep
    for k, got, want in (("y", y.float(), y_o), ("gx", gx_got, gx_want), ("gmask", g["gmask"], g_o["gmask"])):
        if got is None:
            continue
        if not rel_err(got, want) < tol:
            report.append(f"{k} {rel_err(got, want):.3e}")
        if dtype == "f32" and not elem_err(got, want) < 1e-3:
            report.append(f"{k} element-wise {elem_err(got, want):.3e}")
    for k in ("gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta"):
        want = g_o[k].double()
        d = float((g[k].detach().double().cpu() - want).abs().max())
        if not d <= tol * float(want.abs().max()) + floor:
            report.append(f"{k} |diff| {d:.3e} over {tol * float(want.abs().max()) + floor:.3e}")
    assert not report, f"{name}: " + "; ".join(report)


@pytest.mark.parametrize("row", EDGE_ROWS, ids=[r[0] for r in EDGE_ROWS])
def test_channels_last_geometry_corner_vs_oracle(F, row):
    name, dt, B, C, H, W, k, kind, mask3d, mask_grad = row
    dtype = DT[dt]
    x, mask, gy = synth(B, C, H, W, seed=300 + C + H, mask_kind=kind, mask3d=mask3d)
    use_sig = kind != "prob"
    p = _params(C, k, seed=C)
    if dt != "f32":
        x, gy = x.to(dtype).float(), gy.to(dtype).float()
    y_o, g_o, c = _oracle(x, mask, gy, p, use_sig, double=dt == "f32")
    y, g = _run(F, x, mask, gy, p, k, use_sig, dtype, mask_grad)
    assert y.dtype == dtype and g["gx"].dtype == dtype
    assert _is_cl(y) and _is_cl(g["gx"]), f"{name}: y / gx came back in another layout"
    assert (g["gmask"] is None) == (mask is None or not mask_grad)
    skip = _near_tie_pixels(x, c, B, C, H, W)
    assert int(skip.sum()) <= 4, f"{name}: {int(skip.sum())} channel arg-max near-ties"
    _check(name, dt, y, g, y_o, g_o, gy, x, skip)


# ---------------------------------------------------------------------------------------------------------------------------
# exact ties: no tolerance.  Both layouts (the NCHW path for free).
# ---------------------------------------------------------------------------------------------------------------------------
# masked max over pixels: integer-valued x (9 distinct values), so every channel's maximum sits at many pixels -- in different tiles,
# chunks and waves of k_pool_fin's combine at these rp >= 2 shapes; amax must be the first of them
POOL_TIE_ROWS = [("f32", 1, 16, 190, 190, "randn"), ("f32", 2, 130, 48, 47, "mixed"), ("f32", 2, 256, 40, 52, "none"),
                 ("bf16", 1, 72, 140, 120, "sparse")]


def _integer_x(B, C, H, W, seed):
    return torch.randint(-4, 5, (B, C, H, W), generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("fmt", [CL, torch.contiguous_format], ids=["channels_last", "nchw"])
@pytest.mark.parametrize("dt,B,C,H,W,kind", POOL_TIE_ROWS)
def test_masked_max_ties_go_to_the_first_pixel(F, dt, B, C, H, W, kind, fmt):
    dtype = DT[dt]
    _, mask, gy = synth(B, C, H, W, seed=17, mask_kind=kind)
    x = _integer_x(B, C, H, W, seed=C + H)
    p = O.Params.default_init(C, seed=4)               # unperturbed: no ca saturates to 1.0 in fp32, where equal x would tie in u as well
    if dt != "f32":
        gy = gy.to(dtype).float()
    y_o, g_o, c = _oracle(x, mask, gy, p, True, double=True)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    _, v = F.forward_with_ctx(x.cuda().to(dtype).to(memory_format=fmt), None if mask is None else mask.cuda(), ps,
                              F.BlockConfig(hidden=p.w1.shape[0]))
    torch.cuda.synchronize()
    valid = v["valid"].cpu().bool()
    assert torch.equal(valid, c.valid)
    assert bool(valid.any())
    got, want = v["amax"].cpu().long(), c.amax.long()
    assert torch.equal(got[valid], want[valid]), f"{int((got != want)[valid].sum())} channels with another arg-max"
    y, g = _run(F, x, mask, gy, p, 7, True, dtype, fmt=fmt)
    skip = _near_tie_pixels(x, c, B, C, H, W)
    assert int(skip.sum()) <= 4
    _check(f"{dt} {B}x{C}x{H}x{W}", dt, y, g, y_o, g_o, gy, x, skip)


# channel max over lanes: at every third pixel channels [0, j0) are -1 and channels [j0, C) are 0 (j0 cycles through 0..C-1), so the
# maximum, 0, is shared by C - j0 channels that sit in different lanes and channel-group passes; cidx must be j0 exactly
CHAN_TIE_ROWS = [("f32", 2, 130, 23, 17), ("f32", 2, 260, 20, 13), ("f16", 2, 260, 20, 13), ("bf16", 2, 520, 12, 12),
                 ("f32", 3, 7, 9, 11)]


@pytest.mark.parametrize("fmt", [CL, torch.contiguous_format], ids=["channels_last", "nchw"])
@pytest.mark.parametrize("dt,B,C,H,W", CHAN_TIE_ROWS)
def test_channel_max_ties_go_to_the_first_channel(F, dt, B, C, H, W, fmt):
    dtype = DT[dt]
    x, mask, _ = synth(B, C, H, W, seed=23)
    x = x.to(dtype).float()
    xf = x.view(B, C, H * W)
    px = torch.arange(0, H * W, 3)
    j0 = (px * 7 + 3) % C
    for b in range(B):
        for q, j in zip(px.tolist(), j0.tolist()):
            xf[b, :j, q] = -1.0
            xf[b, j:, q] = 0.0
    p = _params(C, 7, seed=6)
    _, _, c = _oracle(x, mask, torch.zeros_like(x), p, True, double=True)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    _, v = F.forward_with_ctx(x.cuda().to(dtype).to(memory_format=fmt), mask.cuda(), ps, F.BlockConfig(hidden=p.w1.shape[0]))
    torch.cuda.synchronize()
    got = v["cidx"].cpu().long()
    assert torch.equal(c.cidx[:, px].long(), j0.expand(B, -1))
    assert torch.equal(got[:, px], j0.expand(B, -1)), f"{int((got[:, px] != j0).sum())} tied pixels with another channel"
    other = torch.ones(H * W, dtype=torch.bool)
    other[px] = False
    differ = (got != c.cidx.long()) & other & ~_near_tie_pixels(x, c, B, C, H, W)
    assert not bool(differ.any()), int(differ.sum())


# ---------------------------------------------------------------------------------------------------------------------------
# layout rows
# ---------------------------------------------------------------------------------------------------------------------------
def _level(F, x, mask, ps, cfg, gy):
    xl = x.detach().requires_grad_(True)                                 # (a view keeps its storage offset)
    ml = mask.detach().clone().requires_grad_(True)
    pl = [t.detach().clone().requires_grad_(True) for t in ps]
    y = F.mask_cbam(xl, ml, *pl, cfg)
    y.backward(gy)
    torch.cuda.synchronize()
    return [y.detach(), xl.grad, ml.grad] + [t.grad for t in pl]


def test_batch_sliced_channels_last_view_equals_a_fresh_copy(F):
    B, C, H, W = 6, 64, 20, 20
    x, mask, gy = synth(B, C, H, W, seed=51, mask_kind="mixed")
    p = _params(C, 7, seed=8)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0])
    xd, gd, md = x.cuda().to(memory_format=CL), gy.cuda().to(memory_format=CL), mask.cuda()
    xv, gv = xd[2:5].detach(), gd[2:5]
    assert xv.storage_offset() > 0 and _is_cl(xv) and _is_cl(gv)
    view = _level(F, xv, md[2:5], ps, cfg, gv)
    fresh = _level(F, xv.clone(memory_format=CL), md[2:5].clone(), ps, cfg, gv.clone(memory_format=CL))
    assert _is_cl(view[0]) and _is_cl(view[1])
    for i, (a, b) in enumerate(zip(view, fresh)):
        assert torch.equal(a, b), i


def test_nchw_gy_for_a_channels_last_level_equals_a_channels_last_gy(F):
    B, C, H, W = 3, 48, 17, 19
    x, mask, gy = synth(B, C, H, W, seed=52, mask_kind="sparse")
    p = _params(C, 5, seed=9)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0], k=5)
    xd, md = x.cuda().to(memory_format=CL), mask.cuda()
    a = _level(F, xd.clone(memory_format=CL), md, ps, cfg, gy.cuda().contiguous())
    b = _level(F, xd.clone(memory_format=CL), md, ps, cfg, gy.cuda().to(memory_format=CL))
    assert _is_cl(a[0]) and _is_cl(a[1])
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
