"""GPU tests (-m gpu) of the channels-last MaskECA path (csrc/eca_nhwc.cuh, MGACBAM_LAYOUT_NHWC on the ECA levels): the reference goldens
and the live-oracle shapes of tests/test_oracle_eca.py fed channels_last, half precision, the tiling corners of host.cuh's nhwc_geo
against the fp64 oracle element by element (tests/test_abi_eca_nhwc.py checks on the CPU that ECA_EDGE_ROWS reach the branches their
comments claim), bit-identity across repeats / batch composition / call composition / layouts of the NCHW path, a copy-free step, the
static plan and a small AMP model."""
import pytest
import torch

from conftest import elem_err, rel_err, synth
from oracle import maskeca_oracle as E
from test_oracle_eca import ECA_CASES, load_eca

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_TOL = {"f16": 4e-3, "bf16": 3e-2}        # tests/test_gpu_channels_last_edges.py
TOL = 1e-4                                     # test_gpu_matches_reference_golden / test_gpu_vs_oracle_live

# The (dtype, B, C, H, W), mask kind, 3-D mask and mask-gradient columns are those of test_gpu_channels_last_edges.EDGE_ROWS (the rows the
# MaskECA kernels share a geometry with); k is the conv1d size over the channel axis (odd, 1..15).
# name, dtype, B, C, H, W, k, mask kind, 3-D mask, mask requires grad            geometry (nhwc_geo) in the comment
ECA_EDGE_ROWS = [
    ("v1_nj3_fold", "f32", 3, 130, 23, 17, 3, "mixed", False, True),          # vec 1, cs 64, nj 3, 3 fold blocks (the last: 2 channels)
    ("v1_rp2", "f32", 2, 130, 48, 47, 5, "sparse", False, True),              # vec 1, 71 tiles of 32 px, rp 2, 36 chunks (ragged)
    ("v4_cs4_rp2", "f32", 1, 16, 190, 190, 5, "randn", False, True),          # vec 4, cs 4, tiles of 512 px, 71 tiles, rp 2 (ragged)
    ("v4_cs64_rp2", "f32", 2, 256, 40, 52, 15, "mixed", False, True),         # vec 4, cs 64, 65 tiles, rp 2, 33 chunks (ragged)
    ("h4_nj2", "f16", 2, 260, 20, 13, 5, "prob", False, True),                # vec 4 in half precision, cs 64, nj 2; raw-probability mask
    ("v8_nj2_fold", "bf16", 2, 520, 12, 12, 1, "none", False, False),         # vec 8, cs 64, nj 2, 9 fold blocks (the last: 8 channels); k = 1
    ("v8_rp5", "bf16", 1, 72, 140, 120, 3, "sparse", True, True),             # vec 8, cs 16, 263 tiles of 64 px, rp 5 (ragged); 3-D mask
    ("v8_rp2_nograd", "f16", 3, 64, 100, 100, 3, "randn", False, False),      # vec 8, cs 8, 79 tiles, rp 2 (ragged); mask without grad
    ("w1", "f32", 2, 3, 9, 1, 3, "tiny", False, True),                        # W = 1, vec 1, cs 4; use = 0; C = 3 with k = 3
    ("w3_cs4", "f32", 5, 12, 700, 3, 5, "all_negative", False, True),         # vec 4, cs 4: 5 tiles of 512 px
    ("v1_b11", "f32", 11, 7, 30, 31, 15, "mixed", True, True),                # vec 1, cs 4, B = 11; 3-D mask; taps wider than the channel axis
    ("prob_f32", "f32", 9, 20, 37, 41, 15, "prob", False, True),              # vec 4, cs 8; raw-probability mask in fp32
]


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


def _is_cl(t):
    return t.is_contiguous(memory_format=CL) and not t.is_contiguous()


def _eca_params(C, k, seed):
    g = torch.Generator().manual_seed(seed)
    return E.EcaParams(0.6 * torch.randn(1, 1, k, generator=g), torch.tensor(0.4))


def _run(F, x, mask, gy, p, use_sig=True, dtype=torch.float32, mask_grad=True, fmt=CL, tiny_thr=1e-4, eps=1e-6):
    """-> (y, dict(gx, gmask, gw, gbeta)) of mask_eca on the device; x / gy in `fmt`."""
    xd = x.cuda().to(dtype).to(memory_format=fmt).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(mask_grad)
    w, beta = p.w.cuda().requires_grad_(True), p.beta.cuda().requires_grad_(True)
    y = F.mask_eca(xd, md, w, beta, F.EcaConfig(k=p.w.shape[-1], use_sigmoid_mask=use_sig, tiny_thr=tiny_thr, eps=eps))
    y.backward(gy.cuda().to(dtype).to(memory_format=fmt))
    torch.cuda.synchronize()
    return y.detach(), dict(gx=xd.grad, gmask=md.grad if (md is not None and mask_grad) else None, gw=w.grad, gbeta=beta.grad)


def _oracle(x, mask, gy, p, use_sig, double):
    cast = (lambda t: None if t is None else t.double()) if double else (lambda t: t)
    pp = E.EcaParams(cast(p.w), cast(p.beta))
    cfg = E.EcaConfig(use_sigmoid_mask=use_sig)
    y_o, t = E.forward(cast(x), cast(mask), pp, cfg)
    return y_o, E.backward(cast(gy), cast(x), cast(mask), pp, cfg, t)


def _expect_layout(x, *ts):
    B, C, H, W = x.shape
    if C > 1 and H * W > 1:
        for t in ts:
            assert _is_cl(t), "y / gx came back in another layout"


# ---------------------------------------------------------------------------------------------------------------------------
# the reference goldens and the live-oracle shapes, channels_last
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ECA_CASES)
def test_goldens_channels_last(F, name):
    d = load_eca(name)
    p = E.EcaParams(d["params"]["conv1d.weight"], d["params"]["beta"])
    assert p.w.shape[-1] == d["meta"]["k"]
    y, g = _run(F, d["x"], d["mask"], d["gy"], p, use_sig=d["meta"]["use_sigmoid_mask"], tiny_thr=d["meta"]["tiny_thr"], eps=d["meta"]["eps"])
    _expect_layout(d["x"], y, g["gx"])
    rep = []
    for nm, got in (("y", y), ("gx", g["gx"]), ("gw", g["gw"]), ("gbeta", g["gbeta"])) + ((("gmask", g["gmask"]),) if d["mask"] is not None else ()):
        want = d["out"][nm]
        assert got.shape == want.shape, nm
        e = rel_err(got, want)
        print(f"{name} {nm} rel_err {e:.3e}")
        if not e < TOL:
            rep.append(f"{nm} {e:.3e}")
    assert not rep, f"{name}: " + "; ".join(rep)


LIVE_SHAPES = [((32, 64, 80, 80), "sparse"), ((32, 256, 20, 20), "randn"), ((3, 48, 17, 17), "mixed"), ((2, 512, 40, 40), "mixed"),
               ((1, 1024, 10, 10), "randn"), ((5, 8, 3, 5), "randn")]          # test_gpu_vs_oracle_live


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape,mask_kind", LIVE_SHAPES)
def test_live_oracle_channels_last(F, shape, mask_kind, with_mask):
    from mga_yolo_amd import MaskECA
    B, C, H, W = shape
    if mask_kind == "mixed" and B < 2:
        mask_kind = "randn"
    x, mask, gy = synth(B, C, H, W, seed=31, mask_kind=mask_kind)
    if not with_mask:
        mask = None
    torch.manual_seed(1)
    m = MaskECA(C)
    with torch.no_grad():
        m.beta.fill_(0.4)
    p = E.EcaParams(m.conv1d.weight.detach().clone(), m.beta.detach().clone())
    y_o, t = E.forward(x, mask, p)
    g_o = E.backward(gy, x, mask, p, E.EcaConfig(), t)
    m.cuda()
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(True)
    y = m(xd if md is None else [xd, md])
    y.backward(gy.cuda().to(memory_format=CL))
    _expect_layout(x, y, xd.grad)
    got = dict(y=y, gx=xd.grad, gw=m.conv1d.weight.grad, gbeta=m.beta.grad, gmask=None if md is None else md.grad)
    want = dict(g_o, y=y_o)
    rep = []
    for k in ("y", "gx", "gw", "gbeta", "gmask"):
        if want[k] is None:
            assert got[k] is None
            continue
        e = rel_err(got[k], want[k])
        print(f"{shape} {k} rel_err {e:.3e}")
        if not e < TOL:
            rep.append(f"{k} {e:.3e}")
    assert not rep, "; ".join(rep)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("C,hw", [(64, (40, 40)), (192, (20, 20)), (256, (20, 20)), (520, (10, 12)), (260, (10, 12))])
def test_half_precision_channels_last(F, C, hw, dt):
    """cfg2 / configs[4] widths and 520 (all multiples of 8: 8-element lanes, one and two channel passes) and 260 (4-element lanes in half
    precision), against the fp32 oracle on the rounded inputs."""
    dtype, tol = DT[dt], HALF_TOL[dt]
    B, (H, W) = 4, hw
    x, mask, gy = synth(B, C, H, W, seed=21)
    x, gy = x.to(dtype).float(), gy.to(dtype).float()
    p = _eca_params(C, E.eca_kernel_size(C), seed=C)
    y_o, g_o = _oracle(x, mask, gy, p, True, double=False)
    y, g = _run(F, x, mask, gy, p, dtype=dtype)
    assert y.dtype == dtype and g["gx"].dtype == dtype and _is_cl(y) and _is_cl(g["gx"])
    for k, got, want in (("y", y.float(), y_o), ("gx", g["gx"].float(), g_o["gx"]), ("gmask", g["gmask"], g_o["gmask"]), ("gw", g["gw"], g_o["gw"]),
                         ("gbeta", g["gbeta"], g_o["gbeta"])):
        e = rel_err(got, want)
        print(f"{dt} C={C} {k} rel_err {e:.3e}")
        assert e < tol, k


# ---------------------------------------------------------------------------------------------------------------------------
# tiling corners against the fp64 oracle, element-wise
# ---------------------------------------------------------------------------------------------------------------------------
def _check(name, dt, y, g, y_o, g_o, gy, x):
    """The bars of test_gpu_channels_last_edges._check: fp32 1e-4 relative on every output and 1e-3 element-wise on y / gx / gmask, the
    parameter gradients 1e-4 of their scale plus the fuzzers' absolute floor (1e-7 |gy| |x|: fp32 rounding of a cancelling sum's terms).
    Half precision: the same forms at 4e-3 / 3e-2."""
    tol = TOL if dt == "f32" else HALF_TOL[dt]
    floor = 1e-7 * float(gy.double().norm() * x.double().norm())
    report = []
    for k, got, want in (("y", y.float(), y_o), ("gx", g["gx"].float(), g_o["gx"]), ("gmask", g["gmask"], g_o["gmask"])):
        if got is None:
            continue
        e = rel_err(got, want)
        print(f"{name} {k} rel_err {e:.3e} elem_err {elem_err(got, want):.3e}")
        if not e < tol:
            report.append(f"{k} {e:.3e}")
        if dt == "f32" and not elem_err(got, want) < 1e-3:
            report.append(f"{k} element-wise {elem_err(got, want):.3e}")
    for k in ("gw", "gbeta"):
        want = g_o[k].double()
        d = float((g[k].detach().double().cpu() - want).abs().max())
        print(f"{name} {k} |diff| {d:.3e} bound {tol * float(want.abs().max()) + floor:.3e}")
        if not d <= tol * float(want.abs().max()) + floor:
            report.append(f"{k} |diff| {d:.3e} over {tol * float(want.abs().max()) + floor:.3e}")
    assert not report, f"{name}: " + "; ".join(report)


@pytest.mark.parametrize("row", ECA_EDGE_ROWS, ids=[r[0] for r in ECA_EDGE_ROWS])
def test_eca_channels_last_geometry_corner_vs_oracle(F, row):
    name, dt, B, C, H, W, k, kind, mask3d, mask_grad = row
    dtype = DT[dt]
    x, mask, gy = synth(B, C, H, W, seed=300 + C + H, mask_kind=kind, mask3d=mask3d)
    use_sig = kind != "prob"
    p = _eca_params(C, k, seed=C)
    if dt != "f32":
        x, gy = x.to(dtype).float(), gy.to(dtype).float()
    y_o, g_o = _oracle(x, mask, gy, p, use_sig, double=dt == "f32")
    y, g = _run(F, x, mask, gy, p, use_sig, dtype, mask_grad)
    assert y.dtype == dtype and g["gx"].dtype == dtype
    assert _is_cl(y) and _is_cl(g["gx"]), f"{name}: y / gx came back in another layout"
    assert (g["gmask"] is None) == (mask is None or not mask_grad)
    if g["gmask"] is not None:
        assert g["gmask"].shape == mask.shape
    _check(name, dt, y, g, y_o, g_o, gy, x)


# ---------------------------------------------------------------------------------------------------------------------------
# bit-identity
# ---------------------------------------------------------------------------------------------------------------------------
def _level_run(F, x, mask, w, beta, cfg, gy):
    xd = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    md = mask.detach().clone().requires_grad_(True)
    wl, bl = w.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
    y = F.mask_eca(xd, md, wl, bl, cfg)
    y.backward(gy)
    torch.cuda.synchronize()
    return [y.detach(), xd.grad, md.grad, wl.grad, bl.grad]


def test_batch_slice_and_repeat_are_bit_identical(F):
    B, C, H, W = 32, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=9)
    p = _eca_params(C, 5, seed=2)
    w, beta, cfg = p.w.cuda(), p.beta.cuda(), F.EcaConfig(k=5)
    xd, md, gd = x.cuda().to(memory_format=CL), mask.cuda(), gy.cuda().to(memory_format=CL)
    full = _level_run(F, xd, md, w, beta, cfg, gd)
    again = _level_run(F, xd, md, w, beta, cfg, gd)
    assert _is_cl(full[0]) and _is_cl(full[1])
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for b in (0, 13, 31):
        one = _level_run(F, xd[b:b + 1].contiguous(memory_format=CL), md[b:b + 1], w, beta, cfg, gd[b:b + 1].contiguous(memory_format=CL))
        for i, (a, s) in enumerate(zip(full[:3], one[:3])):        # y, gx, gmask
            assert torch.equal(a[b:b + 1], s), (b, i)


def test_mixed_layout_call_equals_per_level_calls(F):
    shapes = [(4, 64, 40, 40), (4, 128, 20, 20), (4, 256, 10, 10)]
    fmts = [CL, torch.contiguous_format, CL]
    data = []
    for i, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=30 + i)
        p = _eca_params(C, E.eca_kernel_size(C), seed=i)
        data.append((x.cuda().to(memory_format=fmts[i]), mask.cuda(), p.w.cuda(), p.beta.cuda(), F.EcaConfig(k=p.w.shape[-1]),
                     gy.cuda().to(memory_format=fmts[i])))
    leaves = []
    for x, m, w, beta, cfg, _ in data:
        leaves.append((x.clone(memory_format=torch.preserve_format).requires_grad_(True), m.clone().requires_grad_(True),
                       w.clone().requires_grad_(True), beta.clone().requires_grad_(True), cfg))
    ys = F.mask_eca_pyramid(leaves)
    torch.autograd.backward(ys, [d[5] for d in data])
    torch.cuda.synchronize()
    for i, ((x, m, w, beta, cfg, gy), (xl, ml, wl, bl, _), y) in enumerate(zip(data, leaves, ys)):
        single = _level_run(F, x, m, w, beta, cfg, gy)
        mixed = [y.detach(), xl.grad, ml.grad, wl.grad, bl.grad]
        assert _is_cl(y) == (fmts[i] is CL) and _is_cl(xl.grad) == (fmts[i] is CL), i
        for j, (a, b) in enumerate(zip(mixed, single)):
            assert torch.equal(a, b), (i, j)


def test_nchw_input_is_bit_identical_to_the_contiguous_copy_path(F):
    """An NCHW feature takes the NCHW kernels exactly as before the channels-last path existed: the same values as the kernels give for
    the `.contiguous()` copy of the channels_last tensor (what the block did with a channels_last feature until now), NCHW out."""
    B, C, H, W = 6, 96, 24, 20
    x, mask, gy = synth(B, C, H, W, seed=14, mask_kind="mixed")
    p = _eca_params(C, 5, seed=5)
    w, beta, cfg = p.w.cuda(), p.beta.cuda(), F.EcaConfig(k=5)
    xd, md, gd = x.cuda(), mask.cuda(), gy.cuda()
    direct = _level_run(F, xd, md, w, beta, cfg, gd)
    copied = _level_run(F, xd.to(memory_format=CL).contiguous(), md, w, beta, cfg, gd.to(memory_format=CL).contiguous())
    assert direct[0].is_contiguous() and direct[1].is_contiguous()
    for i, (a, b) in enumerate(zip(direct, copied)):
        assert torch.equal(a, b), i
    # and an NCHW gy for a channels_last level is converted once: the same bits as a channels_last gy
    a = _level_run(F, xd.to(memory_format=CL), md, w, beta, cfg, gd)
    b = _level_run(F, xd.to(memory_format=CL), md, w, beta, cfg, gd.to(memory_format=CL))
    assert _is_cl(a[1])
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i


@pytest.mark.parametrize("shape,kind", [((8, 64, 40, 40), "randn"), ((4, 130, 23, 17), "mixed"), ((2, 256, 40, 52), "sparse")])
def test_both_layouts_agree(F, shape, kind):
    B, C, H, W = shape
    x, mask, gy = synth(B, C, H, W, seed=40, mask_kind=kind)
    p = _eca_params(C, E.eca_kernel_size(C), seed=1)
    y0, g0 = _run(F, x, mask, gy, p, fmt=torch.contiguous_format)
    y1, g1 = _run(F, x, mask, gy, p, fmt=CL)
    assert y0.is_contiguous() and _is_cl(y1)
    assert rel_err(y1, y0) < TOL
    for k in ("gx", "gmask", "gw", "gbeta"):
        e = rel_err(g1[k], g0[k])
        print(f"{shape} {k} NHWC vs NCHW {e:.3e}")
        assert e < TOL, k


# ---------------------------------------------------------------------------------------------------------------------------
# no copies; the static plan; a small model
# ---------------------------------------------------------------------------------------------------------------------------
def test_channels_last_step_launches_only_library_kernels(F):
    B, C, H, W = 4, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=3)
    p = _eca_params(C, 5, seed=3)
    w, beta, cfg = p.w.cuda().requires_grad_(True), p.beta.cuda().requires_grad_(True), F.EcaConfig(k=5)
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    md = mask.cuda().requires_grad_(True)
    gd = gy.cuda().to(memory_format=CL)
    F.mask_eca(xd, md, w, beta, cfg).backward(gd)                       # warm: sizes
    for t in (xd, md, w, beta):
        t.grad = None
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        F.mask_eca(xd, md, w, beta, cfg).backward(gd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    kernels = [n for n in names if n.startswith(("k_", "void mgacbam", "mgacbam")) or "mgacbam::" in n]
    others = [n for n in names if n not in kernels and not n.lower().startswith(("memset", "memcpy"))]
    assert kernels, names
    assert any("nhwc" in n for n in kernels), kernels
    assert not [n for n in names if "copy" in n.lower() or "contiguous" in n.lower()], names
    assert not others, others


def test_channels_last_plan_equals_eager_and_replays(F):
    from mga_yolo_amd.plan import EcaPyramidPlan
    shapes = [(4, 64, 40, 40), (4, 128, 20, 20), (4, 260, 10, 10)]
    data, params, cfgs = [], [], []
    for i, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=60 + i, mask_kind="mixed")
        p = _eca_params(C, E.eca_kernel_size(C), seed=10 + i)
        data.append((x.cuda().to(memory_format=CL), mask.cuda(), gy.cuda().to(memory_format=CL)))
        params.append((p.w.cuda(), p.beta.cuda()))
        cfgs.append(F.EcaConfig(k=p.w.shape[-1]))
    plan = EcaPyramidPlan(shapes, params, cfgs, channels_last=True)
    assert plan.channels_last and not EcaPyramidPlan(shapes[:1], params[:1], cfgs[:1]).channels_last
    for l, (x, m, gy) in enumerate(data):
        assert _is_cl(plan.x[l]) and _is_cl(plan.y[l]) and _is_cl(plan.gy[l]) and _is_cl(plan.gx[l])
        plan.x[l].copy_(x); plan.mask[l].copy_(m); plan.gy[l].copy_(gy)
    plan.forward()
    plan.backward()
    torch.cuda.synchronize()
    direct = []
    for l, ((x, m, gy), (w, beta), cfg) in enumerate(zip(data, params, cfgs)):
        eager = _level_run(F, x, m, w, beta, cfg, gy)
        mine = [plan.y[l], plan.gx[l], plan.gmask[l], plan.param_grads[l][0], plan.param_grads[l][1]]
        for j, (a, b) in enumerate(zip(mine, eager)):
            assert torch.equal(a, b), (l, j)
        direct.append([t.clone() for t in mine])
    graph = plan.capture(lambda: (plan.forward(), plan.backward()))
    for l in range(plan.n):
        for t in (plan.y[l], plan.gx[l], plan.gmask[l]):
            t.zero_()
    plan.grad_bucket.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for l in range(plan.n):
        mine = [plan.y[l], plan.gx[l], plan.gmask[l], plan.param_grads[l][0], plan.param_grads[l][1]]
        for j, (a, b) in enumerate(zip(mine, direct[l])):
            assert torch.equal(a, b), (l, j)


def test_amp_channels_last_block_matches_nchw(F):
    """AMP fp16 + GradScaler step of MaskECA -> conv on ONE fp16 feature in both layouts, channels_last against NCHW, with the tolerances of
    test_gpu_channels_last.test_amp_channels_last_model_matches_nchw (4e-3 on values, 4 x 4e-3 on gradients).  The block's input is the
    SAME fp16 tensor in both layouts (the first conv runs once), so only the block and the 1x1 conv after it see the layout."""
    from mga_yolo_amd import MaskECA
    tol = 4e-3
    torch.manual_seed(0)
    c1 = torch.nn.Conv2d(16, 64, 3, padding=1).cuda()
    x, mask, _ = synth(4, 16, 32, 32, seed=12)
    with torch.autocast("cuda", dtype=torch.float16):
        h0 = c1(x.cuda()).detach()                       # fp16 feature, NCHW
    res = {}
    for fmt in (torch.contiguous_format, CL):
        torch.manual_seed(1)
        m = torch.nn.ModuleDict(dict(eca=MaskECA(64), c2=torch.nn.Conv2d(64, 8, 1))).cuda()
        with torch.no_grad():
            m["eca"].beta.fill_(0.5)
        m = m.to(memory_format=fmt)
        opt = torch.optim.SGD(m["eca"].parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda")
        h = h0.detach().clone(memory_format=fmt).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = m["eca"]([h, mask.cuda()])
            assert _is_cl(y) == (fmt is CL)
            loss = m["c2"](y).float().square().mean()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        inv = 1.0 / float(scaler.get_scale())
        grads = {n: p.grad.detach().float().clone() for n, p in m["eca"].named_parameters()}
        grads["block_input"] = h.grad.detach().float() * inv
        assert _is_cl(h.grad) == (fmt is CL)
        scaler.step(opt)
        scaler.update()
        res[fmt] = (float(loss.detach()), grads, {n: p.detach().clone() for n, p in m["eca"].named_parameters()})
    l0, g0, p0 = res[torch.contiguous_format]
    l1, g1, p1 = res[CL]
    assert abs(l0 - l1) <= tol * abs(l0)
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 4 * tol, n
    for n in p0:
        assert rel_err(p1[n], p0[n]) < tol, n


def test_amp_channels_last_model_matches_nchw(F):
    """conv -> MaskECA -> conv as ONE model under fp16 autocast with GradScaler: the whole model and its input converted to channels_last
    against the same model in NCHW, all parameters optimised.  The block takes whatever layout the conv in front produces and hands its
    gx back to that conv; compared: the loss, every parameter gradient (the first conv's included) and every parameter after the step,
    at the tolerances of test_gpu_channels_last.test_amp_channels_last_model_matches_nchw (4e-3 on values, 4 x 4e-3 on gradients)."""
    from mga_yolo_amd import MaskECA
    tol = 4e-3
    x, mask, _ = synth(4, 16, 32, 32, seed=12)
    res = {}
    for fmt in (torch.contiguous_format, CL):
        torch.manual_seed(1)
        m = torch.nn.ModuleDict(dict(c1=torch.nn.Conv2d(16, 64, 3, padding=1), eca=MaskECA(64), c2=torch.nn.Conv2d(64, 8, 1))).cuda()
        with torch.no_grad():
            m["eca"].beta.fill_(0.5)
        m = m.to(memory_format=fmt)
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda")
        xin = x.cuda().contiguous(memory_format=fmt)
        seen = {}
        with torch.autocast("cuda", dtype=torch.float16):
            h = m["c1"](xin)
            y = m["eca"]([h, mask.cuda()])
            seen.update(h_cl=_is_cl(h), y_cl=_is_cl(y))
            loss = m["c2"](y).float().square().mean()
        print(f"{fmt}: feature channels_last {seen['h_cl']}, block output channels_last {seen['y_cl']}")
        assert h.dtype == torch.float16 and seen["y_cl"] == seen["h_cl"]     # the block keeps the layout it is given
        if fmt is CL:
            assert seen["h_cl"], "the channels_last conv handed the block an NCHW feature: this run does not exercise the channels-last path"
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        grads = {n: p.grad.detach().float().clone() for n, p in m.named_parameters()}
        scaler.step(opt)
        scaler.update()
        res[fmt] = (float(loss.detach()), grads, {n: p.detach().clone() for n, p in m.named_parameters()})
    l0, g0, p0 = res[torch.contiguous_format]
    l1, g1, p1 = res[CL]
    assert "c1.weight" in g0 and "eca.conv1d.weight" in g0
    assert abs(l0 - l1) <= tol * abs(l0)
    for n in g0:
        print(f"{n} grad rel_err {rel_err(g1[n], g0[n]):.3e}  param rel_err {rel_err(p1[n], p0[n]):.3e}")
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 4 * tol, n
    for n in p0:
        assert rel_err(p1[n], p0[n]) < tol, n


def test_wider_than_the_channels_last_limit_keeps_the_copy_path(F):
    """C > 4096 (the channels-last kernels keep 3 floats per channel in LDS): a channels_last feature is copied to NCHW once and runs the
    NCHW kernels, as it did before the channels-last path existed; y comes back NCHW."""
    B, C, H, W = 2, 4100, 3, 4
    x, mask, gy = synth(B, C, H, W, seed=77)
    p = _eca_params(C, 7, seed=7)
    y_o, g_o = _oracle(x, mask, gy, p, True, double=False)
    y, g = _run(F, x, mask, gy, p, fmt=CL)
    assert y.is_contiguous()
    y2, g2 = _run(F, x, mask, gy, p, fmt=torch.contiguous_format)
    assert torch.equal(y, y2) and torch.equal(g["gx"], g2["gx"]) and torch.equal(g["gmask"], g2["gmask"])
    assert rel_err(y, y_o) < TOL and rel_err(g["gx"], g_o["gx"]) < TOL and rel_err(g["gmask"], g_o["gmask"]) < TOL
