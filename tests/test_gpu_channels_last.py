"""GPU tests (-m gpu) of MaskCBAM on channels_last features: the MGACBAM_LAYOUT_NHWC kernels against the reference's golden vectors,
the NCHW path's saved statistics, the reference checksums at BASELINE sizes, and the reproducibility / composition properties."""
import pytest
import torch

from conftest import checksum, elem_err, golden_case_names, load_golden, rel_err, synth
from oracle import maskcbam_oracle as O
from test_gpu_parity import (CONFIG5_SHAPES, CONFIG_LEVELS, FULL_SIZE_SHAPES, FUZZER_REGRESSIONS, GENERIC_KS, GRADS, TOL, _cfg,
                              _params_dev)

pytestmark = pytest.mark.gpu
CL = torch.channels_last


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


def _is_cl(t):
    return t.is_contiguous(memory_format=CL) and not t.is_contiguous()


ORACLE_FALLBACK = {("r4", "gw1")}


@pytest.mark.parametrize("name", golden_case_names())
def test_golden_channels_last(F, name):
    d = load_golden(name)
    x = d["x"].cuda().to(memory_format=CL).requires_grad_(True)
    mask = None if d["mask"] is None else d["mask"].cuda().requires_grad_(True)
    ps = _params_dev(d, True)
    y = F.mask_cbam(x, mask, *ps, _cfg(F, d))
    y.backward(d["gy"].cuda().to(memory_format=CL))
    torch.cuda.synchronize()
    g = dict(gx=x.grad, gmask=None if mask is None else mask.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad,
             gb2=ps[3].grad, gwsa=ps[4].grad, gbeta=ps[5].grad)
    layout_kept = _is_cl(y) and _is_cl(x.grad)
    if d["x"].shape[1] == 1 or d["x"].shape[2] * d["x"].shape[3] == 1:
        layout_kept = True                                             # ambiguous layouts run the NCHW path
    assert layout_kept, f"{name}: y / gx came back in another layout"
    # The bounds of test_fwd_bwd_vs_reference_golden.  For the (case, tensor) pairs in ORACLE_FALLBACK alone, the element-wise bound may
    # instead hold against the fp64 oracle on the golden's inputs: the golden is the reference's own fp32 result, and its small elements
    # carry its summation order, which the channels-last reductions do not share (case_r4.npz, reduction ratio 4: the golden's gw1 is
    # itself 7.5e-4 element-wise from fp64).  Any other pair that misses the golden fails, and a listed pair must still meet 1e-3.
    exact = None

    def elem_ok(k, got):
        nonlocal exact
        if elem_err(got, d["out"][k]) < 1e-3:
            return True
        if (name, k) not in ORACLE_FALLBACK:
            return False
        if exact is None:
            p = O.Params.from_state_dict({n: v.double() for n, v in d["params"].items()})
            m = d["meta"]
            oc = O.Config(use_sigmoid_mask=m["use_sigmoid_mask"], tiny_thr=m["tiny_thr"], eps=m["eps"])
            md = None if d["mask"] is None else d["mask"].double()
            y_o, c = O.forward(d["x"].double(), md, p, oc)
            exact = dict(O.backward(d["gy"].double(), d["x"].double(), md, p, oc, c), y=y_o)
        return elem_err(got, exact[k]) < 1e-3

    report = []
    if not rel_err(y, d["out"]["y"]) < TOL or not elem_ok("y", y):
        report.append(f"y {rel_err(y, d['out']['y']):.3e}")
    for k in GRADS:
        if k == "gmask" and d["mask"] is None:
            assert g[k] is None
            continue
        assert g[k].shape == d["out"][k].shape, k
        e = rel_err(g[k], d["out"][k])
        if not (e < TOL and elem_ok(k, g[k])):
            report.append(f"{k} {e:.3e} / element-wise {elem_err(g[k], d['out'][k]):.3e}")
    assert not report, f"{name}: " + "; ".join(report)


@pytest.mark.parametrize("shape", [(32, 64, 80, 80), (1, 48, 17, 17), (3, 5, 9, 7)])
def test_stagewise_statistics_match_nchw(F, shape):
    B, C, H, W = shape
    x, mask, _ = synth(B, C, H, W, seed=5)
    p = O.Params.default_init(C)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0])
    xd, md = x.cuda(), mask.cuda()
    y0, v0 = F.forward_with_ctx(xd, md, ps, cfg)
    y1, v1 = F.forward_with_ctx(xd.to(memory_format=CL), md, ps, cfg)
    torch.cuda.synchronize()
    assert _is_cl(y1)
    assert torch.equal(v0["amax"], v1["amax"]) and torch.equal(v0["valid"], v1["valid"])
    for k in ("S", "den", "avg", "mx", "mavg", "ca", "planes", "sa"):
        assert rel_err(v1[k], v0[k]) < 1e-5, k
    assert rel_err(y1, y0) < 1e-5
    # cidx: equal except at pixels whose top-2 channel gap of u = x*ca is within rounding
    u = (xd * v0["ca"][:, :, None, None]).reshape(B, C, H * W)
    top = u.topk(min(2, C), dim=1).values
    gap = (top[:, 0] - top[:, -1]).abs() if C > 1 else torch.full_like(top[:, 0], 1.0)
    differ = v0["cidx"] != v1["cidx"]
    assert bool((gap[differ] <= 1e-5 * top[:, 0].abs()[differ].clamp_min(1e-6)).all()), int(differ.sum())


def _pyramid(F, names, dtype, checksums, fmt):
    levels, leaves, gys = [], [], []
    for name in names:
        ref = checksums["big"][name]
        B, C, H, W = ref["shape"]
        x, mask, gy = synth(B, C, H, W, mask_kind=ref["mask_kind"])
        p = O.Params.default_init(C)
        ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
        xd = x.cuda().to(dtype).to(memory_format=fmt).requires_grad_(True)
        md = mask.cuda().requires_grad_(True)
        levels.append((xd, md, ps, F.BlockConfig(hidden=p.w1.shape[0])))
        leaves.append((xd, md, ps))
        gys.append(gy.cuda().to(dtype).to(memory_format=fmt))
    ys = F.mask_cbam_pyramid(levels)
    torch.autograd.backward(ys, gys)
    torch.cuda.synchronize()
    return [dict(y=y.detach(), gx=xd.grad, gmask=md.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad, gb2=ps[3].grad,
                 gwsa=ps[4].grad, gbeta=ps[5].grad) for y, (xd, md, ps) in zip(ys, leaves)]


@pytest.mark.parametrize("config", list(CONFIG_LEVELS))
def test_baseline_config_pyramid_channels_last_vs_reference_checksums(F, checksums, config):
    _, names, dtype = CONFIG_LEVELS[config]
    tol = TOL if dtype == torch.float32 else 1e-3
    got = _pyramid(F, names, dtype, checksums, CL)
    report = []
    for name, g in zip(names, got):
        assert _is_cl(g["y"]) and _is_cl(g["gx"]), name
        ref = checksums["big"][name]
        for k, v in g.items():
            c = checksum(v.float())
            scale = ref[k]["abs"] + 1e-12
            for f in ("sum", "wsum", "abs"):
                if not abs(c[f] - ref[k][f]) <= tol * scale:
                    report.append(f"{name}.{k}.{f}: got {c[f]:.6f} want {ref[k][f]:.6f}")
    assert not report, f"{config}: " + "; ".join(report)
    again = _pyramid(F, names, dtype, checksums, CL)                    # bitwise run-to-run reproducible
    for g0, g1 in zip(got, again):
        for k in g0:
            assert torch.equal(g0[k], g1[k]), k


@pytest.mark.parametrize("C,hw", [(64, (20, 20)), (128, (10, 10)), (256, (5, 5)), (192, (40, 40)), (384, (20, 20)), (576, (10, 10)),
                                  (60, (6, 7)), (7, (9, 5))])
@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2)])
def test_half_precision_channels_last(F, dtype, tol, C, hw):
    """cfg2 widths (64 / 128 / 256), configs[4] widths (192 / 384 / 576) and the 8-byte / scalar lanes, against the fp32 oracle."""
    B, (H, W) = 4, hw
    x, mask, gy = synth(B, C, H, W, seed=21)
    x, gy = x.to(dtype).float(), gy.to(dtype).float()
    p = O.Params.default_init(C)
    y_o, ctx = O.forward(x, mask, p)
    g_o = O.backward(gy, x, mask, p, O.Config(), ctx)
    xd = x.cuda().to(dtype).to(memory_format=CL).requires_grad_(True)
    md = mask.cuda().requires_grad_(True)
    ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    y = F.mask_cbam(xd, md, *ps, F.BlockConfig(hidden=p.w1.shape[0]))
    assert y.dtype == dtype and _is_cl(y)
    y.backward(gy.cuda().to(dtype).to(memory_format=CL))
    assert xd.grad.dtype == dtype and _is_cl(xd.grad)
    assert rel_err(y.float(), y_o) < tol
    assert rel_err(xd.grad.float(), g_o["gx"]) < tol
    assert rel_err(md.grad, g_o["gmask"]) < tol
    assert rel_err(ps[0].grad, g_o["gw1"]) < tol and rel_err(ps[5].grad, g_o["gbeta"]) < tol


def _level_run(F, x, mask, ps, cfg, gy):
    xd = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    md = mask.detach().clone().requires_grad_(True)
    pl = [t.detach().clone().requires_grad_(True) for t in ps]
    y = F.mask_cbam(xd, md, *pl, cfg)
    y.backward(gy)
    return [y.detach(), xd.grad, md.grad] + [t.grad for t in pl]


def test_batch_slice_and_repeat_are_bit_identical(F):
    B, C, H, W = 32, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=9)
    p = O.Params.default_init(C)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0])
    xd, md, gd = x.cuda().to(memory_format=CL), mask.cuda(), gy.cuda().to(memory_format=CL)
    full = _level_run(F, xd, md, ps, cfg, gd)
    again = _level_run(F, xd, md, ps, cfg, gd)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for b in (0, 13, 31):
        one = _level_run(F, xd[b:b + 1].contiguous(memory_format=CL), md[b:b + 1], ps, cfg, gd[b:b + 1].contiguous(memory_format=CL))
        for a, s in zip(full[:3], one[:3]):
            assert torch.equal(a[b:b + 1], s), b


def test_mixed_layout_call_equals_per_level_calls(F):
    shapes = [(4, 64, 40, 40), (4, 128, 20, 20), (4, 256, 10, 10)]
    fmts = [CL, torch.contiguous_format, CL]
    data = []
    for i, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=30 + i)
        p = O.Params.default_init(C)
        ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
        data.append((x.cuda().to(memory_format=fmts[i]), mask.cuda(), ps, F.BlockConfig(hidden=p.w1.shape[0]),
                     gy.cuda().to(memory_format=fmts[i])))
    leaves = []
    for x, m, ps, cfg, _ in data:
        leaves.append((x.clone(memory_format=torch.preserve_format).requires_grad_(True), m.clone().requires_grad_(True),
                       [t.clone().requires_grad_(True) for t in ps], cfg))
    ys = F.mask_cbam_pyramid(leaves)
    torch.autograd.backward(ys, [d[4] for d in data])
    for i, ((x, m, ps, cfg, gy), (xl, ml, pl, _), y) in enumerate(zip(data, leaves, ys)):
        single = _level_run(F, x, m, ps, cfg, gy)
        mixed = [y.detach(), xl.grad, ml.grad] + [t.grad for t in pl]
        assert (y.is_contiguous(memory_format=fmts[i]))
        for a, b in zip(mixed, single):
            assert torch.equal(a, b), i


def test_alternating_layouts_on_the_pooled_ctx(F):
    """NCHW calls (hand-off counters in the pooled ctx) and NHWC calls on one shape, alternating: every result equals a fresh call's."""
    B, C, H, W = 8, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=44)
    p = O.Params.default_init(C)
    ps = [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0])
    xd, md, gd = x.cuda(), mask.cuda(), gy.cuda()
    F._POOL.clear()
    first = {False: _level_run(F, xd, md, ps, cfg, gd), True: _level_run(F, xd.to(memory_format=CL), md, ps, cfg, gd.to(memory_format=CL))}
    for it in range(6):
        cl = bool(it % 2)
        got = _level_run(F, xd.to(memory_format=CL) if cl else xd, md, ps, cfg, gd.to(memory_format=CL) if cl else gd)
        for a, b in zip(got, first[cl]):
            assert torch.equal(a, b), (it, cl)
    F.handoff_report()


def test_channels_last_step_launches_only_library_kernels(F):
    B, C, H, W = 4, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=3)
    p = O.Params.default_init(C)
    ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    cfg = F.BlockConfig(hidden=p.w1.shape[0])
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    md = mask.cuda().requires_grad_(True)
    gd = gy.cuda().to(memory_format=CL)
    F.mask_cbam(xd, md, *ps, cfg).backward(gd)                        # warm: pools, sizes
    for t in [xd, md] + ps:
        t.grad = None
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        F.mask_cbam(xd, md, *ps, cfg).backward(gd)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    kernels = [n for n in names if n.startswith(("k_", "void mgacbam", "mgacbam")) or "mgacbam::" in n]
    others = [n for n in names if n not in kernels and not n.lower().startswith(("memset", "memcpy"))]
    assert kernels, names
    assert not [n for n in names if "copy" in n.lower() or "contiguous" in n.lower()], names
    assert not others, others


def test_amp_channels_last_model_matches_nchw(F):
    """AMP fp16 + GradScaler step of conv -> MaskCBAM -> conv, channels_last against NCHW, with the tolerances of the AMP slice test
    (test_gpu_slice: 4e-3 on values, 4 x 4e-3 on gradients).  The block's input is the SAME fp16 tensor in both layouts (the first conv
    runs once), so only the block and the 1x1 conv after it see the layout; compared: the loss, the gradient that flows out of the block
    into its input, the block's parameter gradients (unscaled by the scaler) and the block's parameters after the step."""
    from mga_yolo_amd import MaskCBAM
    tol = 4e-3
    torch.manual_seed(0)
    c1 = torch.nn.Conv2d(16, 64, 3, padding=1).cuda()
    x, mask, _ = synth(4, 16, 32, 32, seed=12)
    with torch.autocast("cuda", dtype=torch.float16):
        h0 = c1(x.cuda()).detach()                       # fp16 feature, NCHW
    res = {}
    for fmt in (torch.contiguous_format, CL):
        torch.manual_seed(1)
        m = torch.nn.ModuleDict(dict(cb=MaskCBAM(64), c2=torch.nn.Conv2d(64, 8, 1))).cuda()
        with torch.no_grad():
            m["cb"].beta.fill_(0.5)                      # a non-zero alpha gradient path; parameters compared after the step below
        m = m.to(memory_format=fmt)
        opt = torch.optim.SGD(m["cb"].parameters(), lr=0.1)
        scaler = torch.amp.GradScaler("cuda")
        h = h0.detach().clone(memory_format=fmt).requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = m["cb"]([h, mask.cuda()])
            loss = m["c2"](y).float().square().mean()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        inv = 1.0 / float(scaler.get_scale())
        grads = {n: p.grad.detach().float().clone() for n, p in m["cb"].named_parameters()}
        grads["block_input"] = h.grad.detach().float() * inv
        scaler.step(opt)
        scaler.update()
        res[fmt] = (float(loss.detach()), grads, {n: p.detach().clone() for n, p in m["cb"].named_parameters()})
    l0, g0, p0 = res[torch.contiguous_format]
    l1, g1, p1 = res[CL]
    assert abs(l0 - l1) <= tol * abs(l0)
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 4 * tol, n
    for n in p0:
        assert rel_err(p1[n], p0[n]) < tol, n


# ---------------------------------------------------------------------------------------------------------------------------
# channels_last counterparts of test_gpu_parity's oracle tests: the same shapes, inputs and bars, features channels_last.  The
# full-size rows (1, 256, 160, 160), (8, 512, 80, 80) and (32, 128, 80, 80) have several tiles per chunk (nhwc_geo's rp >= 2) and a
# ragged last chunk: element-wise checks of that tiling.  test_gpu_channels_last_edges.py holds the geometry-corner matrix.
# ---------------------------------------------------------------------------------------------------------------------------
def _run_cl(F, x, mask, gy, p, k=7, use_sig=True, dtype=torch.float32):
    """x / gy channels_last on the device -> (y, grads); asserts y and gx come back channels_last (ambiguous layouts excepted)."""
    xd = x.cuda().to(dtype).to(memory_format=CL).requires_grad_(True)
    md = None if mask is None else mask.cuda().requires_grad_(True)
    ps = [t.cuda().requires_grad_(True) for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]
    y = F.mask_cbam(xd, md, *ps, F.BlockConfig(hidden=p.w1.shape[0], k=k, use_sigmoid_mask=use_sig))
    y.backward(gy.cuda().to(dtype).to(memory_format=CL))
    torch.cuda.synchronize()
    B, C, H, W = x.shape
    if C > 1 and H * W > 1:
        assert _is_cl(y) and _is_cl(xd.grad), "y / gx came back in another layout"
    g = dict(gx=xd.grad, gmask=None if md is None else md.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad, gb2=ps[3].grad,
             gwsa=ps[4].grad, gbeta=ps[5].grad)
    return y.detach(), g


@pytest.mark.parametrize("shape,mask_kind", FULL_SIZE_SHAPES)
def test_full_size_vs_oracle_live_channels_last(F, shape, mask_kind):
    B, C, H, W = shape
    if mask_kind == "mixed" and B < 2:
        mask_kind = "randn"
    x, mask, gy = synth(B, C, H, W, seed=77, mask_kind=mask_kind)
    p = O.Params.default_init(C, seed=3)
    p.beta.fill_(0.3)
    y_o, ctx = O.forward(x, mask, p)
    g_o = O.backward(gy, x, mask, p, O.Config(), ctx)
    y, g = _run_cl(F, x, mask, gy, p)
    report = []
    if not rel_err(y, y_o) < TOL:
        report.append(f"y {rel_err(y, y_o):.3e}")
    for k in GRADS:
        if g_o[k] is None:
            continue
        e = rel_err(g[k], g_o[k])
        if not e < TOL:
            report.append(f"{k} {e:.3e}")
    for k, got, want in (("y", y, y_o), ("gx", g["gx"], g_o["gx"]), ("gmask", g["gmask"], g_o["gmask"])):
        if want is not None and not elem_err(got, want) < 1e-3:
            report.append(f"{k} element-wise {elem_err(got, want):.3e}")
    assert not report, "; ".join(report)


@pytest.mark.parametrize("k", GENERIC_KS)
def test_generic_spatial_kernel_sizes_channels_last(F, k):
    """Run-time k (k_apply_nhwc<..., 0>) and k = 1 on channels_last features."""
    B, C, H, W = 3, 32, 12, 20
    x, mask, gy = synth(B, C, H, W, seed=k, mask_kind="mixed")
    p = O.Params.default_init(C, k=k, seed=2)
    with torch.no_grad():
        p.wsa.mul_(3.0)
    y_o, c = O.forward(x, mask, p)
    g_o = O.backward(gy, x, mask, p, O.Config(), c)
    y, g = _run_cl(F, x, mask, gy, p, k=k)
    assert rel_err(y, y_o) < TOL
    for name in GRADS:
        assert rel_err(g[name], g_o[name]) < TOL, name


@pytest.mark.parametrize("B,C,H,W,k,r,kind", FUZZER_REGRESSIONS)
def test_regressions_found_by_the_fuzzer_channels_last(F, B, C, H, W, k, r, kind):
    x, mask, gy = synth(B, C, H, W, seed=5, mask_kind=kind)
    p = O.Params.default_init(C, r=r, k=k, seed=1)
    cfg = O.Config(use_sigmoid_mask=kind != "prob")
    y_o, c = O.forward(x, mask, p, cfg)
    g_o = O.backward(gy, x, mask, p, cfg, c)
    y, g = _run_cl(F, x, mask, gy, p, k=k, use_sig=kind != "prob")
    assert rel_err(y, y_o) < TOL
    floor = 1e-6 * float(gy.norm() * x.norm())
    for name in GRADS:
        tol = TOL * float(g_o[name].abs().max()) + (floor if name not in ("gx",) else 0.0)
        assert float((g[name].detach().cpu().double() - g_o[name].double()).abs().max()) <= tol, name


@pytest.mark.parametrize("shape,dtype,tol", CONFIG5_SHAPES)
def test_config5_shapes_low_precision_channels_last(F, shape, dtype, tol):
    B, C, H, W = shape
    x, mask, gy = synth(B, C, H, W, seed=91, mask_kind="sparse")
    x, gy = x.to(dtype).float(), gy.to(dtype).float()
    p = O.Params.default_init(C, seed=5)
    y_o, ctx = O.forward(x, mask, p)
    g_o = O.backward(gy, x, mask, p, O.Config(), ctx)
    y, g = _run_cl(F, x, mask, gy, p, dtype=dtype)
    assert y.dtype == dtype and g["gx"].dtype == dtype
    assert rel_err(y.float(), y_o) < tol and rel_err(g["gx"].float(), g_o["gx"]) < tol and rel_err(g["gmask"], g_o["gmask"]) < tol
    for k in ("gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta"):
        assert rel_err(g[k], g_o[k]) < tol, k


def test_backward_is_linear_in_gy_channels_last(F):
    B, C, H, W = 32, 64, 80, 80
    x, mask, gy = synth(B, C, H, W, seed=9, mask_kind="sparse")
    p = O.Params.default_init(C)
    _, g1 = _run_cl(F, x, mask, gy, p)
    _, g2 = _run_cl(F, x, mask, -2.5 * gy, p)
    for k in GRADS:
        assert rel_err(g2[k], -2.5 * g1[k]) < 1e-5, k
