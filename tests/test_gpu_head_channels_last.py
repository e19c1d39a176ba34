"""GPU tests (-m gpu) of MGAMaskHead on channels_last features: the MGAHEAD_LAYOUT_NHWC kernels (csrc/head_nhwc.cuh) against the
reference's goldens and checksums (the bars of test_maskhead.py), the live oracle in half precision, the layout of the gradient, the
absence of layout copies, ACCUM_GX through the C ABI, mixed-layout pyramid calls and the layer-loop hand-off into MaskCBAM."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN, checksum, rel_err
from oracle import maskhead_oracle as HO
from test_maskhead import TOL, _CASE, _close, _module_from_golden, head_golden_names, load_head_golden

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _is_cl(t):
    return t.is_contiguous(memory_format=CL) and not t.is_contiguous()


@pytest.mark.parametrize("name", head_golden_names())
def test_golden_channels_last(built_lib, name):
    """Every head golden with a channels_last feature through the module: logits, every gradient, the running statistics and
    num_batches_tracked at the bars of test_device_path_matches_the_reference_golden; the input gradient comes back channels_last."""
    d = load_head_golden(name)
    _CASE[0] = name
    m = _module_from_golden(d, "cuda")
    x = d["x"].cuda().to(memory_format=CL).requires_grad_(True)
    y = m(x)
    y.backward(d["g"].cuda())
    o = d["out"]
    _close(y.detach().cpu(), o["logits"], TOL, "logits")
    _close(x.grad.cpu(), o["gx"], TOL, "gx")
    p = dict(m.named_parameters())
    for k, n in (("gw1", "proj.0.weight"), ("ggamma", "proj.1.weight"), ("gbeta", "proj.1.bias"), ("gwh", "head.weight"), ("gbh", "head.bias")):
        _close(p[n].grad.cpu(), o[k], TOL, k)
    sd = m.state_dict()
    _close(sd["proj.1.running_mean"].cpu(), o["running_mean"], TOL, "running_mean")
    _close(sd["proj.1.running_var"].cpu(), o["running_var"], TOL, "running_var")
    assert int(sd["proj.1.num_batches_tracked"]) == int(o["num_batches_tracked"])
    ambiguous = x.shape[1] == 1 or x.shape[2] * x.shape[3] == 1
    assert ambiguous or _is_cl(x.grad)


@pytest.mark.parametrize("name", ["cfg2_p3", "cfg2_p4", "cfg2_p5", "cfg3_p3", "cfg3_p4", "cfg3_p5",
                                  "cfg5_640_p3", "cfg5_640_p4", "cfg5_640_p5", "cfg5_1280_p3", "cfg4_p3_192"])
def test_full_size_checksums_channels_last(built_lib, name):
    """The rows of test_device_full_size_checksums_vs_reference fed channels_last, at the same bars; two runs are bit-identical."""
    from mga_yolo_amd import MGAMaskHead
    ref = json.load(open(os.path.join(GOLDEN, "head_checksums.json")))["big"][name]
    B, Cc, hid, H, W = ref["shape"]
    bf16 = ref.get("recipe") == "bf16"
    tol = 1e-3 if bf16 else TOL
    torch.manual_seed(0)
    m = MGAMaskHead(Cc, hid)
    m.proj[1].eps, m.proj[1].momentum = ref["eps"], ref["momentum"]
    m.cuda().train()
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(B, Cc, H, W, generator=g)
    gl = torch.randn(B, 1, H, W, generator=g)
    if bf16:
        x, gl = x.bfloat16(), gl.bfloat16()
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    del x
    y = m(xd)
    y.backward(gl.cuda())
    assert _is_cl(xd.grad)
    p = dict(m.named_parameters())
    got = dict(logits=y.detach(), gx=xd.grad, gw1=p["proj.0.weight"].grad, ggamma=p["proj.1.weight"].grad, gbeta=p["proj.1.bias"].grad,
               gwh=p["head.weight"].grad, gbh=p["head.bias"].grad, running_mean=m.proj[1].running_mean, running_var=m.proj[1].running_var)
    report = []
    for k, v in got.items():
        c = checksum(v.contiguous().float())
        scale = ref[k]["abs"] + 1e-12
        for f in ("sum", "wsum", "abs"):
            if not abs(c[f] - ref[k][f]) <= tol * scale:
                report.append(f"{k}.{f}: got {c[f]:.6f} want {ref[k][f]:.6f}")
    assert not report, f"{name}: " + "; ".join(report)
    gx1, gw1 = xd.grad.clone(), p["proj.0.weight"].grad.clone()
    m.zero_grad(); xd.grad = None
    y2 = m(xd); y2.backward(gl.cuda())
    assert torch.equal(y2, y) and torch.equal(xd.grad, gx1) and torch.equal(p["proj.0.weight"].grad, gw1)


def _perturbed_head(Cc, hid, seed):
    from mga_yolo_amd import MGAMaskHead
    torch.manual_seed(seed)
    m = MGAMaskHead(Cc, hid).train()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for p_ in m.parameters():
            p_.add_(0.3 * torch.randn(p_.shape, generator=g))
    return m


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2), (torch.float32, TOL)])
@pytest.mark.parametrize("B,Cc,hid,H,W", [(4, 128, 32, 20, 20),
                                          (3, 36, 8, 9, 11),      # C % 8 != 0 (4-channel lanes), H*W % 4 != 0
                                          (2, 6, 8, 7, 5),        # C % 4 != 0: per-element lanes along C
                                          (2, 768, 192, 6, 10),   # hidden 192: the hidden > 128 forward template, dW1 in 3 passes
                                          (1, 20, 40, 2, 500),    # the widest row (W = 500)
                                          (1, 130, 200, 12, 20),  # hidden 200 / 256 / 384: more 16-row M tiles; at 384 more than
                                          (2, 64, 256, 8, 8),     # 4 waves x 4 tiles per wave, and dW1 in 4 / 6 passes of 64
                                          (2, 96, 384, 9, 13)])
def test_channels_last_vs_live_oracle(built_lib, dtype, tol, B, Cc, hid, H, W):
    """fp32 / fp16 / bf16 channels_last features against the fp32 oracle on the rounded inputs (4e-3 / 3e-2 for half precision)."""
    m = _perturbed_head(Cc, hid, 21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(B, Cc, H, W, generator=g).to(dtype)
    gl = torch.randn(B, 1, H, W, generator=g).to(dtype)
    p = HO.HeadParams.from_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    lo, c = HO.forward(x.float(), p, True)
    go = HO.backward(gl.float(), x.float(), p, c, True)
    m.cuda()
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    y = m(xd)
    assert y.dtype == dtype
    y.backward(gl.cuda())
    assert xd.grad.dtype == dtype and _is_cl(xd.grad)
    assert rel_err(y.float(), lo) < tol and rel_err(xd.grad.float(), go["gx"]) < tol
    assert rel_err(m.proj[0].weight.grad.reshape(hid, Cc), go["gw1"]) < tol and rel_err(m.head.weight.grad, go["gwh"]) < tol
    assert rel_err(m.proj[1].weight.grad, go["ggamma"]) < tol and rel_err(m.proj[1].bias.grad, go["gbeta"]) < tol


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 4e-3), (torch.bfloat16, 3e-2), (torch.float32, TOL)])
@pytest.mark.parametrize("B,Cc,hid,H,W", [(3, 36, 8, 9, 11), (2, 6, 8, 7, 5), (1, 130, 200, 12, 20), (2, 96, 384, 9, 13)])
def test_channels_last_eval_mode_vs_live_oracle(built_lib, dtype, tol, B, Cc, hid, H, W):
    """Eval mode (running statistics, perturbed) on channels_last features, every element type, against the fp32 oracle."""
    m = _perturbed_head(Cc, hid, 31)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        m.proj[1].running_mean.add_(0.2 * torch.randn(hid, generator=g))
        m.proj[1].running_var.mul_(0.5 + torch.rand(hid, generator=g))
    m.eval()
    x = torch.randn(B, Cc, H, W, generator=g).to(dtype)
    gl = torch.randn(B, 1, H, W, generator=g).to(dtype)
    p = HO.HeadParams.from_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
    lo, c = HO.forward(x.float(), p, False)
    go = HO.backward(gl.float(), x.float(), p, c, False)
    m.cuda()
    xd = x.cuda().to(memory_format=CL).requires_grad_(True)
    y = m(xd)
    y.backward(gl.cuda())
    assert xd.grad.dtype == dtype and _is_cl(xd.grad)
    assert rel_err(y.float(), lo) < tol and rel_err(xd.grad.float(), go["gx"]) < tol
    assert rel_err(m.proj[0].weight.grad.reshape(hid, Cc), go["gw1"]) < tol and rel_err(m.head.weight.grad, go["gwh"]) < tol
    assert rel_err(m.proj[1].weight.grad, go["ggamma"]) < tol and rel_err(m.proj[1].bias.grad, go["gbeta"]) < tol
    assert torch.equal(m.proj[1].running_mean.cpu(), p.running_mean) and torch.equal(m.proj[1].running_var.cpu(), p.running_var)


def test_gradient_comes_back_channels_last(built_lib):
    m = _perturbed_head(64, 16, 3).cuda()
    x = torch.randn(2, 64, 12, 12, device="cuda").to(memory_format=CL).requires_grad_(True)
    (gx,) = torch.autograd.grad(m(x).sum(), x)
    assert _is_cl(gx)


def test_channels_last_head_launches_only_library_kernels(built_lib):
    """Forward + backward of mask_head on a channels_last x with contiguous parameters: library kernels only, no layout copy."""
    import mga_yolo_amd.functional as F
    m = _perturbed_head(64, 16, 4).cuda()
    bn = m.proj[1]
    x = torch.randn(4, 64, 40, 40, device="cuda").to(memory_format=CL).requires_grad_(True)
    gl = torch.randn(4, 1, 40, 40, device="cuda")
    ps = [m.proj[0].weight, bn.weight, bn.bias, m.head.weight, m.head.bias]
    assert all(t.is_contiguous() for t in ps)

    def step():
        y = F.mask_head(x, ps[0], ps[1], ps[2], bn.running_mean, bn.running_var, bn.num_batches_tracked, ps[3], ps[4],
                        eps=bn.eps, momentum=bn.momentum, training=True)
        y.backward(gl)
    step()                                                        # warm: pools, sizes
    for t in [x] + ps:
        t.grad = None
    torch.cuda.synchronize()
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    kernels = [n for n in names if n.startswith(("k_", "void mgacbam", "mgacbam")) or "mgacbam::" in n]
    others = [n for n in names if n not in kernels and not n.lower().startswith(("memset", "memcpy"))]
    assert kernels, names
    assert any("nhwc" in n for n in kernels), kernels
    assert not [n for n in names if "copy" in n.lower() or "contiguous" in n.lower()], names
    assert not others, others


def _abi_levels(m, x, gl, flags, dtype_code):
    """One NHWC level of the C ABI for module m, feature x (channels_last), dL/dlogits gl: (fwd level, bwd level, buffers)."""
    from mga_yolo_amd import _lib
    from mga_yolo_amd.functional import _head_params
    lib = _lib.load()
    B, Cc, H, W = x.shape
    hid = m.proj[0].weight.shape[0]
    bn = m.proj[1]
    w1 = m.proj[0].weight.detach().reshape(hid, Cc).contiguous()
    pars = [w1, bn.weight.detach(), bn.bias.detach(), m.head.weight.detach(), m.head.bias.detach()]
    P = _head_params(*pars[:3], bn.running_mean, bn.running_var, None, *pars[3:], hid, bn.eps, bn.momentum, True)
    cbuf = torch.empty(lib.mgahead_ctx_bytes_flags(B, Cc, H, W, hid, flags), dtype=torch.uint8, device="cuda")
    sbuf = torch.empty(lib.mgahead_bwd_scratch_bytes_flags(B, Cc, H, W, hid, flags), dtype=torch.uint8, device="cuda")
    logits = torch.empty(B, 1, H, W, dtype=x.dtype, device="cuda")
    pg = [torch.empty_like(t) for t in pars]
    fl = (_lib.HeadFwdLevel * 1)()
    F = fl[0]
    F.x, F.logits, F.ctx, F.ctx_bytes, F.p = x.data_ptr(), logits.data_ptr(), cbuf.data_ptr(), cbuf.numel(), P
    F.B, F.C, F.H, F.W, F.dtype, F.flags = B, Cc, H, W, dtype_code, flags
    bl = (_lib.HeadBwdLevel * 1)()
    Bw = bl[0]
    Bw.x, Bw.g_logits, Bw.g_logits2, Bw.ctx, Bw.scratch = x.data_ptr(), gl.data_ptr(), None, cbuf.data_ptr(), sbuf.data_ptr()
    Bw.ctx_bytes, Bw.scratch_bytes = cbuf.numel(), sbuf.numel()
    Bw.gw1, Bw.gbn_weight, Bw.gbn_bias, Bw.gwh, Bw.gbh = (t.data_ptr() for t in pg)
    Bw.p, Bw.B, Bw.C, Bw.H, Bw.W, Bw.dtype, Bw.flags = P, B, Cc, H, W, dtype_code, flags
    return fl, bl, [cbuf, sbuf, logits, pg, pars]


@pytest.mark.parametrize("dtype,code,tol", [(torch.float32, 0, 0.0), (torch.float16, 1, 4e-3), (torch.bfloat16, 2, 3e-2)])
@pytest.mark.parametrize("Cc,H,W", [(64, 16, 16), (36, 7, 9), (6, 5, 5)])
def test_accum_gx_through_the_c_abi_on_an_nhwc_level(built_lib, dtype, code, tol, Cc, H, W):
    """gx pre-filled with G0 and MGAHEAD_BWD_ACCUM_GX: the result is G0 + the non-accumulating result (bitwise in fp32)."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    B = 3
    m = _perturbed_head(Cc, 16, 7).cuda()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(B, Cc, H, W, generator=g).to(dtype).cuda().to(memory_format=CL)
    gl = torch.randn(B, 1, H, W, generator=g).to(dtype).cuda()
    g0 = torch.randn(B, Cc, H, W, generator=g).to(dtype).cuda().to(memory_format=CL)
    NH = _lib.HEAD_LAYOUT_NHWC
    fl, bl, keep = _abi_levels(m, x, gl, NH, code)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mgahead_forward(fl, 1, st), "mgahead_forward")
    gx_plain = torch.full_like(g0, float("nan"))
    bl[0].gx = gx_plain.data_ptr()
    _lib.check(lib.mgahead_backward(bl, 1, st), "mgahead_backward")
    gx_acc = g0.clone(memory_format=CL)
    bl[0].gx, bl[0].flags = gx_acc.data_ptr(), NH | _lib.HEAD_BWD_ACCUM_GX
    _lib.check(lib.mgahead_backward(bl, 1, st), "mgahead_backward")
    torch.cuda.synchronize()
    assert torch.isfinite(gx_plain.float()).all()
    want = (g0.float() + gx_plain.float())
    if dtype == torch.float32:
        assert torch.equal(gx_acc, want)
    else:
        assert rel_err(gx_acc.float(), want) < tol


def _levels_of(mods, xs, training):
    lv = []
    for m, x in zip(mods, xs):
        bn = m.proj[1]
        lv.append((x, m.proj[0].weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, m.head.weight,
                   m.head.bias, bn.eps, bn.momentum, training))
    return lv


def test_mixed_layout_pyramid_equals_per_level_calls(built_lib):
    from mga_yolo_amd import mask_head_pyramid
    shapes = [(4, 64, 16, 16, 16), (4, 128, 8, 8, 32), (4, 256, 4, 4, 64)]
    fmts = [CL, torch.contiguous_format, CL]
    mods = [_perturbed_head(C_, hid, 30 + i).cuda() for i, (_, C_, _, _, hid) in enumerate(shapes)]
    xs = [torch.randn(B, C_, H, W, generator=torch.Generator().manual_seed(40 + i)).cuda().to(memory_format=f)
          for i, ((B, C_, H, W, _), f) in enumerate(zip(shapes, fmts))]
    gls = [torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(50 + i)).cuda() for i, (B, _, H, W, _) in enumerate(shapes)]
    state0 = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    single = []
    for m, x, gl in zip(mods, xs, gls):
        xd = x.detach().requires_grad_(True)
        y = m(xd)
        y.backward(gl)
        single.append((y.detach(), xd.grad, m.proj[0].weight.grad.clone(), m.head.weight.grad.clone(), m.proj[1].running_var.clone()))
    for m, s in zip(mods, state0):
        m.load_state_dict(s)
        m.zero_grad()
    xds = [x.detach().requires_grad_(True) for x in xs]
    ys = mask_head_pyramid(_levels_of(mods, xds, True))
    torch.autograd.backward(ys, gls)
    for i, (y, xd, m) in enumerate(zip(ys, xds, mods)):
        s = single[i]
        assert torch.equal(y, s[0]) and torch.equal(xd.grad, s[1]), i
        assert torch.equal(m.proj[0].weight.grad, s[2]) and torch.equal(m.head.weight.grad, s[3]) and torch.equal(m.proj[1].running_var, s[4])
        assert _is_cl(xd.grad) == (fmts[i] == CL)
    # eval mode: a sample's logits and gx do not depend on the batch it is in
    for m in mods:
        m.eval()
    xds = [x.detach().requires_grad_(True) for x in xs]
    ys = mask_head_pyramid(_levels_of(mods, xds, False))
    torch.autograd.backward(ys, gls)
    for b in range(xs[0].shape[0]):
        x1 = [x[b:b + 1].detach().clone(memory_format=f).requires_grad_(True) for x, f in zip(xs, fmts)]
        y1 = mask_head_pyramid(_levels_of(mods, x1, False))
        torch.autograd.backward(y1, [g_[b:b + 1] for g_ in gls])
        for i in range(3):
            assert torch.equal(y1[i], ys[i][b:b + 1]) and torch.equal(x1[i].grad, xds[i].grad[b:b + 1]), (b, i)


def _hand_off(fmt, dtype=None, amp=False):
    from mga_yolo_amd import MaskCBAM
    torch.manual_seed(0)
    head, blk = _perturbed_head(64, 16, 60).cuda(), MaskCBAM(64).cuda()
    with torch.no_grad():
        blk.beta.fill_(0.5)
    mods = torch.nn.ModuleDict(dict(head=head, blk=blk, c2=torch.nn.Conv2d(64, 8, 1))).cuda().to(memory_format=fmt)
    x = torch.randn(4, 64, 24, 24, generator=torch.Generator().manual_seed(61)).cuda().to(memory_format=fmt).requires_grad_(True)
    scaler = torch.amp.GradScaler("cuda") if amp else None
    with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
        xin = x.half() if amp else x
        y = blk([xin, head(xin)])
        loss = mods["c2"](y).float().square().mean()
    if amp:
        scaler.scale(loss).backward()
        inv = 1.0 / float(scaler.get_scale())
    else:
        loss.backward()
        inv = 1.0
    grads = {n: p.grad.detach().float() * inv for n, p in mods.named_parameters() if not n.startswith("c2") and p.grad is not None}
    grads["x"] = x.grad.detach().float() * inv
    return float(loss.detach()), grads, x.grad


def test_layer_loop_hand_off_channels_last_fp32(built_lib):
    """head -> [x, logits] -> MaskCBAM, one backward through both (model.py:57-64): channels_last against NCHW within 1e-4."""
    l0, g0, _ = _hand_off(torch.contiguous_format)
    l1, g1, gx = _hand_off(CL)
    assert _is_cl(gx)
    assert abs(l0 - l1) <= 1e-4 * abs(l0)
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 1e-4, n


def test_layer_loop_hand_off_channels_last_amp(built_lib):
    """The same hand-off under AMP fp16 + GradScaler, at the tolerances of test_amp_channels_last_model_matches_nchw."""
    tol = 4e-3
    l0, g0, _ = _hand_off(torch.contiguous_format, amp=True)
    l1, g1, _ = _hand_off(CL, amp=True)
    assert abs(l0 - l1) <= tol * abs(l0)
    for n in g0:
        assert rel_err(g1[n], g0[n]) < 4 * tol, n
