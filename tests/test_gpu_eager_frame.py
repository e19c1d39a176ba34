"""The eager frame on the device: one three-level call per block family -- level 0 with an fp16 mask that requires grad, level 1 channels_last
with a mask that does not, level 2 without a mask; the mask head, which has none, varies `training` and num_batches_tracked=None -- against
the same levels run alone through the single-level function.  Per level: which gradients are None, their shapes and element types (dL/dmask
in the mask's own), the memory format of y and dL/dx, and the values.  The bound is the one each family's pyramid-vs-single test already
has: the bits of the level called alone (test_gpu_parity.test_pyramid_call_equals_per_level_calls, test_gpu_eca_nchw, test_gpu_head_nchw,
test_gpu_spade); MaskCBAM's gradients, whose sweeps may regroup with the call's other levels, within test_gpu_bwd_proj's TOL of it."""
import pytest
import torch

from conftest import rel_err
from test_gpu_bwd_proj import TOL as CBAM_REGROUP_TOL
from test_gpu_parity import F  # noqa: F401  (the module's fixture: functional, with the library loaded)

pytestmark = pytest.mark.gpu
SHAPES = [(2, 16, 6, 10), (2, 32, 4, 4), (1, 16, 3, 5)]
NHWC_LEVEL = 1
CL = torch.channels_last
f32 = torch.float32


def _level(Fn, family, l):
    """Seeded leaves of level l -> (x, mask | None, params, buffers, gy, entry of the pyramid call, the single-level call)"""
    g = torch.Generator().manual_seed(100 + l)
    r = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    leaf = lambda t: t.requires_grad_(True)
    B, C, H, W = SHAPES[l]
    x = r(B, C, H, W)
    x = leaf(x.contiguous(memory_format=CL) if l == NHWC_LEVEL else x)
    mask = [lambda: leaf(r(B, 1, H, W).half()), lambda: r(B, 1, H, W), lambda: None][l]()
    gy, buffers = r(B, C, H, W), []                                  # (NCHW for the channels_last level too: converted once)
    if family == "cbam":
        ps = [leaf(t) for t in (r(4, C, scale=0.3), r(4, scale=0.1), r(C, 4, scale=0.3), r(C, scale=0.1), r(1, 3, 7, 7, scale=0.1), r(1).reshape(()))]
        cfg = Fn.BlockConfig(hidden=4, k=7)
        return x, mask, ps, buffers, gy, (x, mask, ps, cfg), lambda: Fn.mask_cbam(x, mask, *ps, cfg)
    if family == "eca":
        ps = [leaf(r(1, 1, 3, scale=0.5)), leaf(r(1).reshape(()))]
        cfg = Fn.EcaConfig(k=3)
        return x, mask, ps, buffers, gy, (x, mask, *ps, cfg), lambda: Fn.mask_eca(x, mask, *ps, cfg)
    if family == "head":
        hid, training = 8, l != 1
        w1, gamma, beta, wh, bh = ps = [leaf(t) for t in (r(hid, C, 1, 1, scale=0.2), 1 + r(hid, scale=0.1), r(hid, scale=0.1), r(1, hid, 3, 3, scale=0.2), r(1))]
        rm, rv, nbt = r(hid, scale=0.1), 1 + r(hid, scale=0.1).abs(), (torch.zeros((), dtype=torch.int64).cuda() if l == 0 else None)
        buffers = [rm, rv] + ([nbt] if nbt is not None else [])
        args = (x, w1, gamma, beta, rm, rv, nbt, wh, bh, 1e-3, 0.03, training)
        return x, None, ps, buffers, r(B, 1, H, W), args, lambda: Fn.mask_head(*args)
    hid = 16
    ps = [leaf(r(*s, scale=0.2)) for s in [(hid, 1, 3, 3), (hid,), (C, hid, 3, 3), (C,), (C, hid, 3, 3), (C,)]]
    cfg = Fn.SpadeConfig(hidden=hid, norm_type="bn" if l == NHWC_LEVEL else "in")
    running = (torch.zeros(C).cuda(), torch.ones(C).cuda(), torch.zeros((), dtype=torch.int64).cuda()) if cfg.bn else None
    buffers = list(running or [])
    return x, mask, ps, buffers, gy, (x, mask, ps, cfg, running), lambda: Fn.mask_spade(x, mask, ps, cfg, running)


def _results(x, mask, ps, buffers, y):
    return [y.detach(), x.grad, None if mask is None else mask.grad] + [p.grad for p in ps] + list(buffers)


@pytest.mark.parametrize("family", ["cbam", "eca", "head", "spade"])
def test_three_level_call_equals_the_levels_alone(F, family):  # noqa: F811
    pyramid = dict(cbam=F.mask_cbam_pyramid, eca=F.mask_eca_pyramid, head=F.mask_head_pyramid, spade=F.mask_spade_pyramid)[family]
    together = [_level(F, family, l) for l in range(len(SHAPES))]
    ys = pyramid([lv[5] for lv in together])
    torch.autograd.backward(list(ys), [lv[4] for lv in together])
    torch.cuda.synchronize()
    for l, ((x, mask, ps, buffers, _, _, _), y) in enumerate(zip(together, ys)):
        fmt = CL if l == NHWC_LEVEL else torch.contiguous_format
        # ---- which gradients came back, in what shape, element type and layout
        assert y.dtype == x.dtype and x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=fmt), l
        if family == "head":
            assert y.shape == (x.shape[0], 1, *x.shape[2:]) and y.is_contiguous()
        else:
            assert y.shape == x.shape and y.is_contiguous(memory_format=fmt), l
            assert (mask is not None and mask.grad is not None) == (l == 0), l           # level 1's mask does not require grad
            if l == 0:
                assert mask.grad.dtype == torch.float16 == mask.dtype and mask.grad.shape == mask.shape
        unread = family == "spade" and mask is None                                      # a MaskSPADE level without a mask reads no parameter
        for p in ps:
            assert (p.grad is None) == unread and (unread or (p.grad.shape == p.shape and p.grad.dtype == f32)), l
        # ---- the values: the same level alone, from the same seeds
        xa, ma, pa, ba, gya, _, single = _level(F, family, l)
        ya = single()
        ya.backward(gya)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(_results(x, mask, ps, buffers, y), _results(xa, ma, pa, ba, ya))):
            assert (a is None) == (b is None), (l, i)
            if a is None:
                continue
            assert a.shape == b.shape and a.dtype == b.dtype and a.stride() == b.stride(), (l, i)
            if family == "cbam" and i > 0:
                e = rel_err(a, b)
                print(f"cbam level {l} output {i}: rel_err {e:.3e}")
                assert e < CBAM_REGROUP_TOL, (l, i, e)
            else:
                assert torch.equal(a, b), (family, l, i)
    if family == "cbam":
        F.handoff_report()                                           # every in-launch hand-off of the calls above completed
