"""fp64 restatement of MaskSPADE (mga_yolo/nn/modules/masked_spade.py) with a hand-derived backward: no autograd anywhere.

    s = sigmoid(m) | m (bilinearly resampled first when its size differs),  pre = conv3x3(s; w0) + b0,  h = relu(pre)
    gamma = conv3x3(h; wg) + bg,  beta = conv3x3(h; wb) + bb,  y = gamma * xhat + beta,  xhat = (x - mean) * rstd
    instance norm: mean / biased variance per (b,c); batch norm: per c over (B,H,W) in training (running statistics updated with the
    unbiased variance), the running statistics in eval.

The tests compare it with every stored fixture (tests/golden/spade_*.npz, written from the reference's own class) on the CPU and use it
as the live reference of the device kernels at the sizes no fixture can hold.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

PARAM_KEYS = ("shared.0.weight", "shared.0.bias", "conv_gamma.weight", "conv_gamma.bias", "conv_beta.weight", "conv_beta.bias")


def _wgrad(g: torch.Tensor, inp: torch.Tensor) -> torch.Tensor:
    """dW[c,j,t] = sum_{b,p} g[b,c,p] * inp[b,j,p+t] for a 3x3, pad-1 convolution."""
    B, J, H, W = inp.shape
    out = torch.zeros(g.shape[1], J, 9, dtype=inp.dtype)
    for b in range(B):                                     # sample by sample: the unfolded planes of a training-size batch are GBs
        cols = F.unfold(inp[b:b + 1], 3, padding=1).reshape(J, 9, H * W)
        out += torch.einsum("cp,jtp->cjt", g[b].reshape(g.shape[1], H * W), cols)
    return out.reshape(g.shape[1], J, 3, 3)


def forward(x, mask, params, norm_type="in", training=True, use_sigmoid=True, eps=1e-6, running=None, momentum=0.1):
    """-> (y, ctx).  params: dict with PARAM_KEYS; running: (mean, var) for batch norm.  Everything is computed in float64."""
    d = torch.float64
    x = x.to(d)
    B, C, H, W = x.shape
    bn = norm_type.lower() == "bn"
    new_running = None
    if not bn:
        mean = x.mean(dim=(2, 3), keepdim=True)
        var = x.var(dim=(2, 3), unbiased=False, keepdim=True)
        mode = "in"
    elif training:
        mean = x.mean(dim=(0, 2, 3), keepdim=True)
        var = x.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        n = B * H * W
        rm, rv = running
        new_running = ((1 - momentum) * rm.to(d) + momentum * mean.flatten(), (1 - momentum) * rv.to(d) + momentum * var.flatten() * n / (n - 1))
        mode = "bn_train"
    else:
        mean = running[0].to(d).view(1, C, 1, 1)
        var = running[1].to(d).view(1, C, 1, 1)
        mode = "bn_eval"
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    ctx = dict(mode=mode, xhat=xhat, rstd=rstd, new_running=new_running)
    if mask is None:
        return xhat, ctx
    m = mask.to(d)
    if m.dim() == 3:
        m = m.unsqueeze(1)
    m_in = m
    if tuple(m.shape[-2:]) != (H, W):
        m = F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)
    s = torch.sigmoid(m) if use_sigmoid else m
    p = {k: v.to(d) for k, v in params.items()}
    pre = F.conv2d(s, p["shared.0.weight"], p["shared.0.bias"], padding=1)
    h = torch.relu(pre)
    gamma = F.conv2d(h, p["conv_gamma.weight"], p["conv_gamma.bias"], padding=1)
    beta = F.conv2d(h, p["conv_beta.weight"], p["conv_beta.bias"], padding=1)
    ctx.update(s=s, pre=pre, h=h, gamma=gamma, p=p, use_sigmoid=use_sigmoid, m_in_shape=tuple(m_in.shape), mask_shape=tuple(mask.shape))
    return gamma * xhat + beta, ctx


def backward(gy, ctx):
    """-> dict(gx, [gmask, g<param key>...]).  Also 'relu_edge': per-gradient bounds of what pre-activations with |pre| < 1e-5 could move."""
    d = torch.float64
    gy = gy.to(d)
    xhat, rstd, mode = ctx["xhat"], ctx["rstd"], ctx["mode"]
    out = {}
    has_mask = "gamma" in ctx
    g_xhat = gy * ctx["gamma"] if has_mask else gy
    if mode == "bn_eval":
        out["gx"] = g_xhat * rstd
    else:
        dims = (2, 3) if mode == "in" else (0, 2, 3)
        m1 = g_xhat.mean(dim=dims, keepdim=True)
        m2 = (g_xhat * xhat).mean(dim=dims, keepdim=True)
        out["gx"] = rstd * (g_xhat - m1 - xhat * m2)
    if not has_mask:
        return out
    p, h, pre, s = ctx["p"], ctx["h"], ctx["pre"], ctx["s"]
    g_gamma, g_beta = gy * xhat, gy
    out["conv_gamma.weight"] = _wgrad(g_gamma, h)
    out["conv_beta.weight"] = _wgrad(g_beta, h)
    out["conv_gamma.bias"] = g_gamma.sum(dim=(0, 2, 3))
    out["conv_beta.bias"] = g_beta.sum(dim=(0, 2, 3))
    dh = F.conv_transpose2d(g_gamma, p["conv_gamma.weight"], padding=1) + F.conv_transpose2d(g_beta, p["conv_beta.weight"], padding=1)
    ctx["dh"] = dh                                          # (relu_edge reuses it)
    dpre = dh * (pre > 0)
    out["shared.0.weight"] = _wgrad(dpre, s)
    out["shared.0.bias"] = dpre.sum(dim=(0, 2, 3))
    ds = F.conv_transpose2d(dpre, p["shared.0.weight"], padding=1)
    gm = ds * s * (1 - s) if ctx["use_sigmoid"] else ds
    H, W = gy.shape[-2:]
    if ctx["m_in_shape"][-2:] != (H, W):                   # adjoint of the bilinear resample: it is linear, so its matrix transposed
        hi, wi = ctx["m_in_shape"][-2:]
        eye = torch.eye(hi * wi, dtype=d).reshape(hi * wi, 1, hi, wi)
        R = F.interpolate(eye, size=(H, W), mode="bilinear", align_corners=False).reshape(hi * wi, H * W)
        gm = (gm.reshape(gm.shape[0], 1, H * W) @ R.t()).reshape(gm.shape[0], 1, hi, wi)
    out["gmask"] = gm.reshape(ctx["mask_shape"])
    return out


def reference_form(x, mask, params, norm_type="in", training=True, use_sigmoid=True, eps=1e-6, running=None, momentum=0.1):
    """The block as the differentiable eager-op sequence the reference executes, one op per line of masked_spade.py, in the dtype of x.
    running: (mean, var) of a batch norm, updated in place as F.batch_norm does.  Unlike forward / backward above it goes through autograd,
    so it says what torch's own operators do with a non-finite value."""
    if norm_type.lower() == "bn":                                                            # masked_spade.py:73, 122
        x_hat = F.batch_norm(x, running[0], running[1], None, None, training, momentum, eps)
    else:                                                                                    # masked_spade.py:75, 122
        x_hat = F.instance_norm(x, None, None, None, None, True, 0.1, eps)
    if mask is None:                                                                         # masked_spade.py:124-126
        return x_hat
    if mask.dim() == 3:                                                                      # masked_spade.py:103-104
        mask = mask.unsqueeze(1)
    if tuple(mask.shape[-2:]) != tuple(x.shape[-2:]):                                        # masked_spade.py:107-108
        mask = F.interpolate(mask, size=tuple(x.shape[-2:]), mode="bilinear", align_corners=False)
    if use_sigmoid:                                                                          # masked_spade.py:109-110
        mask = mask.sigmoid()
    h = F.relu(F.conv2d(mask, params["shared.0.weight"], params["shared.0.bias"], padding=1))      # masked_spade.py:131
    gamma = F.conv2d(h, params["conv_gamma.weight"], params["conv_gamma.bias"], padding=1)         # masked_spade.py:132
    beta = F.conv2d(h, params["conv_beta.weight"], params["conv_beta.bias"], padding=1)            # masked_spade.py:133
    return gamma * x_hat + beta                                                                     # masked_spade.py:138


def reference_form_step(x, mask, params, gy, norm_type="in", training=True, use_sigmoid=True, eps=1e-6, running=None, momentum=0.1):
    """One forward + backward of the eager form through autograd -> (y, dict(gx, [gmask, g<param key>...], [running_mean, running_var]))
    with backward()'s keys.  Nothing given is written to: the running statistics are cloned first."""
    xr = x.detach().clone().requires_grad_(True)
    mr = None if mask is None else mask.detach().clone().requires_grad_(True)
    leaves = {k: params[k].detach().clone().requires_grad_(True) for k in PARAM_KEYS}
    run = None if running is None else tuple(t.detach().clone() for t in running[:2])
    y = reference_form(xr, mr, leaves, norm_type, training, use_sigmoid, eps, run, momentum)
    y.backward(gy)
    out = {"gx": xr.grad}
    if mr is not None:
        out["gmask"] = mr.grad
        out.update({k: v.grad for k, v in leaves.items()})
    if run is not None:
        out["running_mean"], out["running_var"] = run
    return y.detach(), out


def min_abs_pre(ctx) -> float:
    return float(ctx["pre"].abs().min())


def relu_edge(gy, ctx, thr=1e-5):
    """Pre-activations with |pre| < thr may take the other ReLU branch on the device.  Returns (share of h they are, widen) where
    widen[name] bounds, per gradient, the sum of those elements' own contributions (each could appear or vanish)."""
    d = torch.float64
    gy = gy.to(d)
    pre, s, p, xhat = ctx["pre"], ctx["s"], ctx["p"], ctx["xhat"]
    edge = (pre.abs() < thr)
    share = float(edge.double().mean())
    widen = {k: 0.0 for k in ("gx", "gmask") + PARAM_KEYS}
    if not edge.any():
        return share, widen
    dh = ctx.get("dh")
    if dh is None:
        g_gamma, g_beta = gy * xhat, gy
        dh = F.conv_transpose2d(g_gamma, p["conv_gamma.weight"], padding=1) + F.conv_transpose2d(g_beta, p["conv_beta.weight"], padding=1)
    de = (dh * edge).abs()                                  # what flips in dpre
    widen["shared.0.bias"] = float(de.sum(dim=(0, 2, 3)).max())
    widen["shared.0.weight"] = float(_wgrad(de, s.abs()).max())
    widen["gmask"] = float(F.conv_transpose2d(de, p["shared.0.weight"].abs(), padding=1).max())   # (times s(1-s) <= 1)
    return share, widen
