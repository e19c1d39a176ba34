"""fp64 statement of the image batch (include/ext/mgaimage.h) with a per-element error bar, built on the mask resample's oracle.

    source  S = fp64(fp32(v) / fp32(255)): the correctly rounded fp32 quotient of every byte, (B,C,H,W) after the layout and the channel
            order are undone -- they move bytes and change no value.
    no resize   result = S and terms = 0: every output type holds round(S) exactly (fp32: S itself).
    resize      result, terms = resample_oracle.Resample(in_hw, out_hw).forward(S): the separable two-tap operator under the fp32
            coordinate rule, in fp64; the terms are what a correct fp32 implementation may differ by (rounding and a coordinate one ulp
            away).  An element whose terms are 0 has a footprint of zeros: the result there must be exactly 0.0.

A result in a half type is rounded once more: `half_ulp_bar` is half an ulp of that type at a given magnitude."""
import json
import math

import numpy as np
import torch

from resample_oracle import Resample, ratio  # noqa: F401  (ratio: the tests' comparison, re-exported)

import image_cases as IC


def unit(v: torch.Tensor) -> torch.Tensor:
    """fp64(fp32(v) / fp32(255)) of a uint8 tensor, by numpy: one correctly rounded fp32 division"""
    assert v.dtype == torch.uint8
    q = v.cpu().numpy().astype(np.float32) / np.float32(255)
    assert q.dtype == np.float32
    return torch.from_numpy(q.astype(np.float64))


def as_nchw(v: torch.Tensor, src_layout="nchw", reverse_channels=False) -> torch.Tensor:
    v = v.permute(0, 3, 1, 2) if src_layout == "nhwc" else v
    return v.flip(1) if reverse_channels else v


def image(v: torch.Tensor, size=None, src_layout="nchw", reverse_channels=False):
    """-> (result, terms), fp64 (B,C,H',W')"""
    S = unit(as_nchw(v, src_layout, reverse_channels).contiguous())
    if size is None or tuple(size) == tuple(S.shape[2:]):
        return S, torch.zeros_like(S)
    return Resample(tuple(S.shape[2:]), tuple(size)).forward(S)


def rounded(result: torch.Tensor, dtype) -> torch.Tensor:
    """the no-resize result in an output type: fp64 -> fp32 is exact here, then one rounding"""
    f = result.to(torch.float32)
    assert torch.equal(f.double(), result)
    return f.to(dtype)


_MANT = {torch.float32: None, torch.float16: (10, -14), torch.bfloat16: (7, -126)}      # mantissa bits, least normal exponent


def half_ulp_bar(dtype, mag: torch.Tensor) -> torch.Tensor:
    """half an ulp of `dtype` at magnitude `mag` (fp64, >= 0): what the one final rounding may add; 0 for fp32, whose rounding is in the terms"""
    if _MANT[dtype] is None:
        return torch.zeros_like(mag)
    bits, emin = _MANT[dtype]
    e = torch.floor(torch.log2(mag.clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.where(mag > 0, 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - bits), torch.zeros_like(mag))


def within(got: torch.Tensor, result: torch.Tensor, terms: torch.Tensor, K: float, dtype):
    """resample_oracle.ratio of `got` after the allowance for its type's final rounding is taken off every element's difference:
    -> (worst ratio over terms > 0, zero-terms elements, of them not exactly 0.0, non-finite elements).  No element is left out."""
    g = got.detach().double().cpu()
    d = g - result
    bar = half_ulp_bar(dtype, result.abs() + K * terms)
    excess = (d.abs() - bar).clamp_min(0.0)
    finite = torch.isfinite(g)
    adj = torch.where(finite, result + torch.sign(d) * excess, g)
    return ratio(adj, result, terms)


def load_k() -> float:
    """twice torch's own worst ratio over the resize cases, as tools/gen_golden_image.py recorded it"""
    with open(IC.RATIOS) as f:
        return 2.0 * json.load(f)["forward"]


def torch_host(v: torch.Tensor, size) -> torch.Tensor:
    """the composition a user writes, in fp32 on the host"""
    import torch.nn.functional as F
    return F.interpolate(v.float() / 255, size=tuple(size), mode="bilinear", align_corners=False)


def torch_ratio(cases) -> dict:
    """torch's own fp32 host result against the oracle over `cases` (image_cases.Resize) -> dict(forward: worst ratio, zero_terms,
    nonzero_at_zero_terms, elements, per_case)"""
    res = dict(forward=0.0, zero_terms=0, nonzero_at_zero_terms=0, elements=0, per_case={})
    for c in cases:
        v = IC.resize_source(c)
        r, z, nz, bad = ratio(torch_host(v, c.out_hw), *image(v, c.out_hw))
        assert bad == 0 and math.isfinite(r)
        res["forward"] = max(res["forward"], r)
        res["zero_terms"] += z
        res["nonzero_at_zero_terms"] += nz
        res["elements"] += c.B * c.C * c.out_hw[0] * c.out_hw[1]
        res["per_case"][c.name] = r
    return res
