"""fp64 statement of the mask resample (include/mgaresample.h, csrc/resample.cuh) with a per-element error bar, and the cases the tests run.

    F.interpolate(mode="bilinear", align_corners=False) of (B,1,in_h,in_w) to (B,1,out_h,out_w) is separable: per axis a matrix R
    (n_out x n_in) with two taps per row,
        scale = f32(n_in) / f32(n_out),  f = max(scale * (j + 0.5) - 0.5, 0),  i0 = min(int(f), n_in - 1),  i1 = i0 + (i0 < n_in - 1),
        lam = f - i0,  R[j, i0] += 1 - lam,  R[j, i1] += lam
    -- the header's "fp32 coordinate rule", evaluated here in numpy fp32 one operation at a time (no FMA) and promoted to fp64.
        forward : D = Ry . S . Rx^T          backward: dS = Ry^T . G . Rx
    both in fp64.  Axes up to DENSE_MAX use dense matrices; longer ones gather / index_add_ (a dense 65536 x 65536 operator is 34 GB).

Every element has a bar K x terms(element).  The terms are what a correct fp32 implementation may differ by:
    rounding  : eps32 . (|Ry| . |S| . |Rx|^T)                     (backward: eps32 . (|Ry|^T . |G| . |Rx|))
    coordinate: the fp32 coordinate may come out one ulp of f + 0.5 away (an FMA contraction of scale * (j + 0.5) - 0.5, torch's variants)
      forward : ulp(f + 0.5) x the largest |difference of neighbouring source values| over the segments [k, k + 1], k in {i0 - 1, i0, i1}
                (clipped to the axis), interpolated by the other axis with |weights|;
      backward: U (n_out x n_in) holds ulp(f_j + 0.5) at (j, i) for i in {i0 - 1, i0, i1, i1 + 1} (clipped; empty when n_in == 1), and the
                term is Uy^T |G| |Rx| + |Ry|^T |G| Ux.
An element whose terms are 0 has no destination anywhere near it: the result there must be exactly 0.0.  K is twice the worst ratio
|torch's own fp32 host result - oracle| / terms over the cases below (tools/gen_resample_ratios.py -> tests/golden/resample_ratios.json).

coords="fp64" evaluates the same formulas in double; it exists only to pin this file against F.interpolate in fp64."""
from __future__ import annotations

import json
import os
from collections import namedtuple

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)        # 2^-23
DENSE_MAX = 2048
RATIOS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_ratios.json")


# ------------------------------------------------------------------------------------------------------------------------------------
# one axis
# ------------------------------------------------------------------------------------------------------------------------------------
class Axis:
    """The taps of one axis.  i0, i1: int64 (n_out); w0, w1: fp64 weights 1 - lam, lam; ulp: fp64 ulp of fp32(f + 0.5)."""

    def __init__(self, n_in: int, n_out: int, coords: str = "fp32", dense=None):
        assert coords in ("fp32", "fp64") and n_in >= 1 and n_out >= 1
        ft = np.float32 if coords == "fp32" else np.float64
        scale = ft(n_in) / ft(n_out)
        j = np.arange(n_out, dtype=ft)
        f = scale * (j + ft(0.5))                 # one numpy operation per line: no contraction
        f = f - ft(0.5)
        f = np.maximum(f, ft(0))
        i0 = np.minimum(f.astype(np.int64), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        lam = (f - i0.astype(ft)).astype(np.float64)
        self.n_in, self.n_out = n_in, n_out
        self.i0, self.i1 = torch.from_numpy(i0), torch.from_numpy(i1)
        self.w0, self.w1 = torch.from_numpy(1.0 - lam), torch.from_numpy(lam)
        self.ulp = torch.from_numpy(np.spacing((f.astype(np.float32) + np.float32(0.5))).astype(np.float64))
        self.dense = (max(n_in, n_out) <= DENSE_MAX) if dense is None else dense
        self._mats = {}

    # the three operators of the axis as lists of (index, weight): every row j has weight[j] at column index[j]
    def taps(self, kind: str):
        if kind == "R":
            return [(self.i0, self.w0), (self.i1, self.w1)]
        if kind == "absR":
            return [(self.i0, self.w0.abs()), (self.i1, self.w1.abs())]
        assert kind == "U"
        if self.n_in == 1:
            return []
        last = self.n_in - 1
        cand = [(self.i0 - 1, self.i0 >= 1), (self.i0, torch.ones_like(self.i0, dtype=torch.bool)), (self.i1, self.i1 != self.i0),
                (self.i1 + 1, self.i1 + 1 <= last)]       # four distinct columns where valid: a set, nothing counted twice
        return [(i.clamp(0, last), self.ulp * ok) for i, ok in cand]

    def matrix(self, kind: str) -> torch.Tensor:
        if kind not in self._mats:
            M = torch.zeros(self.n_out, self.n_in, dtype=torch.float64)
            rows = torch.arange(self.n_out)
            for idx, w in self.taps(kind):
                M.index_put_((rows, idx), w, accumulate=True)
            self._mats[kind] = M
        return self._mats[kind]

    def apply(self, kind: str, T: torch.Tensor, dim: int) -> torch.Tensor:
        """M . T along dim (-2 or -1): n_in -> n_out"""
        assert dim in (-2, -1) and T.shape[dim] == self.n_in and T.dtype == torch.float64
        if self.dense:
            return self.matrix(kind) @ T if dim == -2 else T @ self.matrix(kind).t()
        shape = list(T.shape)
        shape[dim] = self.n_out
        out = torch.zeros(shape, dtype=torch.float64)
        for idx, w in self.taps(kind):
            out += T.index_select(dim, idx) * (w.unsqueeze(-1) if dim == -2 else w)
        return out

    def apply_t(self, kind: str, T: torch.Tensor, dim: int) -> torch.Tensor:
        """M^T . T along dim: n_out -> n_in"""
        assert dim in (-2, -1) and T.shape[dim] == self.n_out and T.dtype == torch.float64
        if self.dense:
            return self.matrix(kind).t() @ T if dim == -2 else T @ self.matrix(kind)
        shape = list(T.shape)
        shape[dim] = self.n_in
        out = torch.zeros(shape, dtype=torch.float64)
        for idx, w in self.taps(kind):
            out.index_add_(dim, idx, T * (w.unsqueeze(-1) if dim == -2 else w))
        return out

    def slope(self, S: torch.Tensor, dim: int) -> torch.Tensor:
        """per destination index j along dim: ulp(f_j + 0.5) x max |S[k + 1] - S[k]| over k in {i0 - 1, i0, i1}, 0 <= k <= n_in - 2"""
        shape = list(S.shape)
        shape[dim] = self.n_out
        out = torch.zeros(shape, dtype=torch.float64)
        if self.n_in == 1:
            return out
        d = S.diff(dim=dim).abs()
        for k in (self.i0 - 1, self.i0, self.i1):
            ok = ((k >= 0) & (k <= self.n_in - 2)).to(torch.float64)
            v = d.index_select(dim, k.clamp(0, self.n_in - 2)) * (ok.unsqueeze(-1) if dim == -2 else ok)
            out = torch.maximum(out, v)
        return out * (self.ulp.unsqueeze(-1) if dim == -2 else self.ulp)


# ------------------------------------------------------------------------------------------------------------------------------------
# the operator
# ------------------------------------------------------------------------------------------------------------------------------------
class Resample:
    def __init__(self, in_hw, out_hw, coords: str = "fp32", dense=None):
        self.in_hw, self.out_hw = tuple(in_hw), tuple(out_hw)
        self.y = Axis(in_hw[0], out_hw[0], coords, dense)
        self.x = Axis(in_hw[1], out_hw[1], coords, dense)

    def _both(self, ky, kx, T, t=False):
        if t:
            return self.x.apply_t(kx, self.y.apply_t(ky, T, -2), -1)
        return self.x.apply(kx, self.y.apply(ky, T, -2), -1)

    def forward(self, src: torch.Tensor):
        """src (B,1,in_h,in_w) -> (fp64 result, fp64 terms), both (B,1,out_h,out_w)"""
        S = src.detach().double().cpu()
        assert tuple(S.shape[-2:]) == self.in_hw
        out = self._both("R", "R", S)
        terms = EPS32 * self._both("absR", "absR", S.abs())
        terms = terms + self.y.apply("absR", self.x.slope(S, -1), -2) + self.x.apply("absR", self.y.slope(S, -2), -1)
        return out, terms

    def backward(self, gout: torch.Tensor):
        """gout (B,1,out_h,out_w) -> (fp64 dL/dsrc, fp64 terms), both (B,1,in_h,in_w)"""
        G = gout.detach().double().cpu()
        assert tuple(G.shape[-2:]) == self.out_hw
        out = self._both("R", "R", G, t=True)
        A = G.abs()
        terms = EPS32 * self._both("absR", "absR", A, t=True)
        terms = terms + self._both("U", "absR", A, t=True) + self._both("absR", "U", A, t=True)
        return out, terms


def ratio(got: torch.Tensor, ref: torch.Tensor, terms: torch.Tensor):
    """-> (max |got - ref| / terms over the elements with terms > 0 (0.0 when there are none), number of zero-terms elements, number of
    zero-terms elements where got is not exactly 0.0, number of non-finite elements of got).  Every element is in one of the two sets."""
    got = got.detach().double().cpu().reshape(-1)
    ref, terms = ref.reshape(-1), terms.reshape(-1)
    assert got.shape == ref.shape == terms.shape and bool((terms >= 0).all())
    zero = terms == 0
    live = ~zero
    assert int(zero.sum()) + int(live.sum()) == got.numel()
    bad = int((~torch.isfinite(got)).sum())
    r = float(((got[live] - ref[live]).abs() / terms[live]).nan_to_num(nan=float("inf")).max()) if bool(live.any()) else 0.0
    return r, int(zero.sum()), int((got[zero] != 0.0).sum()), bad


def load_k():
    """-> (K forward, K backward): twice torch's own worst ratio, as tools/gen_resample_ratios.py recorded it"""
    with open(RATIOS) as f:
        z = json.load(f)
    return 2.0 * z["forward"], 2.0 * z["backward"]


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "group B in_hw out_hw")


def _c(group, in_hw, out_hw, B=2):
    return Case(group, B, tuple(in_hw), tuple(out_hw))


WORKLOAD = [_c("workload", (64, 64), (8, 8)), _c("workload", (64, 96), (4, 6)), _c("workload", (64, 64), (2, 2))]
NAMED = WORKLOAD + [
    _c("upsample", (3, 5), (200, 300)), _c("upsample", (1, 1), (37, 41)), _c("upsample", (2, 3), (1, 1024)),
    _c("nondyadic", (100, 76), (33, 95)), _c("nondyadic", (33, 95), (100, 76)),
    _c("identity", (12, 20), (12, 20)),
    _c("out_w_mod4", (9, 7), (5, 12)), _c("out_w_mod4", (9, 7), (5, 13)), _c("out_w_mod4", (9, 7), (5, 14)), _c("out_w_mod4", (9, 7), (5, 15)),
    # thread counts at a workgroup (256 threads) edge, B = 1: forward 256 and 257 four-pixel threads, 255 and 257 one-pixel threads
    _c("wg_edge", (5, 9), (16, 64), 1), _c("wg_edge", (3, 300), (1, 1028), 1), _c("wg_edge", (6, 40), (17, 15), 1), _c("wg_edge", (100, 3), (257, 1), 1),
    # ... and backward sources of 255, 256 and 257 elements
    _c("wg_edge", (15, 17), (7, 30), 1), _c("wg_edge", (16, 16), (40, 5), 1), _c("wg_edge", (1, 257), (3, 100), 1),
    _c("batch", (3, 3), (5, 4), 300),
    _c("long", (1, 65536), (1, 65535), 1), _c("long", (1, 65535), (1, 65536), 1), _c("long", (1, 65536), (1, 3), 1),
    _c("long", (1, 3), (1, 65536), 1), _c("long", (65536, 1), (7, 1), 1), _c("long", (1, 4099), (1, 65536), 1),
]
EIGHT = [_c("eight", a, b) for a, b in [((9, 7), (5, 12)), ((100, 76), (33, 95)), ((1, 1), (37, 41)), ((3, 5), (200, 300)), ((33, 95), (100, 76)),
                                        ((64, 64), (8, 8)), ((12, 20), (12, 20)), ((2, 3), (1, 1024))]]     # section d of the GPU tests

SWEEP_N = 40
SWEEP_PAIRS = [(a, b) for a in range(1, SWEEP_N + 1) for b in range(1, SWEEP_N + 1)]


def sweep_cases():
    """All 1600 (in, out) pairs in 1..40 on the H axis and, through the fixed permutation k -> (773 k + 311) mod 1600, on the W axis."""
    n = len(SWEEP_PAIRS)
    out = []
    for k, (a, b) in enumerate(SWEEP_PAIRS):
        c, d = SWEEP_PAIRS[(773 * k + 311) % n]
        out.append(_c("sweep", (a, c), (b, d)))
    return out


def case_id(c: Case) -> str:
    return f"{c.in_hw[0]}x{c.in_hw[1]}-{c.out_hw[0]}x{c.out_hw[1]}-b{c.B}"


def inputs(c: Case, seed: int = 0):
    """-> (src (B,1,*in_hw), gout (B,1,*out_hw)) fp32 randn, a function of the case and the seed alone"""
    s = (seed * 1000003 + c.B * 7919 + c.in_hw[0] * 104729 + c.in_hw[1] * 1299709 + c.out_hw[0] * 15485863 + c.out_hw[1] * 32452843) % (2 ** 31)
    g = torch.Generator().manual_seed(s)
    return torch.randn(c.B, 1, *c.in_hw, generator=g), torch.randn(c.B, 1, *c.out_hw, generator=g)


def torch_host(c: Case, src, gout, dtype=torch.float32):
    """F.interpolate and its autograd on the host in `dtype` -> (forward, backward)"""
    import torch.nn.functional as F
    s = src.detach().clone().to(dtype).requires_grad_(True)
    d = F.interpolate(s, size=c.out_hw, mode="bilinear", align_corners=False)
    d.backward(gout.to(dtype))
    return d.detach(), s.grad


def torch_ratios(cases):
    """torch's own fp32 host run against the oracle over `cases` -> dict(forward, backward: worst ratios; zero_terms, elements: of the
    backward; nonzero_at_zero_terms: elements where torch is not exactly 0 although the terms are; per group the two worst ratios)"""
    res = dict(forward=0.0, backward=0.0, zero_terms=0, elements=0, nonzero_at_zero_terms=0, groups={})
    for c in cases:
        src, gout = inputs(c)
        op = Resample(c.in_hw, c.out_hw)
        f32, b32 = torch_host(c, src, gout)
        rf, _, nzf, badf = ratio(f32, *op.forward(src))
        rb, zb, nzb, badb = ratio(b32, *op.backward(gout))
        assert badf == 0 and badb == 0
        res["forward"], res["backward"] = max(res["forward"], rf), max(res["backward"], rb)
        res["zero_terms"] += zb
        res["elements"] += gout.shape[0] * c.in_hw[0] * c.in_hw[1]
        res["nonzero_at_zero_terms"] += nzf + nzb
        g = res["groups"].setdefault(c.group, [0.0, 0.0])
        g[0], g[1] = max(g[0], rf), max(g[1], rb)
    return res
