"""tests/resample_oracle.py itself, without a GPU: the fp64 operator against F.interpolate, the gather form against the dense form, the
adjoint identity, torch's own fp32 host run inside the bar the device tests use, and the conditions that keep those tests from passing
vacuously (tests/test_gpu_resample.py)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as RO  # noqa: E402

SMALL = [c for c in RO.NAMED if max(*c.in_hw, *c.out_hw) <= RO.DENSE_MAX]
LONG = [c for c in RO.NAMED if c not in SMALL]


def test_the_case_lists_are_what_the_device_tests_rely_on():
    assert len(RO.NAMED) == len(set(RO.NAMED)) == 27 and len(SMALL) == 21 and all(c.group == "long" for c in LONG)
    sw = RO.sweep_cases()
    assert len(sw) == 1600 and len(sw) % 8 == 0
    assert sorted((c.in_hw[0], c.out_hw[0]) for c in sw) == sorted(RO.SWEEP_PAIRS)       # every pair on the H axis ...
    assert sorted((c.in_hw[1], c.out_hw[1]) for c in sw) == sorted(RO.SWEEP_PAIRS)       # ... and every pair on the W axis
    assert sum((c.in_hw[0], c.out_hw[0]) == (c.in_hw[1], c.out_hw[1]) for c in sw) < 16   # the permutation really mixes the axes
    assert len(RO.EIGHT) == 8
    # forward thread counts at the workgroup edge: 256 and 257 four-pixel threads, 255 and 257 one-pixel threads; backward 255, 256, 257
    edge = [c for c in RO.NAMED if c.group == "wg_edge"]
    assert [c.B * c.out_hw[0] * c.out_hw[1] // 4 for c in edge[:2]] == [256, 257] and all(c.out_hw[1] % 4 == 0 for c in edge[:2])
    assert [c.B * c.out_hw[0] * c.out_hw[1] for c in edge[2:4]] == [255, 257] and all(c.out_hw[1] % 4 for c in edge[2:4])
    assert [c.B * c.in_hw[0] * c.in_hw[1] for c in edge[4:]] == [255, 256, 257]
    assert max(max(*c.in_hw, *c.out_hw) for c in RO.NAMED) == 65536 and max(c.B for c in RO.NAMED) == 300


@pytest.mark.parametrize("c", SMALL, ids=RO.case_id)
def test_fp64_coordinates_equal_interpolate_in_fp64(c):
    src, gout = RO.inputs(c)
    f64, b64 = RO.torch_host(c, src, gout, torch.float64)
    op = RO.Resample(c.in_hw, c.out_hw, coords="fp64")
    fwd, tf = op.forward(src)
    bwd, tb = op.backward(gout)
    assert bool(((fwd - f64).abs() <= 1e-12 * tf / RO.EPS32).all())          # 1e-12 x terms / eps32, element by element
    assert bool(((bwd - b64).abs() <= 1e-12 * tb / RO.EPS32).all())          # (so exactly 0 at the zero-terms elements)


@pytest.mark.parametrize("c", RO.NAMED, ids=RO.case_id)
def test_gather_form_equals_dense_form_and_adjoint_identity(c):
    """<R s, g> == <s, R^T g> in fp64; below the dense limit the gather form (the only one the long axes have) equals the dense one."""
    src, gout = RO.inputs(c)
    op = RO.Resample(c.in_hw, c.out_hw)
    fwd, tf = op.forward(src)
    bwd, tb = op.backward(gout)
    lhs, rhs = float((fwd * gout.double()).sum()), float((src.double() * bwd).sum())
    scale = float((fwd.abs() * gout.double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale
    if c in SMALL:
        assert op.y.dense and op.x.dense
        og = RO.Resample(c.in_hw, c.out_hw, dense=False)
        for a, b in zip(op.forward(src) + op.backward(gout), og.forward(src) + og.backward(gout)):
            assert bool(((a - b).abs() <= 1e-13 * a.abs().max().clamp_min(1e-300)).all())
        assert torch.equal(tf == 0, og.forward(src)[1] == 0) and torch.equal(tb == 0, og.backward(gout)[1] == 0)
    else:
        assert not (op.y.dense and op.x.dense)


@pytest.fixture(scope="module")
def torch_named():
    return RO.torch_ratios(RO.NAMED)


@pytest.fixture(scope="module")
def torch_sweep():
    return RO.torch_ratios(RO.sweep_cases())


def test_torch_fp32_host_run_stays_within_k(torch_named, torch_sweep):
    """K = 2 x the recorded worst ratio of torch's fp32 host run; the run is repeated on this machine (its CPU may vectorise differently)."""
    kf, kb = RO.load_k()
    with open(RO.RATIOS) as f:
        rec = json.load(f)
    for name, r in (("named", torch_named), ("sweep", torch_sweep)):
        print(f"torch fp32 host, {name}: forward {r['forward']:.3f} (K {kf:.3f}) backward {r['backward']:.3f} (K {kb:.3f}) "
              f"zero-terms {r['zero_terms']} of {r['elements']}; recorded {rec['forward']:.3f} / {rec['backward']:.3f}")
        assert r["forward"] <= kf and r["backward"] <= kb
        assert r["nonzero_at_zero_terms"] == 0                               # torch itself is exactly 0 where the terms are
    assert rec["forward"] > 0 and rec["backward"] > 0


def test_the_device_tests_cannot_pass_vacuously(torch_sweep):
    """From the oracle alone: at least 90 % of the backward's elements in the workload's three downsampling cases are zero-terms elements
    (they must be exactly 0.0 on the device), in the sweep at least 5 %; every other element has a positive, finite bar, so ratio()
    leaves no element out of a comparison.  At a ratio r per axis two of r source indices carry a weight and four an entry of U, so
    1 - 12 / r^2 of a case's elements have zero terms (81.25 % at 8x, 95.3 % at 16x, 98.8 % at 32x: 92.3 % of the three cases' elements)
    and 1 - 4 / r^2 >= 93.75 % of each case's results are exactly 0."""
    zero = total = 0
    for c, r in zip(RO.WORKLOAD, (8, 16, 32)):
        src, gout = RO.inputs(c)
        op = RO.Resample(c.in_hw, c.out_hw)
        bwd, tb = op.backward(gout)
        _, tf = op.forward(src)
        assert int((tb == 0).sum()) * r * r == tb.numel() * (r * r - 12), c
        assert int((bwd == 0).sum()) * r * r == bwd.numel() * (r * r - 4) and float((bwd == 0).double().mean()) >= 0.90, c
        assert bool((bwd[tb == 0] == 0).all())
        assert bool((tf > 0).all()) and bool(torch.isfinite(tf).all()) and bool(torch.isfinite(tb).all())
        zero, total = zero + int((tb == 0).sum()), total + tb.numel()
    assert zero >= 0.90 * total
    assert torch_sweep["zero_terms"] >= 0.05 * torch_sweep["elements"]
    # ratio() itself: a NaN is counted and makes the ratio infinite, a non-zero at a zero-terms element is counted
    ref, terms = torch.tensor([1.0, 0.0, 2.0]), torch.tensor([1e-7, 0.0, 1e-7])
    assert RO.ratio(torch.tensor([1.0, 0.0, 2.0]), ref, terms) == (0.0, 1, 0, 0)
    assert RO.ratio(torch.tensor([1.0, 1e-30, 2.0]), ref, terms)[2] == 1
    r = RO.ratio(torch.tensor([float("nan"), 0.0, 2.0]), ref, terms)
    assert r[0] == float("inf") and r[3] == 1
    assert RO.ratio(torch.tensor([1.0, float("nan"), 2.0]), ref, terms)[2:] == (1, 1)
