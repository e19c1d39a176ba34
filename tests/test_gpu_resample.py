"""The two resize kernel families element by element on the device:
  a-d. k_resample_fwd / k_resample_bwd (csrc/resample.cuh, include/mgaresample.h) through _binding.fill_resample and the C entry points,
       against tests/resample_oracle.py: every element within K x its own terms, exactly 0.0 where the terms are 0, at the workload's
       ratios, large upsampling, the 65536 limit, workgroup edges, every size pair in 1..40 on either axis, misaligned buffers and
       eight levels in one call;
  e.   k_resize_nearest (csrc/resize.cuh) through functional.resize_nearest, bit-equal to F.interpolate(mode="nearest") on the host and
       to the oracle's index function for every size pair in 1..64 on either axis and at the long axes.
Outputs are pre-filled with NaN and lie inside a larger allocation with 64 sentinel floats on either side; the backward runs twice."""
import os
import sys

import pytest
import torch
import torch.nn.functional as Fnn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as RO  # noqa: E402
from oracle import maskcbam_oracle as O  # noqa: E402
from test_gpu_spade import dev  # noqa: E402,F401  (the module's device fixture)

pytestmark = pytest.mark.gpu
SENT, PAD = -123456.0, 64
NAN = float("nan")


def _starts(sizes, offset):
    """float offsets of tensors of `sizes` elements in one buffer: each start 16-byte aligned (+ `offset` floats), >= PAD floats between"""
    pos, out = PAD, []
    for n in sizes:
        pos = (pos + 3) // 4 * 4 + offset
        out.append(pos)
        pos += n + PAD
    return out, pos


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Guarded:
    """Several output tensors in ONE device allocation: NaN inside, SENT everywhere else."""

    def __init__(self, shapes, offset=0):
        self.shapes = [tuple(s) for s in shapes]
        self.starts, total = _starts([_numel(s) for s in self.shapes], offset)
        self.is_out = torch.zeros(total, dtype=torch.bool)
        for st, s in zip(self.starts, self.shapes):
            self.is_out[st:st + _numel(s)] = True
        init = torch.full((total,), SENT)
        init[self.is_out] = NAN
        self.buf = init.cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.t = [self.buf[st:st + _numel(s)].view(s) for st, s in zip(self.starts, self.shapes)]
        assert all(v.data_ptr() % 16 == 4 * offset for v in self.t)
        self._host = None

    def host(self):
        """the whole buffer on the host (synchronises); -> per-tensor host views"""
        if self._host is None:
            self._host = self.buf.cpu()
        return [self._host[st:st + _numel(s)].view(s) for st, s in zip(self.starts, self.shapes)]

    def intact(self):
        self.host()
        return bool((self._host[~self.is_out] == SENT).all())


def _pack(tensors, offset=0):
    """host tensors -> device views into one upload, each 16-byte aligned (+ `offset` floats)"""
    starts, total = _starts([t.numel() for t in tensors], offset)
    flat = torch.zeros(total)
    for st, t in zip(starts, tensors):
        flat[st:st + t.numel()] = t.reshape(-1)
    d = flat.cuda()
    out = [d[st:st + t.numel()].view(t.shape) for st, t in zip(starts, tensors)]
    assert all(v.data_ptr() % 16 == 4 * offset for v in out)
    return out


def _call(direction, cases, srcs, dsts):
    """one call of the entry point with len(cases) levels; backward: srcs = dL/d(forward dst), dsts = dL/d(forward src)"""
    from mga_yolo_amd import _binding, _lib
    n = len(cases)
    lv = (_lib.ResampleLevel * n)()
    for l, c in enumerate(cases):
        assert srcs[l].shape == (c.B, 1, *(c.in_hw if direction == "forward" else c.out_hw))
        assert dsts[l].shape == (c.B, 1, *(c.out_hw if direction == "forward" else c.in_hw))
        _binding.fill_resample(lv[l], srcs[l], dsts[l], c.in_hw, c.out_hw)
    _binding.call(f"mgaspade_resample_{direction}", srcs[0].device, lv, n)


_refs = {}


def _ref(c):
    """inputs and the oracle's results of a case, computed once: (src, gout, (forward, terms), (backward, terms))"""
    if c not in _refs:
        src, gout = RO.inputs(c)
        op = RO.Resample(c.in_hw, c.out_hw)
        _refs[c] = (src, gout, op.forward(src), op.backward(gout))
    return _refs[c]


def _within(c, dst, gsrc, report):
    """dst, gsrc: host results of case c; appends to `report` what is outside the bar; -> (forward ratio, backward ratio)"""
    kf, kb = RO.load_k()
    _, _, fw, bw = _ref(c)
    rf, _, nzf, badf = RO.ratio(dst, *fw)
    rb, zb, nzb, badb = RO.ratio(gsrc, *bw)
    if badf or badb or nzf or nzb or not rf <= kf or not rb <= kb:
        report.append(dict(case=RO.case_id(c), forward=rf, backward=rb, nonfinite=(badf, badb), nonzero_at_zero_terms=(nzf, nzb), K=(kf, kb)))
    return rf, rb


def _run_one(c, dst_offset=0, src_offset=0):
    """forward, backward and the backward again of one case as single-level calls -> (Guarded of dst, gsrc, gsrc again)"""
    src, gout, _, _ = _ref(c)
    sd, gd = _pack([src, gout], src_offset)
    out = Guarded([(c.B, 1, *c.out_hw), (c.B, 1, *c.in_hw), (c.B, 1, *c.in_hw)], dst_offset)
    _call("forward", [c], [sd], [out.t[0]])
    _call("backward", [c], [gd], [out.t[1]])
    _call("backward", [c], [gd], [out.t[2]])
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# a. the named cases
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RO.NAMED, ids=[f"{c.group}-{RO.case_id(c)}" for c in RO.NAMED])
def test_named_case_element_wise(dev, c):
    out = _run_one(c)
    dst, gsrc, gsrc2 = out.host()
    assert out.intact()
    report = []
    rf, rb = _within(c, dst, gsrc, report)
    kf, kb = RO.load_k()
    print(f"resample {c.group} {RO.case_id(c)}: forward {rf:.3f} (K {kf:.3f}) backward {rb:.3f} (K {kb:.3f})")
    assert not report, report
    assert torch.equal(gsrc, gsrc2)                                           # gather form, fixed order: the same bits
    if c.group == "identity":
        src, gout, _, _ = _ref(c)
        assert torch.equal(dst, src) and torch.equal(gsrc, gout)
    if c.group == "workload":
        assert float((gsrc == 0).double().mean()) >= 0.90


# ------------------------------------------------------------------------------------------------------------------------------------
# b. every size pair in 1..40 on the H axis and, permuted, on the W axis: 200 calls of eight levels each way
# ------------------------------------------------------------------------------------------------------------------------------------
def test_every_small_size_pair_element_wise(dev):
    cases = RO.sweep_cases()
    ins = [RO.inputs(c) for c in cases]
    packed = _pack([t for pair in ins for t in pair])
    srcs, gouts = packed[0::2], packed[1::2]
    dst = Guarded([(c.B, 1, *c.out_hw) for c in cases])
    gsrc = [Guarded([(c.B, 1, *c.in_hw) for c in cases]) for _ in range(2)]
    for k in range(0, len(cases), 8):
        s = slice(k, k + 8)
        _call("forward", cases[s], srcs[s], dst.t[s])
        for g in gsrc:
            _call("backward", cases[s], gouts[s], g.t[s])
    d, g1, g2 = dst.host(), gsrc[0].host(), gsrc[1].host()
    assert dst.intact() and gsrc[0].intact() and gsrc[1].intact()
    kf, kb = RO.load_k()
    report, worst, zeros, total = [], [0.0, None, 0.0, None], 0, 0
    for l, c in enumerate(cases):
        op = RO.Resample(c.in_hw, c.out_hw)
        rf, _, nzf, badf = RO.ratio(d[l], *op.forward(ins[l][0]))
        rb, zb, nzb, badb = RO.ratio(g1[l], *op.backward(ins[l][1]))
        zeros, total = zeros + zb, total + g1[l].numel()
        if badf or badb or nzf or nzb or not rf <= kf or not rb <= kb:
            report.append(dict(case=RO.case_id(c), forward=rf, backward=rb, nonfinite=(badf, badb), nonzero_at_zero_terms=(nzf, nzb)))
        if rf > worst[0]:
            worst[0:2] = [rf, RO.case_id(c)]
        if rb > worst[2]:
            worst[2:4] = [rb, RO.case_id(c)]
    print(f"resample sweep: forward {worst[0]:.3f} at {worst[1]} (K {kf:.3f}) backward {worst[2]:.3f} at {worst[3]} (K {kb:.3f}); "
          f"{zeros} of {total} backward elements have zero terms; {len(report)} of {len(cases)} levels outside")
    assert not report, (len(report), report[:10])
    assert zeros >= 0.05 * total
    assert torch.equal(gsrc[0]._host, gsrc[1]._host)                          # the two runs of the backward: the same bits


# ------------------------------------------------------------------------------------------------------------------------------------
# c. alignment: out_w % 4 == 0 on a destination that is only 4-byte aligned takes the one-pixel path
# ------------------------------------------------------------------------------------------------------------------------------------
def test_misaligned_buffers_give_the_same_bits(dev):
    c = next(k for k in RO.NAMED if (k.in_hw, k.out_hw) == ((9, 7), (5, 12)))
    want = _run_one(c)
    w = want.host()
    report = []
    _within(c, w[0], w[1], report)
    assert not report and want.intact()
    for name, d_off, s_off in (("destination", 1, 0), ("source", 0, 1), ("both", 1, 3)):
        got = _run_one(c, d_off, s_off)
        g = got.host()
        assert got.intact(), name
        for a, b in zip(g, w):
            assert torch.equal(a, b), name


# ------------------------------------------------------------------------------------------------------------------------------------
# d. eight levels in one call: four-pixel and one-pixel levels, levels of one and of several workgroups
# ------------------------------------------------------------------------------------------------------------------------------------
def test_eight_levels_in_one_call(dev):
    from mga_yolo_amd import _lib
    cases = RO.EIGHT
    assert len(cases) == _lib.MAX_LEVELS == 8
    vec = [c.out_hw[1] % 4 == 0 for c in cases]
    assert any(vec) and not all(vec)
    for n in ([c.B * c.out_hw[0] * c.out_hw[1] // (4 if v else 1) for c, v in zip(cases, vec)], [c.B * c.in_hw[0] * c.in_hw[1] for c in cases]):
        assert any(t <= 256 for t in n) and any(t > 512 for t in n)          # threads: one workgroup and several, either direction
        assert any(t <= 256 for t in n[4:]) and any(t > 512 for t in n[4:])  # ... among the last four levels too
    ins = [_ref(c)[:2] for c in cases]
    packed = _pack([t for pair in ins for t in pair])
    srcs, gouts = packed[0::2], packed[1::2]
    dst = Guarded([(c.B, 1, *c.out_hw) for c in cases])
    gsrc = [Guarded([(c.B, 1, *c.in_hw) for c in cases]) for _ in range(2)]
    _call("forward", cases, srcs, dst.t)
    for g in gsrc:
        _call("backward", cases, gouts, g.t)
    single = [_run_one(c) for c in cases]
    d, g1 = dst.host(), gsrc[0].host()
    assert dst.intact() and gsrc[0].intact() and gsrc[1].intact()
    report = []
    for l, c in enumerate(cases):
        rf, rb = _within(c, d[l], g1[l], report)
        print(f"resample eight levels, level {l} {RO.case_id(c)}: forward {rf:.3f} backward {rb:.3f}")
    assert not report, report
    for l, c in enumerate(cases):
        s = single[l].host()
        assert single[l].intact()
        assert torch.equal(d[l], s[0]) and torch.equal(g1[l], s[1]), (l, RO.case_id(c))
    assert torch.equal(gsrc[0]._host, gsrc[1]._host)


# ------------------------------------------------------------------------------------------------------------------------------------
# e. k_resize_nearest: source values are their own index, so a wrong index is a wrong value
# ------------------------------------------------------------------------------------------------------------------------------------
NEAREST_PAIRS = [(a, b) for a in range(1, 65) for b in range(1, 65)] + [(65536, 65535), (65535, 65536), (3, 65536), (65536, 3)]
PLANES, OTHER = 3, (5, 3)        # the other axis: 5 -> 3


@pytest.mark.parametrize("axis", ["h", "w"])
def test_nearest_resize_every_size_pair_bit_exact(dev, axis):
    import mga_yolo_amd.functional as Fn
    assert len(NEAREST_PAIRS) == 4100
    n_max = PLANES * 65536 * max(OTHER)
    assert n_max < 2 ** 24                                                    # every index is an fp32 value
    ramp = torch.arange(n_max, dtype=torch.float32)
    ramp_d = ramp.cuda()
    wrong = []
    for a, b in NEAREST_PAIRS:
        in_hw, out_hw = ((a, OTHER[0]), (b, OTHER[1])) if axis == "h" else ((OTHER[0], a), (OTHER[1], b))
        n = PLANES * in_hw[0] * in_hw[1]
        src = ramp[:n].view(PLANES, 1, *in_hw)                               # value = (plane * in_h + y) * in_w + x
        got = Fn.resize_nearest(ramp_d[:n].view(PLANES, 1, *in_hw), *out_hw).cpu()
        if not (got.shape == (PLANES, 1, *out_hw) and torch.equal(got, Fnn.interpolate(src, size=out_hw, mode="nearest"))
                and torch.equal(got, O.nearest_resize(src, *out_hw))):
            wrong.append((in_hw, out_hw))
    assert not wrong, (len(wrong), wrong[:10])
