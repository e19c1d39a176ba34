"""The image batch on the device (include/ext/mgaimage.h, mga_yolo_amd/image.py), at the smallest shapes at which each piece can go wrong
(tests/image_cases.py says what each is built for).

  no resize   torch.equal with the torch composition computed on the device in the same test -- v.to(dtype) / 255, which the device
              evaluates as a product with the fp32 reciprocal -- in fp32, fp16 and bf16, for both destination layouts, both source layouts,
              with and without the channel reversal; sources that start 1 and 3 bytes into their buffer; destinations that start one to
              three elements into theirs, inside a band of a sentinel value.
  resize      every element against the fp64 oracle (tests/image_oracle.py): |got - oracle| <= K x terms, K twice torch's own recorded worst
              ratio, plus half an ulp of a half output type for its one final rounding; exactly 0.0 where the terms are 0; no element left out.
  ImagePlan   eager run() and three replays of a captured graph with fresh bytes, bit-equal to image_batch.
  Every configuration runs twice on the same bytes: equal bits."""
import itertools

import pytest
import torch

import image_cases as IC
import image_oracle as IO
from mga_yolo_amd import ImagePlan, image_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
K = IO.load_k()
SENTINEL = -7.5


def _torch(v, dt, layout, rev):
    """the composition a user writes, on the device: (B,C,H,W) in dt"""
    return IO.as_nchw(v, layout, rev).to(dt) / 255


def _as(src, layout):
    return src.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else src


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


FORMS = list(itertools.product((False, True), ("nchw", "nhwc"), (False, True)))       # channels_last, src_layout, reverse


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("c", IC.PLAIN, ids=[c.name for c in IC.PLAIN])
def test_no_resize_equals_the_torch_composition(c, dt):
    src = IC.plain_source(c).to(DEV)
    for cl, layout, rev in FORMS:
        v = _as(src, layout)
        want = _torch(v, dt, layout, rev)
        got = image_batch(v, dtype=dt, channels_last=cl, src_layout=layout, reverse_channels=rev)
        assert got.dtype == dt and tuple(got.shape) == c.shape, (cl, layout, rev)
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        assert same_bits(got, want), (cl, layout, rev)
        assert same_bits(image_batch(v, dtype=dt, channels_last=cl, src_layout=layout, reverse_channels=rev), got)      # a second call: the same bits


def test_all_256_bytes_quotient_and_device_product():
    """On the device torch evaluates `x / 255` as x * (1.0f / 255.0f): the no-resize result equals that composition (the test above), which in
    fp16 and bf16 is the oracle's rounded quotient for all 256 bytes and in fp32 is one ulp away from it for 126 of them.  Measured on an
    MI355X: device composition against the host's 126 / 0 / 0 differing bytes in fp32 / fp16 / bf16, against the fp32 product 0 / 0 / 0."""
    v = IC.source(None, ramp=True).to(DEV)
    quotient = IO.image(v.cpu())[0]
    for dt in (torch.float16, torch.bfloat16):
        assert same_bits(image_batch(v, dtype=dt).cpu(), IO.rounded(quotient, dt)), dt
    got = image_batch(v).cpu()
    product = v.cpu().float() * torch.tensor(1.0, dtype=torch.float32).div(255.0)
    assert same_bits(got, product)
    ulps = (_bits(got).long() - _bits(IO.rounded(quotient, torch.float32)).long()).abs()
    assert int(ulps.max()) == 1 and int((ulps != 0).sum()) == 126


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("name", ["odd5x3", "c4_7x15", "wide70x130"])
def test_offset_sources_and_destinations_inside_a_guard_band(name, dt):
    c = IC.PLAIN_BY_NAME[name]
    src = IC.plain_source(c).to(DEV)
    n = src.numel()
    band = 64
    for (cl, layout, rev), s_off, d_off in itertools.product(FORMS, (1, 3), (1, 2, 3)):
        v = _as(src, layout)
        raw = torch.zeros(n + 8, dtype=torch.uint8, device=DEV)
        view = raw[s_off:s_off + n].view(v.shape)
        view.copy_(v)
        assert view.data_ptr() == raw.data_ptr() + s_off and view.is_contiguous()
        buf = torch.full((d_off + n + band,), SENTINEL, dtype=dt, device=DEV)
        flat = buf[d_off:d_off + n]
        B, Cc, H, W = c.shape
        out = flat.view(B, H, W, Cc).permute(0, 3, 1, 2) if cl else flat.view(c.shape)
        assert out.data_ptr() == buf.data_ptr() + d_off * buf.element_size()
        res = image_batch(view, dtype=dt, channels_last=cl, src_layout=layout, reverse_channels=rev, out=out)
        assert res is out and same_bits(out, _torch(v, dt, layout, rev)), (cl, layout, rev, s_off, d_off)
        guard = torch.cat([buf[:d_off], buf[d_off + n:]])
        assert same_bits(guard, torch.full_like(guard, SENTINEL)), (cl, layout, rev, s_off, d_off)


# ---------------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(c, layout="nchw", rev=False):
    """(source as the call takes it, oracle result, terms): computed once per case and form, never changed"""
    key = (c.name, layout, rev)
    if key not in _ORACLE:
        v = _as(IC.resize_source(c), layout)
        _ORACLE[key] = (v,) + tuple(IO.image(v, c.out_hw, layout, rev))
    return _ORACLE[key]


def _check(got, want, terms, dt, what):
    r, zero, nonzero, bad = IO.within(got, want, terms, K, dt)
    print(f"{what}: ratio {r:.4f} of K = {K:.4f}, {zero} zero-terms elements of {got.numel()}")
    assert bad == 0 and nonzero == 0, what
    assert zero > 0, what                                  # the black quarter: the exact-zero set is not empty
    assert r <= K, what


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("c", IC.RESIZE, ids=[c.name for c in IC.RESIZE])
def test_resize_every_element_within_the_oracle_s_bars(c, dt):
    v, want, terms = _oracle(c)
    dv = v.to(DEV)
    for cl in (False, True):
        got = image_batch(dv, dtype=dt, channels_last=cl, size=c.out_hw)
        assert got.dtype == dt and tuple(got.shape) == (c.B, c.C) + c.out_hw
        assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
        _check(got, want, terms, dt, f"{c.name} {dt} channels_last={cl}")
        assert same_bits(image_batch(dv, dtype=dt, channels_last=cl, size=c.out_hw), got)
        if cl:
            assert same_bits(got.contiguous(), first)      # the two layouts hold the same values
        first = got


@pytest.mark.parametrize("name", ["down_odd", "ms96"])
def test_resize_from_an_interleaved_reversed_source(name):
    c = IC.RESIZE_BY_NAME[name]
    v, want, terms = _oracle(c, "nhwc", True)
    for cl, dt in itertools.product((False, True), (torch.float32, torch.float16)):
        got = image_batch(v.to(DEV), dtype=dt, channels_last=cl, size=c.out_hw, src_layout="nhwc", reverse_channels=True)
        _check(got, want, terms, dt, f"{name} nhwc reversed {dt} channels_last={cl}")
    plain = image_batch(IC.resize_source(c).flip(1).contiguous().to(DEV), size=c.out_hw)
    assert same_bits(image_batch(v.to(DEV), size=c.out_hw, src_layout="nhwc", reverse_channels=True), plain)   # the bytes' order changes no value


def test_size_equal_to_the_source_s_is_the_no_resize_result():
    c = IC.IDENTITY
    v = IC.resize_source(c).to(DEV)
    for dt, cl in itertools.product(DTYPES, (False, True)):
        got = image_batch(v, dtype=dt, channels_last=cl, size=c.out_hw)
        assert same_bits(got, image_batch(v, dtype=dt, channels_last=cl)) and same_bits(got, v.to(dt) / 255), (dt, cl)


def test_reference_multi_scale_cases_against_the_recorded_output():
    """the three sizes the reference draws: the device result and the reference's recorded host result are both inside the oracle's bars"""
    import numpy as np
    for seed, size in IC.MULTI_SCALE["seeds"].items():
        z = np.load(IC.path(f"ms{seed}"), allow_pickle=False)
        src = torch.from_numpy(z["src"])
        want, terms = IO.image(src, size)
        _check(image_batch(src.to(DEV), size=size), want, terms, torch.float32, f"seed {seed} device")
        _check(torch.from_numpy(z["ref_f32"]), want, terms, torch.float32, f"seed {seed} recorded")


# ---------------------------------------------------------------------------------------------------------------------------
# ImagePlan
# ---------------------------------------------------------------------------------------------------------------------------
PLANS = [
    ("resized", dict(B=2, C=3, H=40, W=56, size=(64, 64), dtype=torch.float32, channels_last=False, src_layout="nchw", reverse_channels=False)),
    ("channels_last", dict(B=2, C=3, H=70, W=130, size=None, dtype=torch.float16, channels_last=True, src_layout="nchw", reverse_channels=False)),
    ("predictor", dict(B=2, C=3, H=37, W=53, size=None, dtype=torch.float32, channels_last=False, src_layout="nhwc", reverse_channels=True)),
]


@pytest.mark.parametrize("name,kw", PLANS, ids=[p[0] for p in PLANS])
def test_plan_eager_and_captured_equal_image_batch(name, kw):
    kw = dict(kw)
    B, Cc, H, W = (kw.pop(k) for k in "BCHW")
    plan = ImagePlan.create(B, Cc, H, W, device=DEV, **kw)
    assert plan.launches() == 1 and plan.src.dtype == torch.uint8
    g = torch.Generator().manual_seed(11)
    fresh = lambda: torch.randint(0, 256, tuple(plan.src.shape), generator=g, dtype=torch.uint8).to(DEV)
    call = lambda v: image_batch(v, dtype=kw["dtype"], channels_last=kw["channels_last"], size=kw["size"], src_layout=kw["src_layout"],
                                 reverse_channels=kw["reverse_channels"])
    v = fresh()
    plan.src.copy_(v)
    out = plan.run()
    assert out is plan.out and same_bits(out, call(v))
    assert out.is_contiguous(memory_format=torch.channels_last if kw["channels_last"] else torch.contiguous_format)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.run()
    for _ in range(3):
        v = fresh()
        plan.src.copy_(v)
        plan.out.fill_(SENTINEL)
        graph.replay()
        assert same_bits(plan.out, call(v))
