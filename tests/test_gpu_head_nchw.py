"""GPU tests (-m gpu) of MGAMaskHead on NCHW features (csrc/head.cuh: k_head_gemm forward and gx, k_head_stats, k_head_out, k_head_bwd_act,
k_head_bwd_fin, k_head_bwd_gw / _gw2 / _gwf), the path the channels-last head, the slice and the static plans are measured against: the
rows of tests/head_nchw_rows.py at every tiling against the fp64 oracle ELEMENT BY ELEMENT, in units of what each element was summed
from (tests/test_abi_head_nchw.py checks on the CPU that the rows have the geometry their comments state and that the metric finds what
it is for), bit-identity across repeats, batch composition and call composition, the level flags through the C ABI, and work buffers
that are neither read before they are written nor written past their reported sizes."""
import pytest
import torch

from conftest import rel_err
from head_nchw_rows import CASE_IDS, CASES, HALF_FLOOR, HO, OUTPUTS, TOL, U_BAR, U_BAR_HALF, oracle32, row_case

pytestmark = pytest.mark.gpu
GRADS = ("gx", "gw1", "ggamma", "gbeta", "gwh", "gbh")


@pytest.fixture(scope="module")
def F(built_lib):
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


def _level(c, x=None):
    """A case's tensors on the device, fresh: the feature (leaf), the five parameters (leaves, module shapes) and the three buffers."""
    s = c.state
    x = (c.x if x is None else x).cuda().to(c.dtype).requires_grad_(True)
    ps = [s[k].cuda().clone().requires_grad_(True) for k in ("proj.0.weight", "proj.1.weight", "proj.1.bias", "head.weight", "head.bias")]
    bufs = [s[k].cuda().clone() for k in ("proj.1.running_mean", "proj.1.running_var", "proj.1.num_batches_tracked")]
    return x, ps, bufs


def _args(c, lv):
    x, ps, bufs = lv
    return (x, ps[0], ps[1], ps[2], bufs[0], bufs[1], bufs[2], ps[3], ps[4], c.p.eps, c.p.momentum, c.training)


def _collect(c, lv, y):
    x, ps, bufs = lv
    return dict(logits=y.detach(), gx=x.grad, gw1=ps[0].grad.reshape(c.hid, c.C), ggamma=ps[1].grad, gbeta=ps[2].grad, gwh=ps[3].grad,
                gbh=ps[4].grad, running_mean=bufs[0], running_var=bufs[1], nbt=bufs[2])


def _run(F, c, x=None, gl=None):
    """One case through mask_head, forward and backward -> every output, with the checks every run gets on dtypes, shapes and layout."""
    lv = _level(c, x)
    y = F.mask_head(*_args(c, lv)[:9], eps=c.p.eps, momentum=c.p.momentum, training=c.training)
    y.backward((c.gl if gl is None else gl).cuda().to(c.dtype))
    torch.cuda.synchronize()
    o = _collect(c, lv, y)
    B = lv[0].shape[0]
    assert o["logits"].dtype == c.dtype and o["logits"].shape == (B, 1, c.H, c.W)
    assert o["gx"].dtype == c.dtype and o["gx"].shape == lv[0].shape and o["gx"].is_contiguous(), f"{c.name}: gx came back in another layout"
    for k in GRADS[1:]:
        assert o[k].dtype == torch.float32, k
    assert o["gwh"].shape == (1, c.hid, 3, 3) and o["gbh"].shape == (1,) and o["ggamma"].shape == o["gbeta"].shape == (c.hid,)
    return o


def _same_bits(a, b, what):
    for k in OUTPUTS + ("nbt",):
        assert torch.equal(a[k], b[k]), (what, k)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. every row, every output, element by element
# ---------------------------------------------------------------------------------------------------------------------------
def _check(cid, c, o, keys=OUTPUTS):
    """fp32 rows against the fp64 oracle: rel_err < 1e-4 on every output (the project's tensor-scale bar) and u < U_BAR element-wise,
    u = |got - want| / (sum of the absolute values of the element's terms): 8 x what the fp32 oracle at one thread is off by against the
    fp64 one, + 4e-6 for what passes through sigmoid_fast (head_nchw_rows.U_BAR; DESIGN.md has the measured table).  fp16 / bf16 rows:
    rel_err < 4e-3 / 3e-2 against the fp32 oracle on the rounded inputs, and u < 2^-9 / 2^-6 against head_nchw_rows.oracle_fmt, the fp32
    oracle with the type's roundings where the kernels have them, with the smallest normal number of the type added to the magnitude
    (below it the format rounds absolutely)."""
    tol = TOL[c.dt]
    ewant, bars = (c.want, U_BAR) if c.dt == "f32" else (c.want_fmt, dict.fromkeys(OUTPUTS, U_BAR_HALF[c.dt]))
    report = []
    for k in keys:
        e = rel_err(o[k].float(), c.want[k].reshape(o[k].shape))
        u = HO.elem_u(o[k].float(), ewant[k], c.mag[k], HALF_FLOOR[c.dt])
        print(f"{cid} {k} rel_err {e:.3e} u {u:.3e} (bar {bars[k]:.1e})")
        if not e < tol:
            report.append(f"{k} rel_err {e:.3e}")
        if not u < bars[k]:
            report.append(f"{k} u {u:.3e} over {bars[k]:.1e}")
    assert not report, f"{cid}: " + "; ".join(report)


@pytest.mark.parametrize("name,dt,training,gkind", CASES, ids=CASE_IDS)
def test_head_nchw_row_vs_oracle(F, name, dt, training, gkind):
    """Every case under a dL/dlogits of uniform size, the eval-mode ones under the five-decade envelope as well (head_nchw_rows.CASES)."""
    c = row_case(name, dt, training, gkind)
    o = _run(F, c)
    nbt0 = int(c.state["proj.1.num_batches_tracked"])
    assert int(o["nbt"]) == nbt0 + (1 if training else 0)
    if not training:                                               # eval mode writes nothing back
        assert torch.equal(o["running_mean"].cpu(), c.state["proj.1.running_mean"])
        assert torch.equal(o["running_var"].cpu(), c.state["proj.1.running_var"])
    _check(f"{name}-{dt}-{'train' if training else 'eval'}-{gkind}", c, o)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. / 3. bits
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", [("ksplit_c132", "f32"), ("kw2_h64", "f32"), ("mw3_h80", "f32"), ("mtw4_h144", "f32"), ("mblk2_h384", "f32"),
                                     ("v1_guard", "f32"), ("gxk4_h130", "bf16"), ("gw2_ragged", "bf16")])
def test_two_runs_give_the_same_bits(F, name, dt):
    """Both dW1 forms (k_head_bwd_gw2: hidden 24, 64, 16; k_head_bwd_gw: the rest), both forward templates (MTW 2 / 4), K splits each way."""
    c = row_case(name, dt, True)
    _same_bits(_run(F, c), _run(F, c), name)


@pytest.mark.parametrize("name,dt", [("ksplit_c132", "f32"), ("gxk4_h130", "f32"), ("gxk4_h130", "f16"), ("gather_c6", "bf16")])
def test_eval_mode_is_per_sample(F, name, dt):
    """The tiling is per sample (b = wg / tps) and eval mode has no batch statistics: sample b alone gives the bits of row b of the batched
    call, logits and gx (under the same slice of dL/dlogits).  Any indexing that leaks across samples shows here."""
    c = row_case(name, dt, False)
    full = _run(F, c)
    for b in range(c.B):
        one = _run(F, c, c.x[b:b + 1], c.gl[b:b + 1])
        assert torch.equal(one["logits"], full["logits"][b:b + 1]), (name, b)
        assert torch.equal(one["gx"], full["gx"][b:b + 1]), (name, b)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. / 5. the level flags and the work buffers, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 256
NAN_BYTE, ZERO_BYTE = 0xFF, 0x00          # 0xFF..FF is a NaN in fp32, fp16 and bf16


class AbiLevel:
    """One NCHW level driven through mgahead_forward / mgahead_backward with buffers of its own: each is a byte tensor of its size (the
    size query's, or the tensor's) plus GUARD bytes, filled with one byte value."""

    def __init__(self, c, fill=ZERO_BYTE, fwd_flags=0):
        from mga_yolo_amd import _lib
        self.c, self.fill, self.lib, self._lib = c, fill, _lib.load(), _lib
        s = c.state
        self.x = c.x.cuda().to(c.dtype)
        self.pars = [s["proj.0.weight"].reshape(c.hid, c.C).cuda().contiguous()] + [s[k].cuda().clone() for k in
                                                                                    ("proj.1.weight", "proj.1.bias", "head.weight", "head.bias")]
        self.run = [s["proj.1.running_mean"].cuda().clone(), s["proj.1.running_var"].cuda().clone(), s["proj.1.num_batches_tracked"].cuda().clone()]
        self.fwd_flags = fwd_flags
        ldt = torch.float32 if fwd_flags & _lib.HEAD_LOGITS_F32 else c.dtype
        self.bufs = {}
        self.ctx = self._bytes("ctx", self.lib.mgahead_ctx_bytes(c.B, c.C, c.H, c.W, c.hid))
        self.scratch = self._bytes("scratch", self.lib.mgahead_bwd_scratch_bytes(c.B, c.C, c.H, c.W, c.hid))
        self.logits = self._tensor("logits", (c.B, 1, c.H, c.W), ldt)
        self.gx = self._tensor("gx", (c.B, c.C, c.H, c.W), c.dtype)
        self.pg = [self._tensor(f"pg{i}", t.shape, torch.float32) for i, t in enumerate(self.pars)]

    def _bytes(self, name, n):
        raw = torch.full((n + GUARD,), self.fill, dtype=torch.uint8, device="cuda")
        self.bufs[name] = (raw, n)
        return raw[:n]

    def _tensor(self, name, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        return self._bytes(name, n * torch.empty((), dtype=dtype).element_size()).view(dtype).view(shape)

    def refill(self, *names):
        for nm in names:
            raw, n = self.bufs[nm]
            raw[:n] = self.fill

    def forward(self):
        from mga_yolo_amd._binding import fill_head_fwd
        c = self.c
        fl = (self._lib.HeadFwdLevel * 1)()
        fill_head_fwd(fl[0], self.x, self.logits, self.ctx, self.pars, self.run, c.hid, c.p.eps, c.p.momentum, c.training, self.fwd_flags)
        self._lib.check(self.lib.mgahead_forward(fl, 1, torch.cuda.current_stream().cuda_stream), "mgahead_forward")

    def backward(self, gl, gl2=None, flags=0):
        from mga_yolo_amd._binding import fill_head_bwd
        c = self.c
        bl = (self._lib.HeadBwdLevel * 1)()
        fill_head_bwd(bl[0], self.x, gl, gl2, self.ctx, self.scratch, self.gx, self.pg, self.pars, self.run, c.hid, c.p.eps, c.p.momentum,
                      c.training, flags)
        self._lib.check(self.lib.mgahead_backward(bl, 1, torch.cuda.current_stream().cuda_stream), "mgahead_backward")
        torch.cuda.synchronize()

    def outputs(self):
        pg = self.pg
        return dict(logits=self.logits.clone(), gx=self.gx.clone(), gw1=pg[0].clone(), ggamma=pg[1].clone(), gbeta=pg[2].clone(), gwh=pg[3].clone(),
                    gbh=pg[4].clone(), running_mean=self.run[0].clone(), running_var=self.run[1].clone(), nbt=self.run[2].clone())

    def broken_guards(self):
        return [nm for nm, (raw, n) in self.bufs.items() if not bool((raw[n:] == self.fill).all())]


def _abi_step(c, fill=ZERO_BYTE, gl=None, gl2=None, bwd_flags=0, fwd_flags=0, gx0=None):
    L = AbiLevel(c, fill, fwd_flags)
    L.forward()
    L.refill("scratch")
    if gx0 is not None:
        L.gx.copy_(gx0)
    else:
        L.refill("gx")
    L.backward(c.gl.cuda().to(c.dtype) if gl is None else gl, gl2, bwd_flags)
    return L


FLAG_CASES = [("ksplit_c132", "f32"), ("ksplit_c132", "f16"), ("v1_guard", "f32"), ("v1_guard", "bf16"), ("gxk4_h130", "f32"), ("gxk4_h130", "f16")]


@pytest.mark.parametrize("name,dt", FLAG_CASES)
def test_accum_gx_on_an_nchw_level(F, name, dt):
    """MGAHEAD_BWD_ACCUM_GX: gx pre-filled with G0 comes back as G0 + the plain result -- the bits of that sum in fp32, within the half
    tolerance of G0 + the fp32 oracle's gx in half precision.  Every other output is the plain run's."""
    from mga_yolo_amd import _lib
    c = row_case(name, dt, True)
    g0 = torch.randn(c.B, c.C, c.H, c.W, generator=torch.Generator().manual_seed(77)).to(c.dtype).cuda()
    plain = _abi_step(c, NAN_BYTE).outputs()
    acc = _abi_step(c, NAN_BYTE, bwd_flags=_lib.HEAD_BWD_ACCUM_GX, gx0=g0).outputs()
    assert not torch.isnan(plain["gx"].float()).any()
    if dt == "f32":
        assert torch.equal(acc["gx"], g0 + plain["gx"])
    else:
        e = rel_err(acc["gx"].float(), g0.float().cpu() + c.want["gx"])
        print(f"{name}-{dt} accum gx rel_err {e:.3e}")
        assert e < TOL[dt]
    for k in OUTPUTS:
        if k != "gx":
            assert torch.equal(acc[k], plain[k]), k


@pytest.mark.parametrize("name,dt", FLAG_CASES)
def test_g_logits2_on_an_nchw_level(F, name, dt):
    """(g_logits, g_logits2) equals the pre-summed gradient: the same fp32 add, so every output has the same bits when g_logits is fp32;
    half g_logits with an fp32 g_logits2 meet the half bars of the oracle fed g_logits.float() + g_logits2."""
    c = row_case(name, dt, True)
    gl = c.gl.cuda().to(c.dtype)
    gl2 = (0.5 * torch.randn(c.B, 1, c.H, c.W, generator=torch.Generator().manual_seed(78))).cuda()
    two = _abi_step(c, gl=gl, gl2=gl2).outputs()
    if dt == "f32":
        _same_bits(two, _abi_step(c, gl=gl + gl2).outputs(), name)
        return
    want = oracle32(c.x, (gl.float() + gl2).cpu(), c.p, True)
    for k in GRADS:
        e = rel_err(two[k].float(), want[k].reshape(two[k].shape))
        print(f"{name}-{dt} g_logits2 {k} rel_err {e:.3e}")
        assert e < TOL[dt], k


@pytest.mark.parametrize("name,dt", [("ksplit_c132", "f16"), ("v1_guard", "bf16"), ("gxk4_h130", "f16"), ("gxk4_h130", "bf16")])
def test_logits_f32_with_half_features(F, name, dt):
    """MGAHEAD_LOGITS_F32: the forward's fp32 logits, rounded to the feature type, are the bits of the half-logits run; the backward fed
    fp32 g_logits meets the half bars."""
    from mga_yolo_amd import _lib
    c = row_case(name, dt, True)
    half = _abi_step(c).outputs()
    L = _abi_step(c, fwd_flags=_lib.HEAD_LOGITS_F32, gl=c.gl.cuda(), bwd_flags=_lib.HEAD_LOGITS_F32)
    o = L.outputs()
    assert o["logits"].dtype == torch.float32 and torch.equal(o["logits"].to(c.dtype), half["logits"])
    assert not L.broken_guards()
    _check(f"{name}-{dt}-logits_f32", c, o, keys=GRADS)


@pytest.mark.parametrize("name,dt,training", [("v1_guard", "f32", True), ("ksplit_c132", "f32", True), ("gxk4_h130", "f32", True),
                                              ("gxk4_h130", "bf16", True), ("w500", "f32", True), ("v1_guard", "f32", False),
                                              ("ksplit_c132", "f32", False), ("gxk4_h130", "bf16", False)])
def test_work_buffers_are_written_before_read_and_not_overrun(F, name, dt, training):
    """ctx, scratch, logits, gx and every parameter gradient allocated with 256 bytes beyond the size the library reports (or the
    tensor's), everything NaN before the forward, scratch and gx NaN again before the backward: the results are the bits of a run on
    zero-filled buffers, hold no NaN, and the 256 bytes behind every buffer still hold the fill.  (functional.py hands the library
    torch.empty buffers: whatever they held must not matter.)  Every access stays inside the allocations unless a kernel is wrong."""
    c = row_case(name, dt, training)
    nan, zero = _abi_step(c, NAN_BYTE), _abi_step(c, ZERO_BYTE)
    a, b = nan.outputs(), zero.outputs()
    for k in OUTPUTS:
        assert not torch.isnan(a[k].float()).any(), k
    _same_bits(a, b, name)
    assert not nan.broken_guards() and not zero.broken_guards(), (nan.broken_guards(), zero.broken_guards())
    _check(f"{name}-{dt}-abi", c, a)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. mixed pyramid calls
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [
    # hidden 24, 64, 144, 384: both forward launches (MTW 2 / 4), both dW1 launches, k_head_bwd_act's LDS run length differing by level
    [("ksplit_c132", "f32"), ("kw2_h64", "f32"), ("mtw4_h144", "f32"), ("mblk2_h384", "f32")],
    # a vec 1 and a vec 4 level, an fp32 and a bf16 level: different launch groups
    [("v1_guard", "f32"), ("out2_h40", "f32"), ("gw2_ragged", "bf16"), ("v1_w333", "bf16")]], ids=["four_hidden_widths", "mixed_vec_and_dtype"])
def test_mixed_pyramid_call_equals_the_levels_called_alone(F, levels):
    """Every output of every level of one mask_head_pyramid call each way has the bits of the level called alone from the same running
    statistics (every run starts from fresh copies of the row's state)."""
    cases = [row_case(n, dt, True) for n, dt in levels]
    lvs = [_level(c) for c in cases]
    ys = F.mask_head_pyramid([_args(c, lv) for c, lv in zip(cases, lvs)])
    torch.autograd.backward(ys, [c.gl.cuda().to(c.dtype) for c in cases])
    torch.cuda.synchronize()
    for c, lv, y in zip(cases, lvs, ys):
        _same_bits(_collect(c, lv, y), _run(F, c), c.name)
