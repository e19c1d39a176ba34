"""Loss-side rows on the device (-m gpu): the multi-scale segmentation loss (k_seg_partial / k_seg_final / k_seg_bwd), the Kendall combine
riding in its launches, the ProbMaskGater launch and the nearest resize, at the sizes where their loops take a second trip and at the
edges of their clamps and gates.  Every comparison is with the fp64 oracle (oracle/segloss_oracle.py), torch on the CPU or host math in
fp64; the only library-against-library rows are the ones that say so (bit-for-bit reproducibility, fused == two calls).
tests/test_loss_rows_tables.py proves on the CPU which branch every row below reaches and the conditions on the inputs.
NaN inputs are out of scope: the device's fmaxf returns the other operand where torch.clamp propagates the NaN, by design."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import elem_err
from oracle import loss_rows as R
from oracle import segloss_oracle as O
from test_loss_rows_tables import LADDER_KW, ladder_case

pytestmark = pytest.mark.gpu

HALF_TOL = {torch.float16: 2e-3, torch.bfloat16: 2e-2}        # the bars of test_segloss.test_device_half_precision_logits


@pytest.fixture(scope="module")
def seg(built_lib):
    from mga_yolo_amd import _lib
    from mga_yolo_amd.segloss import SegLossConfig, SegmentationLoss
    _lib.load()
    return SegLossConfig, SegmentationLoss


def _prob_mode(monkeypatch, bilinear):
    if bilinear:
        monkeypatch.setenv("MGA_PROB_MODE", "1")
    else:
        monkeypatch.delenv("MGA_PROB_MODE", raising=False)


def _device_run(seg, preds, tg, kw, gout=1.0):
    SegLossConfig, SegmentationLoss = seg
    pd = {k: v.cuda().requires_grad_(True) for k, v in preds.items()}
    td, ld = SegmentationLoss(SegLossConfig(**kw))(pd, [t.cuda() for t in tg])
    (td * gout).backward()
    return td.detach().cpu(), ld, {k: v.grad.cpu() for k, v in pd.items()}


def _oracle64(preds, tg, kw, bilinear=False, gout=1.0):
    po = {k: v.double().requires_grad_(True) for k, v in preds.items()}
    to, lo = O.forward(po, [t.double() for t in tg], O.SegLossConfig(**kw), bilinear_targets=bilinear)
    (to * gout).backward()
    return to.detach(), lo, {k: v.grad for k, v in po.items()}


def _check_values(td, ld, to, lo):
    assert ld.keys() == lo.keys()
    for k in lo:
        assert abs(ld[k] - lo[k]) <= 1e-5 * max(1.0, abs(lo[k])), (k, ld[k], lo[k])
    assert abs(float(td) - float(to)) <= 1e-5 * max(1.0, abs(float(to)))


def _check_grads_fp32(gd, go, tag, d_rows=None):
    """Tensor-scale 1e-4 (the bar of test_segloss) and element-wise 1e-3 (conftest.elem_err, floor 1e-3 of the maximum).
    d_rows: levels whose target is resampled bilinearly.  There the device holds the target in fp32, up to 4 d_row from the fp64 one
    (test_every_element_of_the_resampled_target asserts exactly that), dg_i/dt_i is about max|g| / max|p - t| ~ max|g|, and an element
    at the floor is measured against 1e-3 max|g|: the target's own fp32 rounding costs up to 4 d_row / 1e-3 there, twice that with the
    Dice / Tversky term's share.  It is 6e-4 at power-of-two ratios (d_row 7e-8) and dominates at odd ratios, where the element map of
    the target itself (part 2) is the sharp check."""
    for k in go:
        w = go[k]
        e_t = float((gd[k].double() - w).abs().max()) / (float(w.abs().max()) + 1e-300)
        e_e = elem_err(gd[k], w)
        bar = 1e-3 + (8 * d_rows[k] / 1e-3 if d_rows else 0.0)
        print(f"{tag} {k}: tensor-scale {e_t:.2e} element-wise {e_e:.2e} (bar {bar:.2e})")
        assert float((gd[k].double() - w).abs().max()) <= 1e-4 * float(w.abs().max()) + 1e-9, (tag, k)
        assert e_e <= bar, (tag, k, e_e)


# ---- 2. every element of the target the kernel saw ------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.TARGET_TABLE, ids=lambda r: r[0])
def test_every_element_of_the_resampled_target(seg, monkeypatch, row):
    """dice_weight = 0, bce_weight = 1, plain mode: k_seg_bwd writes (p_i - t_i) / (B H W), which gives back t_i, the value seg_target
    gathered for that pixel.  nearest: copies, 1e-6.  bilinear: 1e-6 + 4 d_row, d_row = max |F.interpolate fp32 - fp64 resampler| of the
    row, from torch alone.  A wrong tap, a wrong clamp at the last row / column or a transposed index is an error of 0.1 to 1."""
    name, B, size, tsize = row
    HW = size[0] * size[1]
    x = R.logits_for(B, size, R.row_seed(name), scale=1.0)              # |x| < 5: sigmoid(x) keeps its bits for the subtraction
    for bilinear in (False, True):
        _prob_mode(monkeypatch, bilinear)
        for soft in (False, True):
            for dim3 in (False, True):
                t = R.targets_for(B, tsize, soft, R.row_seed(name, soft), dim3=dim3)
                _, _, g = _device_run(seg, {"p3": x}, [t], dict(dice_weight=0.0, bce_weight=1.0))
                got = R.recover_target(x, g["p3"], B, HW)
                want = O.resample64(t if t.dim() == 4 else t.unsqueeze(1), *size, bilinear)
                err = float((got - want).abs().max())
                d = R.d_row(t, size) if bilinear else 0.0
                bar = 1e-6 + 4 * d
                print(f"target {name} {'bilinear' if bilinear else 'nearest'} {'soft' if soft else 'binary'} {'3-D' if dim3 else '4-D'}: "
                      f"d_row {d:.2e} device error {err:.2e} bar {bar:.2e}")
                if err > bar:
                    bad = ((got - want).abs() > bar).nonzero()
                    print("  first offenders (b, 0, y, x):", bad[:8].tolist(), "of", len(bad))
                assert err <= bar, (name, bilinear, soft, dim3, err, bar)


# ---- 3. the loops ---------------------------------------------------------------------------------------------------------
def _ladder_check(seg, preds, tg, ufl, tag):
    kw = dict(LADDER_KW, use_unified_focal=ufl)
    to, lo, go = _oracle64(preds, tg, kw, gout=1.7)
    td, ld, gd = _device_run(seg, preds, tg, kw, gout=1.7)
    _check_values(td, ld, to, lo)
    _check_grads_fp32(gd, go, tag)
    td2, ld2, gd2 = _device_run(seg, preds, tg, kw, gout=1.7)                   # library against itself: the fixed summation order
    assert torch.equal(td, td2) and ld == ld2 and all(torch.equal(gd[k], gd2[k]) for k in gd), "two runs differ in their bits"
    # half-precision logits get their gradient in that type.  Unscaled it is about 1 / (B H W): 5e-6 at 160 x 160, below fp16's smallest
    # normal number (6.1e-5), where the format steps by 6e-8 and cannot hold 2e-3 of such a value.  The rows carry a loss scale of 1024,
    # as the reference trainer's GradScaler does for exactly this reason: a condition on the input, the bars stay
    for dt, tol in HALF_TOL.items():
        ph = {k: v.to(dt) for k, v in preds.items()}
        to, lo, go = _oracle64({k: v.float() for k, v in ph.items()}, tg, kw, gout=1024.0)
        td, ld, gd = _device_run(seg, ph, tg, kw, gout=1024.0)
        _check_values(td, ld, to, lo)
        assert abs(float(td) - float(to)) < 1e-5 * abs(float(to)) + 1e-6
        for k in go:
            assert gd[k].dtype == dt
            assert float((gd[k].double() - go[k]).abs().max()) <= tol * float(go[k].abs().max()), (tag, dt, k)


@pytest.mark.parametrize("ufl", [False, True], ids=["plain", "ufl"])
@pytest.mark.parametrize("n,shape", R.ladder_rows(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_size_ladder(seg, monkeypatch, n, shape, ufl):
    _prob_mode(monkeypatch, False)
    preds, tg = ladder_case(n, shape)
    _ladder_check(seg, preds, tg, ufl, f"ladder {n} as {shape} {'ufl' if ufl else 'plain'}")


@pytest.mark.parametrize("ufl", [False, True], ids=["plain", "ufl"])
@pytest.mark.parametrize("B", R.BATCH_LADDER)
def test_batch_ladder(seg, monkeypatch, B, ufl):
    _prob_mode(monkeypatch, False)
    preds, tg = ladder_case(35, (5, 7), B=B)
    _ladder_check(seg, preds, tg, ufl, f"batch {B} {'ufl' if ufl else 'plain'}")


# ---- through the C ABI ----------------------------------------------------------------------------------------------------
def _levels(_lib, logits, targets, resize, weights, glogits=None, n_alloc=None):
    n = len(logits)
    levels = (_lib.SegLevel * (n_alloc or n))()
    code = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
    for l in range(n):
        S = levels[l]
        S.logits, S.target = logits[l].data_ptr(), targets[l].data_ptr()
        S.glogits = glogits[l].data_ptr() if glogits else None
        S.B, _, S.H, S.W = logits[l].shape
        S.Ht, S.Wt = targets[l].shape[-2:]
        S.dtype, S.scale_weight, S.resize = code[logits[l].dtype], weights[l], resize[l]
    return levels


def _per_level_oracle(logits, targets, resize, weights, cfgkw, lam):
    """More levels / mixed resize rules than the module's interface can express: the oracle level by level, in fp64."""
    out, grads, total = [], [], torch.zeros((), dtype=torch.float64)
    leaves = [x.double().requires_grad_(True) for x in logits]
    for x, t, r, w in zip(leaves, targets, resize, weights):
        tl, lg = O.forward({"p3": x}, [t.double()], O.SegLossConfig(scale_weights=(w,), loss_lambda=1.0, **cfgkw), bilinear_targets=bool(r))
        out += [lg["p3_bce"], lg["p3_dice"], lg["p3_combined"]]
        total = total + tl
    total = total * lam
    return total, out, leaves


def test_four_levels_with_mixed_resize_rules(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(41)
    B = 3
    spec = [((25, 20), (48, 41), _lib.SEG_NEAREST), ((12, 10), (12, 10), _lib.SEG_BILINEAR),       # resampled / identity (rule unused)
            ((96, 90), (48, 45), _lib.SEG_BILINEAR), ((6, 5), (48, 40), _lib.SEG_BILINEAR)]         # level 2: second outer trip, up-sampling
    # (the bilinear levels keep power-of-two ratios: their source coordinates are exact in fp32, see _check_grads_fp32)
    logits = [torch.randn(B, 1, *s, generator=g) * 2 for s, _, _ in spec]
    targets = [torch.rand(B, 1, *t, generator=g) for _, t, _ in spec]
    resize, weights = [r for _, _, r in spec], (1.0, 0.5, 0.25, 2.0)
    st = torch.cuda.current_stream().cuda_stream
    for ufl in (0, 1):
        cfgkw = dict(bce_weight=0.9, dice_weight=1.1, smooth=1.0, use_unified_focal=bool(ufl), ufl_lambda=0.4, ufl_delta=0.6, ufl_gamma=0.5)
        if ufl:          # keep every resampled pixel clear of the t > 0.5 decision (see test_loss_rows_tables, part 4): binary sources, nearest only
            tg = [(t > 0.7).float() for t in targets]
            rs = [_lib.SEG_NEAREST] * 4
        else:
            tg, rs = targets, resize
        total, want, leaves = _per_level_oracle(logits, tg, rs, weights, cfgkw, 0.7)
        (total * 1.3).backward()
        ld, td = [x.cuda() for x in logits], [t.cuda() for t in tg]
        gl = [torch.zeros_like(x) for x in ld]
        levels = _levels(_lib, ld, td, rs, weights, gl)
        cfg = _lib.SegCfg(0.9, 1.1, 1.0, 0.7, ufl, 0.4, 0.6, 0.5)
        ws = torch.zeros(lib.mgaseg_ws_bytes(levels, 4), dtype=torch.uint8, device="cuda")
        out = torch.zeros(13, device="cuda")
        gout = torch.tensor([1.3], device="cuda")
        _lib.check(lib.mgaseg_forward(levels, 4, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), st), "fwd")
        _lib.check(lib.mgaseg_backward(levels, 4, C.byref(cfg), ws.data_ptr(), ws.numel(), gout.data_ptr(), st), "bwd")
        torch.cuda.synchronize()
        got = out.cpu().tolist()
        assert abs(got[0] - float(total)) <= 1e-5 * max(1.0, abs(float(total)))
        for i, v in enumerate(want):
            assert abs(got[1 + i] - v) <= 1e-5 * max(1.0, abs(v)), (ufl, i, got[1 + i], v)
        d_rows = {i: (R.d_row(tg[i], spec[i][0]) if rs[i] == _lib.SEG_BILINEAR else 0.0) for i in range(4)}
        _check_grads_fp32({i: t.cpu() for i, t in enumerate(gl)}, {i: x.grad for i, x in enumerate(leaves)}, f"four levels ufl={ufl}", d_rows)


def test_five_levels_and_an_unknown_resize_rule_are_errors_with_nothing_launched(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    logits = [torch.zeros(1, 1, 4, 4, device="cuda") for _ in range(5)]
    targets = [torch.zeros(1, 1, 8, 8, device="cuda") for _ in range(5)]
    gl = [torch.full_like(x, 7.0) for x in logits]
    st = torch.cuda.current_stream().cuda_stream
    cfg = _lib.SegCfg(1.0, 1.0, 1.0, 1.0, 0, 0.5, 0.6, 0.5)
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((16,), 7.0, device="cuda")
    gout = torch.ones(1, device="cuda")
    five = _levels(_lib, logits, targets, [0] * 5, [1.0] * 5, gl)
    assert lib.mgaseg_ws_bytes(five, 5) == 0
    assert lib.mgaseg_forward(five, 5, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), st) == _lib.E_LEVELS
    assert lib.mgaseg_backward(five, 5, C.byref(cfg), ws.data_ptr(), ws.numel(), gout.data_ptr(), st) == _lib.E_LEVELS
    bad = _levels(_lib, logits[:2], targets[:2], [_lib.SEG_BILINEAR, 2], [1.0, 1.0], gl[:2])
    assert lib.mgaseg_forward(bad, 2, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), st) == _lib.E_SHAPE
    assert lib.mgaseg_backward(bad, 2, C.byref(cfg), ws.data_ptr(), ws.numel(), gout.data_ptr(), st) == _lib.E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all()) and all(bool((g_ == 7.0).all()) for g_ in gl)


@pytest.mark.parametrize("variant", ["fp16_logits", "bilinear_targets", "unified_focal"])
@pytest.mark.parametrize("n_det", R.KENDALL_N)
def test_fused_kendall_at_every_trip_count(built_lib, variant, n_det):
    """mgaseg_kendall_* against mgaseg_* + mgakendall_* bit for bit (library against itself, on purpose) AND against the closed-form
    combine in fp64 on the fp64 oracle's loss: total_i = e^-s0 det_i + s0 + e^-s1 seg + s1 and its four gradients."""
    from mga_yolo_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(100 + n_det)
    B, sizes, tsize = 5, [(24, 20), (12, 10), (6, 5)], (48, 40)
    dt = torch.float16 if variant == "fp16_logits" else torch.float32
    bil, ufl = variant == "bilinear_targets", int(variant == "unified_focal")
    logits = [(torch.randn(B, 1, h, w, generator=g) * 2).to(dt) for h, w in sizes]
    targets = [torch.rand(B, 1, *tsize, generator=g) if bil else (torch.rand(B, 1, *tsize, generator=g) > 0.7).float() for _ in sizes]
    det = torch.rand(n_det, generator=g) * 3 + 0.1
    lv = torch.tensor([0.3, -0.2])
    g_total = torch.randn(n_det, generator=g)
    weights, lam = (1.0, 0.5, 0.25), 0.7
    resize = [_lib.SEG_BILINEAR if bil else _lib.SEG_NEAREST] * 3
    ld, td = [x.cuda() for x in logits], [t.cuda() for t in targets]
    det_d, lv_d, gt_d = det.cuda(), lv.cuda(), g_total.cuda()
    st = torch.cuda.current_stream().cuda_stream

    def run(fused):
        gl = [torch.zeros_like(x) for x in ld]
        levels = _levels(_lib, ld, td, resize, weights, gl)
        cfg = _lib.SegCfg(1.0, 1.0, 1.0, lam, ufl, 0.5, 0.6, 0.5)
        ws = torch.zeros(lib.mgaseg_ws_bytes(levels, 3), dtype=torch.uint8, device="cuda")
        out = torch.zeros(10, device="cuda"); total = torch.zeros(n_det, device="cuda")
        g_det = torch.zeros(n_det, device="cuda"); g_seg = torch.zeros((), device="cuda"); g_lv = torch.zeros(2, device="cuda")
        if fused:
            _lib.check(lib.mgaseg_kendall_forward(levels, 3, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), det_d.data_ptr(), n_det,
                                                  lv_d.data_ptr(), total.data_ptr(), st), "fwd")
            _lib.check(lib.mgaseg_kendall_backward(levels, 3, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), det_d.data_ptr(), n_det,
                                                   lv_d.data_ptr(), gt_d.data_ptr(), g_det.data_ptr(), g_seg.data_ptr(), g_lv.data_ptr(), st), "bwd")
        else:
            _lib.check(lib.mgaseg_forward(levels, 3, C.byref(cfg), ws.data_ptr(), ws.numel(), out.data_ptr(), st), "fwd")
            _lib.check(lib.mgakendall_forward(det_d.data_ptr(), n_det, out.data_ptr(), lv_d.data_ptr(), total.data_ptr(), st), "kfwd")
            _lib.check(lib.mgakendall_backward(det_d.data_ptr(), n_det, out.data_ptr(), lv_d.data_ptr(), gt_d.data_ptr(), g_det.data_ptr(),
                                               g_seg.data_ptr(), g_lv.data_ptr(), st), "kbwd")
            _lib.check(lib.mgaseg_backward(levels, 3, C.byref(cfg), ws.data_ptr(), ws.numel(), g_seg.data_ptr(), st), "bwd")
        torch.cuda.synchronize()
        return [out, total, g_det, g_seg.reshape(1), g_lv] + gl

    fused, two = run(True), run(False)
    for i, (a, b) in enumerate(zip(fused, two)):
        assert torch.equal(a, b), f"fused and two-call results differ in tensor {i}"
    # closed form in fp64
    cfgkw = dict(bce_weight=1.0, dice_weight=1.0, smooth=1.0, use_unified_focal=bool(ufl), ufl_lambda=0.5, ufl_delta=0.6, ufl_gamma=0.5)
    seg64, _, leaves = _per_level_oracle([x.float() for x in logits], targets, [int(bil)] * 3, weights, cfgkw, lam)
    s0, s1 = float(lv[0]), float(lv[1])
    e0, e1 = math.exp(-s0), math.exp(-s1)
    gsum = float(g_total.double().sum())
    (seg64 * (gsum * e1)).backward()
    out, total, g_det, g_seg, g_lv = (t.cpu().double() for t in fused[:5])
    sv = float(seg64.detach())
    assert abs(float(out[0]) - sv) <= 1e-5 * max(1.0, abs(sv))
    want_total = e0 * det.double() + s0 + e1 * sv + s1
    assert bool(((total - want_total).abs() <= 1e-5 * want_total.abs().clamp_min(1.0)).all())
    assert torch.allclose(g_det, g_total.double() * e0, rtol=1e-6, atol=0)
    want_seg = gsum * e1
    want0 = float((g_total.double() * (1 - e0 * det.double())).sum())
    want1 = gsum * (1 - e1 * sv)
    assert abs(float(g_seg) - want_seg) <= 1e-4 * max(1.0, abs(want_seg))
    assert abs(float(g_lv[0]) - want0) <= 1e-4 * max(1.0, abs(want0)) and abs(float(g_lv[1]) - want1) <= 1e-4 * max(1.0, abs(want1))
    tol = 2e-3 if dt == torch.float16 else 1e-4
    for x, gd in zip(leaves, fused[5:]):
        w = x.grad
        assert float((gd.cpu().double() - w).abs().max()) <= tol * float(w.abs().max()) + 1e-9
        if dt == torch.float32:
            d = R.d_row(targets[0], tuple(w.shape[-2:])) if bil else 0.0
            assert elem_err(gd, w) <= 1e-3 + 8 * d / 1e-3


# ---- 4. clamp and gate edges ----------------------------------------------------------------------------------------------
def _corner_data():
    g = torch.Generator().manual_seed(23)
    B, sizes = 3, ((12, 10), (6, 5))
    preds = {k: torch.randn(B, 1, *s, generator=g) * 2 for k, s in zip(("p3", "p4"), sizes)}
    tg = [(torch.rand(B, 1, *s, generator=g) > 0.6).float() for s in sizes]
    return preds, tg


def _zero_target(preds, tg):
    for t in tg:
        t[0] = 0.0


def _one_target(preds, tg):
    for t in tg:
        t[0] = 1.0


def _saturated(preds, tg):
    # sigmoid(13.8) = 1 - 1.017e-6 and sigmoid(13.9) = 1 - 9.2e-7 straddle the pt / base clamps at 1e-6.  In fp32 1 - p is a multiple of
    # 2^-24: 1.07e-6 at 13.8, 9.5e-7 at 13.9 -- both on the same side of 1e-6 as the fp64 values, by 5 % or more of the bound (an fp32
    # sigmoid cannot be placed closer: its own grid is 6 % of the bound there).  Each value meets both target values along its row.
    for i, v in enumerate((13.8, -13.8, 13.9, -13.9, 30.0, -30.0)):
        preds["p3"][1, 0, i, :] = v
        tg[0][1, 0, i, ::2] = 1.0
        tg[0][1, 0, i, 1::2] = 0.0


def _perfect_sample(preds, tg):
    # sample 2 predicted perfectly and confidently: 1 - mti is 1e-13 in fp64 and at most 6e-8 in fp32, both far below eps = 1e-6
    for k, t in zip(("p3", "p4"), tg):
        preds[k][2] = (t[2] * 2 - 1) * 30.0


UFL = dict(use_unified_focal=True, ufl_lambda=0.4, ufl_delta=0.6, ufl_gamma=0.5)
CORNERS = {
    "ufl_smooth0_zero_target": (dict(UFL, smooth=0.0), _zero_target),                          # Du = (1 - delta) P, mti = 0
    "dice_smooth0_zero_target": (dict(smooth=0.0), _zero_target),                              # plain Dice denominator P + T = P
    "ufl_smooth0_delta1_zero_target": (dict(UFL, smooth=0.0, ufl_delta=1.0), _zero_target),    # Du_raw = 0 < eps: clamped, no gradient through it
    "ufl_all_one_target": (dict(UFL), _one_target),
    "dice_all_one_target": (dict(), _one_target),
    "ufl_saturated_logits": (dict(UFL), _saturated),
    "ufl_gamma_0.999": (dict(UFL, ufl_gamma=0.999), _saturated),
    "ufl_gamma_0.05": (dict(UFL, ufl_gamma=0.05), _saturated),
    "ufl_perfect_sample": (dict(UFL), _perfect_sample),
    "ufl_perfect_sample_smooth0": (dict(UFL, smooth=0.0), _perfect_sample),
}


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_clamp_corners(seg, monkeypatch, name):
    _prob_mode(monkeypatch, False)
    kw, edit = CORNERS[name]
    kw = dict(kw, scale_weights=(1.0, 2.0, 0.5), loss_lambda=1.3)
    preds, tg = _corner_data()
    edit(preds, tg)
    to, lo, go = _oracle64(preds, tg, kw)
    td, ld, gd = _device_run(seg, preds, tg, kw)
    _check_values(td, ld, to, lo)
    _check_grads_fp32(gd, go, f"corner {name}")


@pytest.mark.parametrize("name", [r[0] for r in R.UFL_BILINEAR])
def test_unified_focal_with_bilinear_soft_targets(seg, monkeypatch, name):
    """t > 0.5 is decided per pixel on the resampled target; the inputs keep every pixel 10 (1e-6 + 4 d_row) away from 0.5 (asserted on
    the CPU in test_loss_rows_tables), so fp32 and fp64 decide alike and every pixel is compared."""
    _prob_mode(monkeypatch, True)
    B, size, tsize, x, t = R.ufl_bilinear_inputs(name)
    kw = dict(UFL, scale_weights=(1.0,), loss_lambda=1.3)
    to, lo, go = _oracle64({"p3": x}, [t], kw, bilinear=True)
    td, ld, gd = _device_run(seg, {"p3": x}, [t], kw)
    _check_values(td, ld, to, lo)
    _check_grads_fp32(gd, go, name, {"p3": R.d_row(t, size)})


def test_unified_focal_bilinear_pixels_exactly_one_half(seg, monkeypatch):
    """Binary targets, 160 <- 1280: thousands of resampled pixels are exactly 0.5 in fp32 and fp64 alike: `t > 0.5`, not `>=`."""
    _prob_mode(monkeypatch, True)
    t = R.targets_for(1, (1280, 1280), False, R.row_seed("half_exact"))
    x = R.logits_for(1, (160, 160), R.row_seed("half_exact"))
    kw = dict(UFL, scale_weights=(1.0,), loss_lambda=1.3)
    to, lo, go = _oracle64({"p3": x}, [t], kw, bilinear=True)
    td, ld, gd = _device_run(seg, {"p3": x}, [t], kw)
    _check_values(td, ld, to, lo)
    _check_grads_fp32(gd, go, "half_exact")              # d_row is 0 here: the weights are 1/2 exactly


# ---- ProbMaskGater ----------------------------------------------------------------------------------------------------------
def _gater_device(p, u1, u2, tau, p_min, hard, gout):
    from mga_yolo_amd import prob_mask_gate
    x = p.cuda().requires_grad_(True)
    out = prob_mask_gate(x, u1.cuda(), u2.cuda(), tau, p_min, 0.5, hard)
    out.backward(gout.cuda())
    return out.detach().cpu(), x.grad.cpu()


def _gater_values(out, ref, hard, tag):
    if hard:
        near = (ref["soft"] - 0.5).abs() < 1e-6                     # the fuzzer's rule: decisions within rounding of the threshold may flip
        flips = out.double() != ref["out"]
        print(f"{tag}: {int(flips.sum())} hard decisions differ, {int(near.sum())} elements within 1e-6 of the threshold")
        assert not bool((flips & ~near).any())
    else:
        d = (out.double() - ref["soft"]).abs()
        r = d / (1e-7 + 2e-6 * ref["soft"].abs())
        print(f"{tag}: value max abs {float(d.max()):.2e}, worst error / bar {float(r.max()):.2f}")
        assert torch.allclose(out.double(), ref["soft"], rtol=2e-6, atol=1e-7), (tag, float(d.max()), float(r.max()))


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("tau", [0.3, 2.5])
@pytest.mark.parametrize("p_min", [0.0, 0.15])
def test_gater_edge_grid(built_lib, p_min, tau, hard):
    p, u1, u2 = R.gater_edge_grid(p_min)
    g = torch.Generator().manual_seed(7)
    gout = (torch.rand(p.shape, generator=g) + 0.5) * torch.where(torch.rand(p.shape, generator=g) > 0.5, 1.0, -1.0)
    ref = R.gater_host64(p, u1, u2, tau, p_min, 0.5, hard, gout)
    out, gp = _gater_device(p, u1, u2, tau, p_min, hard, gout)
    tag = f"gater edges p_min={p_min} tau={tau} {'hard' if hard else 'soft'}"
    _gater_values(out, ref, hard, tag)
    rows = p.shape[2]
    worst = max(elem_err(gp[0, 0, r], ref["grad"][0, 0, r]) for r in range(rows) if bool(ref["gate_open"][0, 0, r].any()))
    print(f"{tag}: gradient element-wise (per p row) {worst:.2e}")
    assert worst <= 1e-3
    # which elements get a zero gradient.  A closed gate (clamp(0,1), p_min, the logit's own clamp) is an exact zero on both sides.  An
    # open gate gives g m (1 - m) dlogit / tau, and 1 - m rounds to 0 in fp32 once it falls below 2^-25 (3e-8): there the device's
    # zero is rounding, not a gate, and the fp64 value is not zero.  So: closed => zero; open and m (1 - m) >= 2.4e-7 in fp64 (four
    # fp32 steps from 1) => not zero; in between either, and elem_err above still binds those elements.
    zero = gp == 0
    closed = ~ref["gate_open"]
    assert bool(zero[closed].all()), "a closed gate let a gradient through"
    m = ref["soft"]
    alive = ref["gate_open"] & (m * (1 - m) >= 2.4e-7)
    assert not bool(zero[alive].any()), "an open gate gave a zero gradient"
    assert int(alive.sum()) > 0 and int(closed.sum()) > 0
    assert torch.equal(ref["grad"][closed], torch.zeros_like(ref["grad"][closed]))


@pytest.mark.parametrize("hard", [False, True], ids=["soft", "hard"])
@pytest.mark.parametrize("row", R.GATER_BIG, ids=lambda r: r[0])
def test_gater_grid_stride_trip(built_lib, row, hard):
    p, u1, u2, gout = R.gater_big_inputs(row[1], R.row_seed(row[0]))
    p_min, tau = (0.15, 2.5) if hard else (0.0, 0.3)
    ref = R.gater_host64(p, u1, u2, tau, p_min, 0.5, hard, gout)
    out, gp = _gater_device(p, u1, u2, tau, p_min, hard, gout)
    _gater_values(out, ref, hard, f"gater {row[0]}")
    # element-wise: 1e-3 of max(|ref_i|, 1e-3 max|ref|) as conftest.elem_err has it, plus what the storage format of the saved gate costs:
    # the backward forms m (1 - m) from m held in fp32, so 1 - m is a multiple of 2^-24 and m itself is one rounding (2^-25) of a value
    # computed to about an ulp -- 2^-23 in all; d[m (1 - m)] = |1 - 2m| dm, and the gradient is gout m (1 - m) dlogit / tau with
    # dlogit = 1 / p + 1 / (1 - p) up to 1e6 for a continuous p.  (The edge grid above needs no such term.)
    w, m = ref["grad"], ref["soft"]
    q = p.double().clamp(0.0, 1.0).clamp_min(p_min).clamp(1e-6, 1 - 1e-6)
    fmt = gout.double().abs() * (1 / q + 1 / (1 - q)) / tau * (1 - 2 * m).abs() * 2.0 ** -23 * ref["gate_open"]
    bar = 1e-3 * w.abs().clamp_min(1e-3 * float(w.abs().max())) + fmt
    ratio = (gp.double() - w).abs() / bar
    print(f"gater {row[0]} {'hard' if hard else 'soft'}: gradient element-wise {elem_err(gp, w):.2e}, worst error / bar {float(ratio.max()):.2f}")
    assert float(ratio.max()) <= 1.0
    assert bool((gp[~ref["gate_open"]] == 0).all())
    first = R.constants()["pmg_cap"] * R.constants()["block"]       # from here on only the second grid-stride trip writes
    assert p.numel() > first and float(ratio.reshape(-1)[first:].max()) <= 1.0


# ---- nearest resize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_shape,out_hw", R.RESIZE_ROWS, ids=lambda v: "x".join(map(str, v)))
def test_nearest_resize_grid_stride_rows_bit_exact(built_lib, src_shape, out_hw):
    import mga_yolo_amd.functional as Fn
    from oracle import maskcbam_oracle as MO
    g = torch.Generator().manual_seed(3)
    src = (torch.rand(*src_shape, generator=g) > 0.5).float() + torch.rand(*src_shape, generator=g)
    want = F.interpolate(src, size=out_hw, mode="nearest")
    got = Fn.resize_nearest(src.cuda(), *out_hw).cpu()
    assert torch.equal(got, want)
    assert torch.equal(got, MO.nearest_resize(src, *out_hw))
