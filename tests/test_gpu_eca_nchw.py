"""GPU tests (-m gpu) of MaskECA on NCHW features (csrc/eca.cuh: k_eca_pool, k_eca_apply, k_eca_reduce, k_eca_bwd and its role workgroups),
the path the channels-last kernels, the plans and the slice are measured against: the reference goldens, the rows of
tests/eca_nchw_rows.py at every launch geometry against the fp64 oracle element by element (tests/test_abi_eca_nchw.py checks on the CPU
that the rows have the geometry their comments state), the forced launch geometries, half precision at the benchmark widths,
bit-identity across repeats and call composition, linearity of the backward, and the channel limit k_eca_bwd's LDS sets."""
import pytest
import torch

from conftest import rel_err, synth
from eca_nchw_rows import DT, KNOB_ROWS, ROW_IDS, eca_params, nchw_max_c, oracle, row_case
from oracle import maskeca_oracle as E
from test_gpu_eca_channels_last import HALF_TOL, TOL, _check, _level_run, _run
from test_oracle_eca import ECA_CASES, load_eca

pytestmark = pytest.mark.gpu
NCHW = torch.contiguous_format


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the reference goldens
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ECA_CASES)
def test_goldens_nchw(F, name):
    d = load_eca(name)
    p = E.EcaParams(d["params"]["conv1d.weight"], d["params"]["beta"])
    assert p.w.shape[-1] == d["meta"]["k"]
    y, g = _run(F, d["x"], d["mask"], d["gy"], p, use_sig=d["meta"]["use_sigmoid_mask"], fmt=NCHW, tiny_thr=d["meta"]["tiny_thr"],
                eps=d["meta"]["eps"])
    assert y.is_contiguous() and g["gx"].is_contiguous(), "y / gx came back in another layout"
    rep = []
    for nm, got in (("y", y), ("gx", g["gx"]), ("gw", g["gw"]), ("gbeta", g["gbeta"])) + ((("gmask", g["gmask"]),) if d["mask"] is not None else ()):
        want = d["out"][nm]
        assert got.shape == want.shape, nm
        e = rel_err(got, want)
        print(f"{name} {nm} rel_err {e:.3e}")
        if not e < TOL:
            rep.append(f"{nm} {e:.3e}")
    assert not rep, f"{name}: " + "; ".join(rep)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every launch geometry against the fp64 oracle, element-wise
# ---------------------------------------------------------------------------------------------------------------------------
def _run_row(F, c):
    """One row on the device -> (y, grads), with the checks every row gets on dtypes, layout and the mask gradient's shape."""
    y, g = _run(F, c.x, c.mask, c.gy, c.p, c.use_sig, c.dtype, c.mask_grad, fmt=NCHW, tiny_thr=c.tiny_thr, eps=c.eps)
    assert y.dtype == c.dtype and g["gx"].dtype == c.dtype and y.shape == c.x.shape == g["gx"].shape
    assert y.is_contiguous() and g["gx"].is_contiguous(), f"{c.name}: y / gx came back in another layout"
    assert (g["gmask"] is None) == (c.mask is None or not c.mask_grad)
    if g["gmask"] is not None:
        assert g["gmask"].shape == c.mask.shape and g["gmask"].dtype == torch.float32
    assert g["gw"].dtype == torch.float32 and g["gw"].shape == c.p.w.shape and g["gbeta"].shape == ()
    return y, g


@pytest.mark.parametrize("name", ROW_IDS)
def test_eca_nchw_geometry_row_vs_oracle(F, name):
    """The bars of test_gpu_eca_channels_last._check: fp32 against the fp64 oracle, 1e-4 relative on every output, 1e-3 element-wise on
    y / gx / gmask, gw / gbeta within 1e-4 max|want| + 1e-7 |gy| |x|; fp16 / bf16 against the fp32 oracle on the rounded inputs at
    4e-3 / 3e-2."""
    c = row_case(name)
    y, g = _run_row(F, c)
    _check(name, c.dt, y, g, c.y_o, c.g_o, c.gy, c.x)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. forced launch geometries (cpt 4 and pool_tx / chan_tx untied from H*W are reachable only through the knobs)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [dict(MGACBAM_POOL_TX="16", MGACBAM_POOL_CPT="1", MGACBAM_CHAN_TX="16"),
                                 dict(MGACBAM_POOL_TX="64", MGACBAM_POOL_CPT="4", MGACBAM_CHAN_TX="64"),
                                 dict(MGACBAM_POOL_TX="128", MGACBAM_POOL_CPT="2", MGACBAM_CHAN_TX="32"),
                                 dict(MGACBAM_POOL_TX="256", MGACBAM_POOL_CPT="4", MGACBAM_CHAN_TX="8"),
                                 dict(MGACBAM_POOL_TX="1", MGACBAM_POOL_CPT="1", MGACBAM_CHAN_TX="1")],
                         ids=["tx16_cpt1_ctx16", "tx64_cpt4_ctx64", "tx128_cpt2_ctx32", "tx256_cpt4_ctx8", "tx1_cpt1_ctx1"])
def test_forced_launch_geometries_hold_the_same_bars(F, env, monkeypatch):
    """The knob sets of test_gpu_parity.test_every_launch_geometry_gives_the_same_answer on five rows of the table (fp32, fp16, bf16): each
    holds the row's bars, and a second run under the same knobs gives the same bits."""
    from mga_yolo_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _lib.reload_env()                            # the library reads its knobs once; tell it the environment changed
    try:
        for name in KNOB_ROWS:
            c = row_case(name)
            y, g = _run_row(F, c)
            _check(f"{name} {'/'.join(env.values())}", c.dt, y, g, c.y_o, c.g_o, c.gy, c.x)
            y2, g2 = _run_row(F, c)
            assert torch.equal(y, y2), name
            for k in ("gx", "gmask", "gw", "gbeta"):
                assert torch.equal(g[k], g2[k]), (name, k)
    finally:
        monkeypatch.undo()
        _lib.reload_env()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. half precision at the benchmark widths
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("C,hw", [(64, (40, 40)), (128, (20, 20)), (256, (20, 20)), (256, (10, 10)), (48, (17, 17))])
def test_half_precision_nchw(F, C, hw, dt):
    """The NCHW twin of test_half_precision_channels_last: the benchmark widths (8-byte accesses) and 48 x 17 x 17 (scalar), against the
    fp32 oracle on the rounded inputs; the mask gradient is fp32."""
    dtype, tol = DT[dt], HALF_TOL[dt]
    B, (H, W) = 4, hw
    x, mask, gy = synth(B, C, H, W, seed=21)
    x, gy = x.to(dtype).float(), gy.to(dtype).float()
    p = eca_params(E.eca_kernel_size(C), seed=C)
    y_o, g_o = oracle(x, mask, gy, p, True, double=False)
    y, g = _run(F, x, mask, gy, p, dtype=dtype, fmt=NCHW)
    assert y.dtype == dtype and g["gx"].dtype == dtype and y.is_contiguous() and g["gx"].is_contiguous()
    assert g["gmask"].dtype == torch.float32 and g["gw"].dtype == torch.float32 and g["gbeta"].dtype == torch.float32
    rep = []
    for k, got, want in (("y", y.float(), y_o), ("gx", g["gx"].float(), g_o["gx"]), ("gmask", g["gmask"], g_o["gmask"]), ("gw", g["gw"], g_o["gw"]),
                         ("gbeta", g["gbeta"], g_o["gbeta"])):
        e = rel_err(got, want)
        print(f"{dt} C={C} {H}x{W} {k} rel_err {e:.3e}")
        if not e < tol:
            rep.append(f"{k} {e:.3e}")
    assert not rep, "; ".join(rep)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. bits
# ---------------------------------------------------------------------------------------------------------------------------
def test_repeat_is_bit_identical(F):
    B, C, H, W = 32, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=9)
    p = eca_params(5, seed=2)
    w, beta, cfg = p.w.cuda(), p.beta.cuda(), F.EcaConfig(k=5)
    xd, md, gd = x.cuda(), mask.cuda(), gy.cuda()
    first = _level_run(F, xd, md, w, beta, cfg, gd)
    again = _level_run(F, xd, md, w, beta, cfg, gd)
    assert first[0].is_contiguous() and first[1].is_contiguous()
    for i, (a, b) in enumerate(zip(first, again)):            # y, gx, gmask, gw, gbeta
        assert torch.equal(a, b), i


def test_pyramid_level_equals_the_single_call(F):
    """Three NCHW levels of different launch signatures (fp32 vec 4, fp32 vec 1, bf16), so three launch groups in one call: each level's
    y, gx, gmask, gw and gbeta are the bits of the level called alone."""
    specs = [((4, 64, 40, 40), torch.float32), ((4, 48, 17, 17), torch.float32), ((4, 128, 20, 20), torch.bfloat16)]
    data = []
    for i, ((B, C, H, W), dtype) in enumerate(specs):
        x, mask, gy = synth(B, C, H, W, seed=30 + i, mask_kind="mixed")
        p = eca_params(E.eca_kernel_size(C), seed=i)
        data.append((x.cuda().to(dtype), mask.cuda(), p.w.cuda(), p.beta.cuda(), F.EcaConfig(k=p.w.shape[-1]), gy.cuda().to(dtype)))
    leaves = [(x.clone().requires_grad_(True), m.clone().requires_grad_(True), w.clone().requires_grad_(True), beta.clone().requires_grad_(True), cfg)
              for x, m, w, beta, cfg, _ in data]
    ys = F.mask_eca_pyramid(leaves)
    torch.autograd.backward(ys, [d[5] for d in data])
    torch.cuda.synchronize()
    for i, ((x, m, w, beta, cfg, gy), (xl, ml, wl, bl, _), y) in enumerate(zip(data, leaves, ys)):
        single = _level_run(F, x, m, w, beta, cfg, gy)
        together = [y.detach(), xl.grad, ml.grad, wl.grad, bl.grad]
        assert y.is_contiguous() and xl.grad.is_contiguous() and y.dtype == specs[i][1], i
        for j, (a, b) in enumerate(zip(together, single)):
            assert torch.equal(a, b), (i, j)


def test_backward_is_linear_in_gy_nchw(F):
    """bwd(-2.5 gy) = -2.5 bwd(gy), at the 1e-5 of test_gpu_parity.test_backward_is_linear_in_gy (no oracle needed)."""
    B, C, H, W = 8, 64, 40, 40
    x, mask, gy = synth(B, C, H, W, seed=9, mask_kind="sparse")
    p = eca_params(5, seed=4)
    _, g1 = _run(F, x, mask, gy, p, fmt=NCHW)
    _, g2 = _run(F, x, mask, -2.5 * gy, p, fmt=NCHW)
    for k in ("gx", "gmask", "gw", "gbeta"):
        e = rel_err(g2[k], -2.5 * g1[k])
        print(f"{k} linearity rel_err {e:.3e}")
        assert e < 1e-5, k


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the channel limit of an NCHW level
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_widest_level_runs_and_one_channel_more_is_refused_at_the_forward(F):
    """A forward must never succeed whose backward cannot be launched.  C = the limit: forward and backward run (k_eca_bwd asks for all
    but 4 of the 64 KB of LDS) and hold the fp32 bars.  One channel more: mask_eca raises at the forward, naming the limit, and no kernel
    of the library has been launched."""
    from torch.profiler import ProfilerActivity, profile
    limit = nchw_max_c()
    B, H, W, k = 1, 2, 2, 7
    x, mask, gy = synth(B, limit, H, W, seed=88)
    p = eca_params(k, seed=8)
    y_o, g_o = oracle(x, mask, gy, p, True, double=True)
    y, g = _run(F, x, mask, gy, p, fmt=NCHW)
    _check(f"C={limit}", "f32", y, g, y_o, g_o, gy, x)
    x, mask, _ = synth(B, limit + 1, H, W, seed=88)
    xd, md = x.cuda().requires_grad_(True), mask.cuda().requires_grad_(True)
    w, beta = p.w.cuda().requires_grad_(True), p.beta.cuda().requires_grad_(True)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        with pytest.raises(RuntimeError, match=f"an NCHW level takes C <= {limit}"):
            F.mask_eca(xd, md, w, beta, F.EcaConfig(k=k))
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name == "CUDA"]
    assert not [n for n in names if "k_eca" in n or "mgacbam" in n], names
