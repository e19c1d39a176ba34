"""W1-projection planes for 4 < hidden <= 16, formed on the matrix cores (-m gpu).  An fp32 NCHW level with dL/dmask wanted, H*W % 4 == 0,
16-lane tiles (chan_tx 16) and at least 1 MiB of x gets P[b,j,hw] = sum_c W1[j,c] x[b,c,hw] from the k_bwd_reduce1 tiles -- one
v_mfma_f32_16x16x4_f32 per channel step and vector element -- into the LAST region of its backward scratch, and k_bwd_apply reads those
planes instead of x.  A launch group in which every level has planes runs the k_bwd_apply instantiation that cannot read x.
Checked here: the planes themselves, the results against the oracle, bit-identity across launch forms, call splits, call compositions
(which covers both k_bwd_apply instantiations) and graph replay, and that the apply stage reads x exactly where the rule says it does.
Tolerance against the oracle: 1e-4 relative fp32, that of test_gpu_bwd_proj.py.  Planes: 4 x the error of torch's own fp32 einsum on
the same inputs, both against float64 -- the factor covers the different association order of at most 256 terms."""
import pytest
import torch

from conftest import rel_err, synth
from oracle import maskcbam_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4
R = 16          # reduction ratio of every level here: hidden = C // 16

QUALIFY = {
    "hidden8_floor": (2, 128, 32, 32),     # exactly 1 MiB of x: the size floor itself
    "hidden16": (2, 256, 24, 24),
    "hidden6": (3, 96, 32, 32),            # rows 6..15 of the A operand are zero
    "hidden5_partial": (5, 80, 27, 28),    # 189 vectors: the last 16-lane tile is partial
}
SCALAR = (4, 128, 23, 23)                  # H*W % 4 != 0: scalar lanes, reads x
SMALL = (2, 128, 20, 20)                   # below the size floor, reads x


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()                      # fail loudly if libmgacbam.so is missing
    return Fn


def _make(F, shapes, seed=700, **kw):
    """-> (plan, data): a PyramidPlan over `shapes` (hidden = C // 16) with its inputs filled."""
    from mga_yolo_amd.plan import PyramidPlan
    data, params, cfgs = [], [], []
    for l, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=seed + l, mask_kind="mixed")
        p = O.Params.default_init(C, r=R, seed=l)
        p.beta.fill_(-0.4)
        data.append((x, mask, gy, p))
        params.append((p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta))
        cfgs.append(F.BlockConfig(hidden=p.w1.shape[0]))
    plan = PyramidPlan(shapes, params, cfgs, **kw)
    for l, (x, mask, gy, _) in enumerate(data):
        plan.x[l].copy_(x); plan.gy[l].copy_(gy); plan.mask[l].copy_(mask)
    return plan, data


def _planes(plan, l):
    """The level's planes: (B, hidden, HW) fp32, the last region of its scratch buffer (host.cuh: scratch_layout)."""
    B, C, H, W = plan.shapes[l]
    n = B * plan.cfgs[l].hidden * H * W * 4
    assert n % 16 == 0
    return plan.scratch[l][plan.scratch[l].numel() - n:].view(torch.float32).view(B, plan.cfgs[l].hidden, H * W)


def _outputs(plan, with_planes=()):
    torch.cuda.synchronize()
    out = [t.clone() for t in plan.gx] + [t.clone() for t in plan.gmask] + [plan.grad_bucket.clone()]
    return out + [_planes(plan, l).clone() for l in with_planes]


@pytest.mark.parametrize("name", sorted(QUALIFY))
def test_planes_and_gradients_of_a_qualifying_level(F, name):
    """The planes against einsum("jc,bcn->bjn", W1, x) in float64, bounded by 4 x the error of torch's fp32 einsum; gx, gmask and every
    parameter gradient against the oracle; graph replay equals the eager step; the hand-off status stays clear."""
    shape = QUALIFY[name]
    plan, data = _make(F, [shape])
    plan.forward(); plan.backward()
    eager = _outputs(plan, [0])
    g = plan.capture(lambda: (plan.forward(), plan.backward()))
    g.replay(); g.replay()
    plan.check_handoff()
    for a, b in zip(eager, _outputs(plan, [0])):
        assert torch.equal(a, b), "graph replay differs from the eager step"
    x, mask, gy, p = data[0]
    B, C, H, W = shape
    xr = x.reshape(B, C, H * W)
    want = torch.einsum("jc,bcn->bjn", p.w1.double(), xr.double())
    ref_err = float((torch.einsum("jc,bcn->bjn", p.w1, xr).double() - want).abs().max())
    got_err = float((_planes(plan, 0).double().cpu() - want).abs().max())
    print(name, f"planes: max |err| {got_err:.3e}, torch fp32 einsum {ref_err:.3e}, scale {float(want.abs().max()):.3e}")
    y_o, c = O.forward(x, mask, p)
    g_o = O.backward(gy, x, mask, p, O.Config(), c)
    errs = dict(y=rel_err(plan.y[0], y_o), gx=rel_err(plan.gx[0], g_o["gx"]), gmask=rel_err(plan.gmask[0], g_o["gmask"]))
    for k, v in plan.named_param_grads(0).items():
        errs[k] = rel_err(v, g_o[k])
    print(name, {k: f"{v:.2e}" for k, v in errs.items()})
    assert ref_err > 0 and got_err <= 4 * ref_err, f"planes: {got_err:.3e} against 4 x {ref_err:.3e}"
    bad = {k: v for k, v in errs.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", ["hidden8_floor", "hidden5_partial"])
def test_every_launch_form_gives_the_same_bits(F, name, monkeypatch):
    """Merged (k_bwd_r12), folded (k_bwd_reduce1_fold) and unfolded (k_bwd_reduce1 + k_bwd_convT) launches share one tile body."""
    from mga_yolo_amd import _lib

    def run():
        plan, _ = _make(F, [QUALIFY[name]])
        for _ in range(2):
            plan.forward(); plan.backward()
        plan.check_handoff()
        return _outputs(plan, [0])

    merged = run()
    try:
        monkeypatch.setenv("MGACBAM_BWD_MERGE", "0")
        _lib.reload_env()
        folded = run()
        monkeypatch.setenv("MGACBAM_FOLD_BWD", "0")             # PyramidPlan: no MGACBAM_BWD_FOLD bit -> separate launches
        unfolded = run()
    finally:
        monkeypatch.undo()
        _lib.reload_env()
    for i, (a, b, c) in enumerate(zip(merged, folded, unfolded)):
        assert torch.equal(a, b), f"output {i}: merged != folded"
        assert torch.equal(a, c), f"output {i}: merged != unfolded"


def test_split_backward_calls_equal_one_call(F):
    """The tile stages in one call and the apply stages in a later one, then every stage a call of its own: producer and consumer decide
    by the level alone whether its planes exist."""
    from mga_yolo_amd import _lib
    shapes = [QUALIFY["hidden16"], SMALL]
    plan, _ = _make(F, shapes)
    plan.forward(); plan.backward()
    one = _outputs(plan, [0])
    Bs = _lib.BWD_STAGES

    def clear():
        for t in plan.gx + plan.gmask + [plan.grad_bucket, _planes(plan, 0)]:
            t.zero_()

    clear()
    plan.forward()
    plan.backward(Bs["reduce1"] | Bs["convT"] | Bs["reduce2"] | Bs["wsa"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    plan.backward(Bs["params"] | Bs["apply"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    plan.check_handoff()
    for i, (a, b) in enumerate(zip(one, _outputs(plan, [0]))):
        assert torch.equal(a, b), f"output {i}: two calls != one call"
    clear()
    plan.forward()
    for s in ("reduce1", "convT", "reduce2", "wsa", "params", "apply"):
        plan.backward(Bs[s])
    for i, (a, b) in enumerate(zip(one, _outputs(plan, [0]))):
        assert torch.equal(a, b), f"output {i}: six calls != one call"


def test_a_level_alone_equals_the_level_inside_a_mixed_pyramid(F):
    """A qualifying level beside a level that reads x runs the k_bwd_apply instantiation that can read x; alone, on the same ctx and
    scratch, the one that cannot.  gx, gmask, the parameter gradients and the planes are the same bits.  (Small batches: the sweeps'
    channel grouping is 1 in both compositions.)"""
    from mga_yolo_amd.plan import PyramidPlan
    shapes = [QUALIFY["hidden8_floor"], SMALL, QUALIFY["hidden6"]]
    pyr, _ = _make(F, shapes)
    pyr.forward(); pyr.backward()
    pyr.check_handoff()
    for l in (0, 2):
        want = [pyr.gx[l].clone(), pyr.gmask[l].clone()] + [v.clone() for v in pyr.param_grads[l]] + [_planes(pyr, l).clone()]
        _planes(pyr, l).zero_()
        solo = PyramidPlan([shapes[l]], [pyr.params[l]], [pyr.cfgs[l]])
        solo.x[0].copy_(pyr.x[l]); solo.mask[0].copy_(pyr.mask[l]); solo.gy[0].copy_(pyr.gy[l])
        assert solo.scratch[0].numel() == pyr.scratch[l].numel()
        for lv in (solo._fwd[0], solo._bwd[0]):                      # the ctx and scratch of the pyramid call
            lv.ctx, lv.ctx_bytes = pyr.ctx[l].data_ptr(), pyr.ctx[l].numel()
        solo._bwd[0].scratch, solo._bwd[0].scratch_bytes = pyr.scratch[l].data_ptr(), pyr.scratch[l].numel()
        solo.ctx[0] = pyr.ctx[l]
        solo.forward(); solo.backward()
        solo.check_handoff()
        got = [solo.gx[0], solo.gmask[0]] + list(solo.param_grads[0]) + [_planes(pyr, l)]
        for i, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), f"level {l} output {i}: alone != inside the pyramid"


def _nan_probe(F, shapes):
    """Tile stages, x := NaN, apply stages -> per level (gx, gmask) of the undisturbed run and of the disturbed one."""
    from mga_yolo_amd import _lib
    plan, _ = _make(F, shapes)
    Bs = _lib.BWD_STAGES
    first = Bs["reduce1"] | Bs["convT"] | Bs["reduce2"] | Bs["wsa"] | _lib.BWD_FUSE | _lib.BWD_FOLD
    second = Bs["params"] | Bs["apply"] | _lib.BWD_FUSE | _lib.BWD_FOLD
    plan.forward(); plan.backward(first); plan.backward(second)
    torch.cuda.synchronize()
    ref = [(plan.gx[l].clone(), plan.gmask[l].clone()) for l in range(plan.n)]
    plan.forward(); plan.backward(first)
    for l in range(plan.n):
        plan.x[l].fill_(float("nan"))
    plan.backward(second)
    plan.check_handoff()
    torch.cuda.synchronize()
    return ref, [(plan.gx[l], plan.gmask[l]) for l in range(plan.n)]


def test_apply_stage_reads_x_only_where_the_rule_says(F):
    """Qualifying levels: gx and gmask finite and bit-equal to the undisturbed run, alone (no lane can read x) and beside levels that
    read x.  The scalar-lane level and the level below the size floor: NaN reaches gmask -- the test can see a read."""
    for shapes, qualifies in (([QUALIFY["hidden16"]], [True]),
                              ([QUALIFY["hidden8_floor"], SCALAR, SMALL, QUALIFY["hidden5_partial"]], [True, False, False, True])):
        ref, got = _nan_probe(F, shapes)
        for l, q in enumerate(qualifies):
            assert torch.equal(got[l][0], ref[l][0]), f"level {l}: gx needs x in no level"
            if q:
                assert torch.isfinite(got[l][1]).all(), f"level {l}: the apply stage read x"
                assert torch.equal(got[l][1], ref[l][1])
            else:
                assert torch.isnan(got[l][1]).any(), f"level {l} re-reads x but did not see the NaN"


def test_wider_tiles_keep_reading_x(F, monkeypatch):
    """MGACBAM_CHAN_TX=32: a wave of the tiles is no longer 4 channel rows x 16 lanes, the hidden-8 level gets no planes (and no room
    for them in its scratch), its apply stage reads x and its gmask still matches the oracle."""
    from mga_yolo_amd import _lib
    shape = QUALIFY["hidden8_floor"]
    B, C, H, W = shape
    default = _lib.scratch_bytes(B, C, H, W, C // R, 7)
    try:
        monkeypatch.setenv("MGACBAM_CHAN_TX", "32")
        _lib.reload_env()
        assert _lib.scratch_bytes(B, C, H, W, C // R, 7) < default - B * (C // R) * H * W * 4 + (1 << 16)
        ref, got = _nan_probe(F, [shape])
        assert torch.equal(got[0][0], ref[0][0])
        assert torch.isnan(got[0][1]).any(), "the level has 32-lane tiles but its apply stage did not read x"
        plan, data = _make(F, [shape])
        plan.forward(); plan.backward()
        plan.check_handoff()
        x, mask, gy, p = data[0]
        y_o, c = O.forward(x, mask, p)
        assert rel_err(plan.gmask[0], O.backward(gy, x, mask, p, O.Config(), c)["gmask"]) < TOL
    finally:
        monkeypatch.undo()
        _lib.reload_env()
