"""The backward forms the W1-projection planes itself (-m gpu).  For an fp32 NCHW level with a mask, dL/dmask wanted and
hidden <= PROJ_MAX_HIDDEN, the k_bwd_reduce1 tiles (stand-alone, folded, or phase 0 of k_bwd_r12) write
P[b,j,hw] = sum_c W1[j,c] x[b,c,hw] into ctx.proj while they stream x, and k_bwd_apply takes the masked-average part of dL/dmask
from those planes instead of reading x a third time.  Checked here: the results against the oracle, the planes themselves,
bit-identity across launch forms and call compositions, and that k_bwd_apply really does not read x of a qualifying level.
Tolerance: 1e-4 relative fp32, what test_gpu_parity.py applies to the use_proj=True plan."""
import pytest
import torch

from conftest import rel_err, synth
from oracle import maskcbam_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()                      # fail loudly if libmgacbam.so is missing
    return Fn


def _make(F, shapes, rs=None, seed=300, **kw):
    """-> (plan, data): a PyramidPlan over `shapes` (rs[l] = reduction ratio of level l, hidden = C // r) with its inputs filled."""
    from mga_yolo_amd.plan import PyramidPlan
    data, params, cfgs = [], [], []
    for l, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=seed + l, mask_kind="mixed")
        p = O.Params.default_init(C, r=(rs[l] if rs else 16), seed=l)
        p.beta.fill_(-0.4)
        data.append((x, mask, gy, p))
        params.append((p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta))
        cfgs.append(F.BlockConfig(hidden=p.w1.shape[0]))
    plan = PyramidPlan(shapes, params, cfgs, **kw)
    for l, (x, mask, gy, _) in enumerate(data):
        plan.x[l].copy_(x); plan.gy[l].copy_(gy)
        if plan.mask[l] is not None:
            plan.mask[l].copy_(mask)
    return plan, data


def _qualifies(plan, l):
    from mga_yolo_amd import _lib
    return plan.gmask[l] is not None and plan.cfgs[l].hidden <= _lib.PROJ_MAX_HIDDEN and plan.dtype == torch.float32


def _outputs(plan):
    torch.cuda.synchronize()
    out = [t.clone() for t in plan.gx] + [t.clone() for t in plan.gmask if t is not None] + [plan.grad_bucket.clone()]
    return out + [plan.ctx_view(l)["proj"].clone() for l in range(plan.n) if _qualifies(plan, l)]


CASES = {
    # name: (shapes, reduction ratios, with_mask, want_gmask)
    "cfg2_b4": ([(4, 64, 80, 80), (4, 128, 40, 40), (4, 256, 20, 20)], None, True, True),   # the benchmark pyramid, reduced batch: only P3 qualifies
    "hidden1": ([(3, 64, 24, 24)], [64], True, True),
    "hidden2": ([(3, 64, 24, 24)], [32], True, True),
    "hidden3": ([(3, 64, 24, 24)], [21], True, True),
    "hidden4": ([(3, 64, 24, 24)], [16], True, True),
    "odd_17x17": ([(3, 48, 17, 17)], None, True, True),                                     # scalar lanes, a partial last tile, hidden 3
    "all_qualify": ([(5, 64, 40, 40), (5, 32, 20, 20), (5, 16, 12, 12)], None, True, True), # hidden 4, 2, 1 in one launch group
    "one_of_two": ([(2, 128, 20, 20), (2, 32, 40, 40)], None, True, True),                  # hidden 8 re-reads x, hidden 2 does not
    "no_mask": ([(4, 64, 40, 40), (4, 128, 20, 20)], None, False, False),
    "no_gmask": ([(4, 64, 40, 40), (4, 128, 20, 20)], None, True, False),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_backward_with_its_own_projection_planes_matches_the_oracle(F, name):
    """gx, gmask and every parameter gradient against the oracle, eagerly and under graph replay; ctx.proj of every qualifying level
    equals einsum("jc,bcn->bjn", W1, x) after the backward; the hand-off status stays clear."""
    shapes, rs, with_mask, want_gmask = CASES[name]
    plan, data = _make(F, shapes, rs, with_mask=with_mask, want_gmask=want_gmask)
    plan.forward(); plan.backward()
    eager = _outputs(plan)
    g = plan.capture(lambda: (plan.forward(), plan.backward()))
    g.replay(); g.replay()
    plan.check_handoff()
    for a, b in zip(eager, _outputs(plan)):
        assert torch.equal(a, b), "graph replay differs from the eager step"
    report = []
    for l, (x, mask, gy, p) in enumerate(data):
        m = mask if with_mask else None
        y_o, c = O.forward(x, m, p)
        g_o = O.backward(gy, x, m, p, O.Config(), c)
        errs = dict(y=rel_err(plan.y[l], y_o), gx=rel_err(plan.gx[l], g_o["gx"]))
        if plan.gmask[l] is not None:
            errs["gmask"] = rel_err(plan.gmask[l], g_o["gmask"])
        for k, v in plan.named_param_grads(l).items():
            errs[k] = rel_err(v, g_o[k])
        if _qualifies(plan, l):
            B, C, H, W = shapes[l]
            want = torch.einsum("jc,bcn->bjn", p.w1.double(), x.double().reshape(B, C, H * W))
            errs["proj"] = rel_err(plan.ctx_view(l)["proj"], want)
        print(name, "level", l, {k: f"{v:.2e}" for k, v in errs.items()})
        report += [f"level {l} {k}: {v:.3e}" for k, v in errs.items() if not v < TOL]
    assert not report, f"{name}: " + "; ".join(report)
    assert any(_qualifies(plan, l) for l in range(plan.n)) == (with_mask and want_gmask), "the case no longer covers what its name says"


@pytest.mark.parametrize("name", ["cfg2_b4", "odd_17x17", "all_qualify"])
def test_every_launch_form_gives_the_same_bits(F, name, monkeypatch):
    """The merged launch (k_bwd_r12), the folded form (MGACBAM_BWD_MERGE=0: k_bwd_reduce1_fold) and the unfolded form (k_bwd_reduce1 +
    k_bwd_convT) share one tile body: gx, gmask, the parameter gradients and the planes are bit-identical."""
    from mga_yolo_amd import _lib
    shapes, rs, with_mask, want_gmask = CASES[name]

    def run():
        plan, _ = _make(F, shapes, rs, with_mask=with_mask, want_gmask=want_gmask)
        for _ in range(2):
            plan.forward(); plan.backward()
        plan.check_handoff()
        return _outputs(plan)

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
    assert len(merged) == len(folded) == len(unfolded)
    for i, (a, b, c) in enumerate(zip(merged, folded, unfolded)):
        assert torch.equal(a, b), f"output {i}: merged != folded"
        assert torch.equal(a, c), f"output {i}: merged != unfolded"


def test_split_backward_calls_equal_one_call(F):
    """backward(the k_bwd_r12 stages) followed by backward(the k_bwd_apply stages) -- what bench.py --full and tools/stage_alone.py do --
    equals one backward() call: producer and consumer decide per level, not per call, whether the planes are used."""
    from mga_yolo_amd import _lib
    shapes, rs, _, _ = CASES["cfg2_b4"]
    plan, _ = _make(F, shapes, rs)
    plan.forward(); plan.backward()
    one = _outputs(plan)
    for t in plan.gx + plan.gmask + [plan.grad_bucket] + [plan.ctx_view(0)["proj"]]:
        t.zero_()
    Bs = _lib.BWD_STAGES
    plan.forward()
    plan.backward(Bs["reduce1"] | Bs["convT"] | Bs["reduce2"] | Bs["wsa"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    plan.backward(Bs["params"] | Bs["apply"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    plan.check_handoff()
    for i, (a, b) in enumerate(zip(one, _outputs(plan))):
        assert torch.equal(a, b), f"output {i}: two calls != one call"
    # and stage by stage, every launch its own call
    for t in plan.gx + plan.gmask + [plan.grad_bucket] + [plan.ctx_view(0)["proj"]]:
        t.zero_()
    plan.forward()
    for s in ("reduce1", "convT", "reduce2", "wsa", "params", "apply"):
        plan.backward(Bs[s])
    for i, (a, b) in enumerate(zip(one, _outputs(plan))):
        assert torch.equal(a, b), f"output {i}: six calls != one call"


def test_a_level_alone_equals_the_level_inside_a_pyramid_on_the_same_ctx(F):
    """Each level of a three-level pyramid, run alone on the ctx and scratch it used inside the pyramid call, gives the pyramid call's bits
    for gx, gmask, its parameter gradients and its planes: whether a level's planes are made and used depends on the level alone.
    (Reduced batch: the sweeps' channel grouping -- group_cpt, which reassociates the hidden-gradient partials -- is 1 alone and
    grouped.  The planes do not depend on that grouping: at the benchmark's full batch, where P3 regroups, they are compared too.)"""
    from mga_yolo_amd.plan import PyramidPlan
    shapes = [(4, 64, 80, 80), (4, 32, 40, 40), (4, 128, 20, 20)]     # hidden 4, 2, 8: two qualify, one re-reads x
    pyr, data = _make(F, shapes)
    pyr.forward(); pyr.backward()
    pyr.check_handoff()
    for l, (B, C, H, W) in enumerate(shapes):
        want = [pyr.gx[l].clone(), pyr.gmask[l].clone()] + [v.clone() for v in pyr.param_grads[l]]
        if _qualifies(pyr, l):
            want.append(pyr.ctx_view(l)["proj"].clone())
            pyr.ctx_view(l)["proj"].zero_()
        solo = PyramidPlan([shapes[l]], [pyr.params[l]], [pyr.cfgs[l]])
        solo.x[0].copy_(pyr.x[l]); solo.mask[0].copy_(pyr.mask[l]); solo.gy[0].copy_(pyr.gy[l])
        for lv in (solo._fwd[0], solo._bwd[0]):                      # the pooled ctx of the pyramid call
            lv.ctx, lv.ctx_bytes = pyr.ctx[l].data_ptr(), pyr.ctx[l].numel()
        solo._bwd[0].scratch, solo._bwd[0].scratch_bytes = pyr.scratch[l].data_ptr(), pyr.scratch[l].numel()
        solo.ctx[0] = pyr.ctx[l]
        solo.forward(); solo.backward()
        solo.check_handoff()
        got = [solo.gx[0], solo.gmask[0]] + list(solo.param_grads[0])
        if _qualifies(pyr, l):
            got.append(pyr.ctx_view(l)["proj"])
        for i, (a, b) in enumerate(zip(want, got)):
            assert torch.equal(a, b), f"level {l} output {i}: alone != inside the pyramid"
    # full batch: P3's sweeps regroup between the two compositions, its planes must not notice
    shapes = [(32, 64, 80, 80), (32, 128, 40, 40), (32, 256, 20, 20)]
    pyr, _ = _make(F, shapes)
    pyr.forward(); pyr.backward()
    planes = pyr.ctx_view(0)["proj"].clone()
    solo = PyramidPlan(shapes[:1], pyr.params[:1], pyr.cfgs[:1])
    solo.x[0].copy_(pyr.x[0]); solo.mask[0].copy_(pyr.mask[0]); solo.gy[0].copy_(pyr.gy[0])
    solo.forward(); solo.backward()
    solo.check_handoff()
    assert torch.equal(planes, solo.ctx_view(0)["proj"])
    assert rel_err(solo.gmask[0], pyr.gmask[0]) < TOL and rel_err(solo.gx[0], pyr.gx[0]) < TOL


def test_apply_stage_does_not_read_x_of_a_qualifying_level(F):
    """Run the first backward launch, overwrite x with NaN, run the apply stage.  For the qualifying level gx and gmask are finite and
    bit-equal to the undisturbed run; for the level that re-reads x the same procedure puts NaN into gmask -- the test can see a read."""
    from mga_yolo_amd import _lib
    shapes, rs, _, _ = CASES["one_of_two"]                           # level 0: hidden 8, level 1: hidden 2
    plan, data = _make(F, shapes, rs)
    assert not _qualifies(plan, 0) and _qualifies(plan, 1)
    Bs = _lib.BWD_STAGES
    first = Bs["reduce1"] | Bs["convT"] | Bs["reduce2"] | Bs["wsa"] | _lib.BWD_FUSE | _lib.BWD_FOLD
    second = Bs["params"] | Bs["apply"] | _lib.BWD_FUSE | _lib.BWD_FOLD
    plan.forward(); plan.backward(first); plan.backward(second)
    torch.cuda.synchronize()
    ref = [(plan.gx[l].clone(), plan.gmask[l].clone()) for l in range(2)]
    plan.forward(); plan.backward(first)
    for l in range(2):
        plan.x[l].fill_(float("nan"))
    plan.backward(second)
    plan.check_handoff()
    assert torch.isfinite(plan.gx[1]).all() and torch.isfinite(plan.gmask[1]).all()
    assert torch.equal(plan.gx[1], ref[1][0]) and torch.equal(plan.gmask[1], ref[1][1])
    assert torch.isnan(plan.gmask[0]).any(), "the level that re-reads x did not see the NaN: this test cannot detect a read"
    assert torch.equal(plan.gx[0], ref[0][0]), "gx needs x in no level"


def test_planes_saved_by_the_forward_are_left_alone(F):
    """MGACBAM_BWD_HAVE_PROJ (PyramidPlan(use_proj=True)): the forward's k_chan saved the planes and the backward tiles skip making
    them -- a ctx.proj overwritten between forward and backward shows in gmask, so the tiles did not rewrite it."""
    shapes, rs, _, _ = CASES["hidden4"]
    plan, data = _make(F, shapes, rs, use_proj=True)
    plan.forward(); plan.backward()
    torch.cuda.synchronize()
    x, mask, gy, p = data[0]
    y_o, c = O.forward(x, mask, p)
    assert rel_err(plan.gmask[0], O.backward(gy, x, mask, p, O.Config(), c)["gmask"]) < TOL
    ref = plan.gmask[0].clone()
    plan.forward()
    plan.ctx_view(0)["proj"].mul_(2.0)
    plan.backward()
    torch.cuda.synchronize()
    assert not torch.equal(plan.gmask[0], ref)
    assert rel_err(plan.ctx_view(0)["proj"], 2.0 * torch.einsum("jc,bcn->bjn", p.w1.double(), x.double().reshape(3, 64, -1))) < TOL


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 3e-2), (torch.float16, 4e-3)])
def test_half_precision_levels_keep_reading_x(F, dtype, tol):
    """The tiles make planes for fp32 levels only (the half-precision step measured slower with them): a bf16 / fp16 level with hidden 4
    leaves ctx.proj untouched, its k_bwd_apply reads x (NaN in x between the two launches reaches gmask), and gmask matches the oracle at
    the half-precision tolerances of test_gpu_parity.py."""
    from mga_yolo_amd import _lib
    shapes, rs, _, _ = CASES["hidden4"]
    plan, data = _make(F, shapes, rs, dtype=dtype)
    assert not _qualifies(plan, 0)
    plan.forward(); plan.backward()
    plan.check_handoff()
    assert not bool(plan.ctx_view(0)["proj"].any()), "a half-precision level wrote projection planes"
    x, mask, gy, p = data[0]
    xh, gyh = x.to(dtype).float(), gy.to(dtype).float()
    y_o, c = O.forward(xh, mask, p)
    g_o = O.backward(gyh, xh, mask, p, O.Config(), c)
    errs = dict(gmask=rel_err(plan.gmask[0], g_o["gmask"]), gx=rel_err(plan.gx[0].float(), g_o["gx"]))
    print(dtype, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(v < tol for v in errs.values()), errs
    Bs = _lib.BWD_STAGES
    plan.forward()
    plan.backward(Bs["reduce1"] | Bs["convT"] | Bs["reduce2"] | Bs["wsa"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    plan.x[0].fill_(float("nan"))
    plan.backward(Bs["params"] | Bs["apply"] | _lib.BWD_FUSE | _lib.BWD_FOLD)
    torch.cuda.synchronize()
    assert torch.isnan(plan.gmask[0]).any()
