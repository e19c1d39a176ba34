"""k_pool forms ca (-m gpu): at the levels the rule picks (csrc/host.cuh: pool_forms_ca) the last workgroup of a sample to arrive in
k_pool runs the shared MLP, and k_gate has no role workgroups and no ca wait for them.  The comparison target is the role-workgroup
path of the same build (MGACBAM_POOL_MLP=0): ca, h_avg, h_mx, y and every gradient bit for bit, the hand-off status word clear; y and
the gradients also against the oracle at the tolerances of tests/test_gpu_parity.py.  MGACBAM_POOL_MLP=2 takes the path at every
shape its MLP takes, however small; "rule" = the knob unset.

Which path ran is observed through the stage calls: after the pool stage ca is overwritten with a constant; role workgroups (or k_chan's
prologue) in the chan|apply call form ca again, a level whose ca k_pool formed keeps the constant.  (The per-sample ca flags count the
k_gate calls under either path -- tile 0 of a sample bumps the flag where no role workgroup does -- so that the two paths can
alternate on one ctx: test_fused_forward_launch_equals_three_launches pins the flags to the call count at the benchmark shapes.)"""
import contextlib
import os

import pytest
import torch

from conftest import elem_err, rel_err, synth
from oracle import maskcbam_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-4                                                   # fp32 vs the oracle, as test_gpu_parity.py
TOL_HALF = {torch.float16: 4e-3, torch.bfloat16: 3e-2}       # as test_gpu_parity.test_half_precision_io
GRADS = ("gx", "gmask", "gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta")
SAVED = ("avg", "mx", "h_avg", "h_mx", "ca", "sa", "cidx")


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()
    return Fn


@contextlib.contextmanager
def knobs(**env):
    """MGACBAM_* knobs for the library calls inside the block (None: unset); the library reads them once, so it is told"""
    from mga_yolo_amd import _lib
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        _lib.reload_env()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.reload_env()


def pool_mlp(v):
    return knobs(MGACBAM_POOL_MLP=v)


def _params(shapes, hiddens, seed=0):
    out = []
    for l, ((B, C, H, W), h) in enumerate(zip(shapes, hiddens)):
        p = O.Params.default_init(C, r=C // h, seed=seed + l)
        assert p.w1.shape[0] == h
        p.beta.fill_(0.3)
        out.append(p)
    return out


def _plan(F, shapes, params, dtype=torch.float32, with_mask=True):
    from mga_yolo_amd.plan import PyramidPlan
    return PyramidPlan(shapes, [(p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta) for p in params],
                       [F.BlockConfig(hidden=p.w1.shape[0]) for p in params], dtype=dtype, with_mask=with_mask)


def _data(shapes, seed, dtype=torch.float32, mask_kind="mixed"):
    out = []
    for l, (B, C, H, W) in enumerate(shapes):
        x, mask, gy = synth(B, C, H, W, seed=seed + l, mask_kind=mask_kind if B > 1 else "randn")    # ("mixed" treats samples 1 and 2)
        out.append((x.to(dtype), mask, gy.to(dtype)))
    return out


def _load(plan, data):
    for l, (x, mask, gy) in enumerate(data):
        plan.x[l].copy_(x); plan.gy[l].copy_(gy)
        if plan.mask[l] is not None:
            plan.mask[l].copy_(mask)


def _status(plan):
    from mga_yolo_amd import _lib
    torch.cuda.synchronize()
    return [int(plan.ctx_view(l)["sync"][_lib.sync_slices(*shp)["status"]].abs().sum()) for l, shp in enumerate(plan.shapes)]


def _arrivals(plan):
    from mga_yolo_amd import _lib
    torch.cuda.synchronize()
    return [int(plan.ctx_view(l)["sync"][_lib.sync_slices(*shp)["arrive"]].abs().sum()) for l, shp in enumerate(plan.shapes)]


def _snap_fwd(plan):
    torch.cuda.synchronize()
    out = []
    for l in range(plan.n):
        v = plan.ctx_view(l)
        d = {k: v[k].clone() for k in SAVED}
        d["y"] = plan.y[l].clone()
        out.append(d)
    return out


def _snap(plan):
    out = _snap_fwd(plan)
    for l, d in enumerate(out):
        d["gx"] = plan.gx[l].clone()
        if plan.gmask[l] is not None:
            d["gmask"] = plan.gmask[l].clone()
        for k, g in plan.named_param_grads(l).items():
            d[k] = g.clone()
    return out


def _diff(got, want, what=""):
    """names of the tensors that are not bit-identical"""
    rep = []
    for l, (a, b) in enumerate(zip(got, want)):
        assert a.keys() == b.keys()
        rep += [f"{what}level {l}: {k}" for k in a if not torch.equal(a[k], b[k])]
    return rep


def _step(plan, data):
    _load(plan, data)
    plan.forward(); plan.backward()
    return _snap(plan)


def _k_pool_formed_ca(plan):
    """Per level: did the pool stage leave ca final?  Pool, overwrite ca, chan|apply: a role workgroup (or a prologue) forms ca again."""
    from mga_yolo_amd import _lib
    S = _lib.FWD_STAGES
    plan.forward(S["pool"])
    torch.cuda.synchronize()
    for l in range(plan.n):
        plan.ctx_view(l)["ca"].fill_(0.25)
    plan.forward(S["chan"] | S["apply"])
    torch.cuda.synchronize()
    kept = [bool((plan.ctx_view(l)["ca"] == 0.25).all()) for l in range(plan.n)]
    plan.forward()                                           # leaves the ctx as a whole forward does
    torch.cuda.synchronize()
    return kept


def _oracle_report(data, params, got, dtype=torch.float32, with_mask=True):
    rep = []
    for l, ((x, mask, gy), p) in enumerate(zip(data, params)):
        x, gy = x.float(), gy.float()
        m = mask if with_mask else None
        y_o, c = O.forward(x, m, p)
        g_o = O.backward(gy, x, m, p, O.Config(), c)
        if dtype == torch.float32:
            # the bound test_gpu_parity.py puts on arbitrary shapes (test_regressions_found_by_the_fuzzer): 1e-4 of the tensor's scale, and
            # for the gradients that are long signed sums (all but gx) a floor of 1e-6 |gy| |x| -- gbeta is ONE sum over B*C*H*W terms, and
            # where it nearly cancels its own value says nothing about the rounding of the sum
            checks = [("y", got[l]["y"], y_o)] + [(k, got[l][k], g_o[k]) for k in GRADS if k in got[l]]
            floor = 1e-6 * float(gy.norm() * x.norm())
            for k, a, b in checks:
                d = float((a.detach().cpu().double() - b.double()).abs().max())
                bar = TOL * float(b.abs().max()) + (floor if k not in ("y", "gx") else 0.0)
                if not d <= bar:
                    rep.append(f"level {l}: {k} |diff| {d:.3e} > {bar:.3e}")
            rep += [f"level {l}: {k} element-wise {elem_err(a, b):.3e}" for k, a, b in checks
                    if k in ("y", "gx") and not elem_err(a, b) < 1e-3]
        else:
            checks = [(k, got[l][k].float(), y_o if k == "y" else g_o[k]) for k in ("y", "gx", "gmask", "gw1", "gbeta")]
            rep += [f"level {l}: {k} {rel_err(a, b):.3e}" for k, a, b in checks if not rel_err(a, b) < TOL_HALF[dtype]]
    return rep


def _both_paths(F, shapes, hiddens, seed, dtype=torch.float32, with_mask=True, knob=2):
    """-> (snapshot under `knob`, snapshot under MGACBAM_POOL_MLP=0, which levels' ca k_pool formed under `knob`, report)"""
    params, data = _params(shapes, hiddens, seed), _data(shapes, 100 + seed, dtype)
    with pool_mlp(0):
        plan = _plan(F, shapes, params, dtype, with_mask)
        ref = _step(plan, data)
        rep = [f"knob 0: status {s}" for s in _status(plan) if s]
        rep += [f"knob 0: k_pool formed ca at level {l}" for l, k in enumerate(_k_pool_formed_ca(plan)) if k]
    with pool_mlp(knob):
        plan = _plan(F, shapes, params, dtype, with_mask)
        got = _step(plan, data)
        again = _step(plan, data)                            # the arrival words came back to 0: a second step counts from there
        rep += [f"status {s}" for s in _status(plan) if s] + [f"arrival words left at {a}" for a in _arrivals(plan) if a]
        kept = _k_pool_formed_ca(plan)
    rep += _diff(got, ref) + _diff(again, ref, "second step, ")
    rep += _oracle_report(data, params, got, dtype, with_mask)
    return got, ref, kept, rep


@pytest.mark.parametrize("shape,hidden", [((1, 64, 16, 16), 4), ((8, 64, 16, 16), 4), ((9, 64, 16, 16), 4), ((17, 64, 16, 16), 4),
                                          ((9, 128, 8, 8), 8), ((9, 128, 8, 8), 16)])
def test_batch_sizes(F, shape, hidden):
    """A full group of 8 samples, a partial last group, workgroup ids past the last sample; one, two and four hidden units per wave."""
    _, _, kept, rep = _both_paths(F, [shape], [hidden], seed=shape[0] + hidden)
    assert kept == [True], "MGACBAM_POOL_MLP=2 did not take the path at this shape: the test would be vacuous"
    assert not rep, "; ".join(rep)


def test_rule_picks_a_level_of_one_mib_per_sample(F):
    """Knob unset: 64 x 64 x 64 fp32 is exactly 1 MiB of x per sample -- k_pool forms its ca, k_gate runs it without role workgroups;
    the level below it (256 KiB per sample) keeps them."""
    shapes, hiddens = [(9, 64, 64, 64), (9, 64, 32, 32)], [4, 4]
    _, _, kept, rep = _both_paths(F, shapes, hiddens, seed=3, knob=None)
    assert kept == [True, False], kept
    assert not rep, "; ".join(rep)


@pytest.mark.parametrize("shape,hidden,with_mask,takes", [((9, 66, 16, 16), 4, True, False),     # C % 4 != 0: the staged MLP
                                                          ((9, 64, 16, 16), 4, False, None)])     # no mask
def test_other_shapes_agree(F, shape, hidden, with_mask, takes):
    _, _, kept, rep = _both_paths(F, [shape], [hidden], seed=11, with_mask=with_mask)
    assert takes is None or kept == [takes], kept
    assert not rep, "; ".join(rep)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision(F, dtype):
    _, _, kept, rep = _both_paths(F, [(9, 64, 16, 16)], [4], seed=21, dtype=dtype)
    assert kept == [True]
    assert not rep, "; ".join(rep)


PYRAMID, PYRAMID_H = [(9, 64, 16, 16), (9, 128, 8, 8), (9, 256, 4, 4)], [4, 8, 16]


def _eager_sequence(F, params, calls, seed):
    """mask_cbam_pyramid / mask_cbam calls with fresh inputs each, on the pooled ctxs of the current knob epoch -> per call {level: tensors}"""
    out = []
    for i, levels in enumerate(calls):
        lv, gys = [], []
        for l in levels:
            x, mask, gy = synth(*PYRAMID[l], seed=seed + 10 * i + l, mask_kind="sparse")
            ps = [t.cuda().requires_grad_(True) for t in (params[l].w1, params[l].b1, params[l].w2, params[l].b2, params[l].wsa, params[l].beta)]
            lv.append((x.cuda().requires_grad_(True), mask.cuda().requires_grad_(True), ps, F.BlockConfig(hidden=PYRAMID_H[l])))
            gys.append(gy.cuda())
        ys = (F.mask_cbam(lv[0][0], lv[0][1], *lv[0][2], lv[0][3]),) if len(lv) == 1 else F.mask_cbam_pyramid(lv)
        torch.autograd.backward(list(ys), gys)
        F.handoff_report()                                   # the status word of every live ctx is clear
        res = {}
        for l, (xd, md, ps, _), y in zip(levels, lv, ys):
            res[l] = dict(y=y.detach(), gx=xd.grad, gmask=md.grad, **{"g" + n: p.grad for n, p in zip(("w1", "b1", "w2", "b2", "wsa", "beta"), ps)})
        out.append(res)
        del ys, lv, y, xd, md, ps                            # the autograd ctx dies here: its pooled buffers go back to the pool
    return out


def test_call_composition_on_pooled_ctx(F):
    """3-level pyramid calls and per-level calls alternated, three rounds, on one pooled ctx per level: the channel grouping of k_pool
    (hence the arrival count a sample needs) follows the call's composition, ca must follow the inputs every time."""
    params = _params(PYRAMID, PYRAMID_H, seed=50)
    calls = [[0, 1, 2], [0], [1], [2]] * 3
    with pool_mlp(0):
        ref = _eager_sequence(F, params, calls, 700)
    with pool_mlp(2):
        got = _eager_sequence(F, params, calls, 700)
        keys = {k for k in F._POOL.free if k[2:6] in [tuple(s) for s in PYRAMID]}
        assert all(len(F._POOL.free[k]) == 1 for k in keys) and len(keys) >= 3, "the calls did not share one pooled ctx per level"
    rep = [f"call {i} level {l}: {k}" for i, (a, b) in enumerate(zip(got, ref)) for l in a for k in a[l] if not torch.equal(a[l][k], b[l][k])]
    assert not rep, "; ".join(rep)


def test_graph_replay_follows_inputs_and_weights(F):
    """A captured forward (k_pool with the MLP tail baked in) replayed three times, x and the weights changed between replays."""
    params = _params(PYRAMID, PYRAMID_H, seed=60)
    with pool_mlp(2):
        plan = _plan(F, PYRAMID, params)
        _load(plan, _data(PYRAMID, 800))
        g = plan.capture(plan.forward)
    with pool_mlp(0):                                         # the graph keeps its kernels; everything launched from here is the role path
        ref = _plan(F, PYRAMID, params)
        rep = []
        for i in range(3):
            data = _data(PYRAMID, 810 + 10 * i, mask_kind="sparse")
            for pl in (plan, ref):
                _load(pl, data)
                for l in range(pl.n):
                    pl.params[l][0].mul_(1.0 + 0.25 * (i + 1)); pl.params[l][3].add_(0.1 * (i + 1))     # W1, b2
                    pl.y[l].zero_()
            g.replay()
            ref.forward()
            rep += _diff(_snap_fwd(plan), _snap_fwd(ref), f"replay {i}, ")
            rep += [f"replay {i}: status {s}" for s in _status(plan) if s]
    assert not rep, "; ".join(rep)


def test_stage_calls(F):
    """pool twice then chan|apply; chan|apply again without a new pool; MGACBAM_POOL_CPT changed between two forwards of one plan."""
    from mga_yolo_amd import _lib
    S = _lib.FWD_STAGES
    params = _params(PYRAMID, PYRAMID_H, seed=70)

    def sequence(knob):
        out = []
        with pool_mlp(knob):
            plan = _plan(F, PYRAMID, params)
            _load(plan, _data(PYRAMID, 900))
            plan.forward(S["pool"])                          # a pool whose results nobody reads ...
            _load(plan, _data(PYRAMID, 910, mask_kind="sparse"))
            plan.forward(S["pool"]); plan.forward(S["chan"] | S["apply"])
            out.append(_snap_fwd(plan))
            for l in range(plan.n):
                plan.y[l].zero_()
            plan.forward(S["chan"] | S["apply"])             # ... and a chan|apply on the ca of the pool before it
            out.append(_snap_fwd(plan))
            for i, cpt in enumerate((1, 2, 4)):
                with knobs(MGACBAM_POOL_CPT=cpt):
                    _load(plan, _data(PYRAMID, 920 + 10 * i))
                    plan.forward()
                    out.append(_snap_fwd(plan))
            assert _status(plan) == [0] * plan.n and _arrivals(plan) == [0] * plan.n
        return out

    got, ref = sequence(2), sequence(0)
    rep = [r for i, (a, b) in enumerate(zip(got, ref)) for r in _diff(a, b, f"step {i}, ")]
    assert not rep, "; ".join(rep)


def test_knob_flipped_between_forwards_on_one_ctx(F):
    """0 -> 2 -> 0 -> 2 -> 0 on one plan, fresh inputs each time: the role path finds its ca flags where its tiles expect them."""
    from mga_yolo_amd import _lib
    params = _params(PYRAMID, PYRAMID_H, seed=80)
    with pool_mlp(0):
        plan, ref = _plan(F, PYRAMID, params), _plan(F, PYRAMID, params)
    rep = []
    for i, knob in enumerate((0, 2, 0, 2, 0)):
        data = _data(PYRAMID, 1000 + 10 * i)
        with pool_mlp(0):
            want = _step(ref, data)
        with pool_mlp(knob):
            rep += _diff(_step(plan, data), want, f"forward {i} (knob {knob}), ")
        rep += [f"forward {i}: status {s}" for s in _status(plan) if s]
        for l, shp in enumerate(plan.shapes):
            sync, r = plan.ctx_view(l)["sync"], _lib.sync_slices(*shp)
            flags = sync[r["gate"]]
            if not (bool((sync[r["ca"]] == i + 1).all()) and int(flags.max()) == i + 1 and set(flags.unique().tolist()) <= {0, i + 1}):
                rep.append(f"forward {i} level {l}: ca flags {sorted(set(sync[r['ca']].tolist()))}, tile flags {sorted(set(flags.tolist()))}")
    assert not rep, "; ".join(rep)
