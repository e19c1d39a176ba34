"""What tests/test_gpu_plan_replays.py and tests/test_gpu_static_plans.py share.  Not a test.

  1. The module-side reference of the layer-loop slice: the modules (build_modules), their tensors in the order the plans take them
     (block_args), and one forward + backward of heads -> [gate] -> blocks -> segmentation loss -> Kendall combine through autograd
     (module_composition).
  2. The replay comparison: a long-lived, captured plan against a fresh plan of the same constructor arguments built from clones of its
     state before every step (fresh_like), on inputs that are new at every step and parameters that moved since the last one (run_row).
     Every output of the two must be the same bits: the kernels are fixed-order, so whatever differs was taken from the
     step before -- a hand-off flag one generation early, an intermediate some tile never rewrote, a parameter read at capture."""
import contextlib
import math
import os
import time
from types import SimpleNamespace

import numpy as np
import torch

from conftest import rel_err

CL = torch.channels_last
SCALE_WEIGHTS = (1.0, 0.5, 2.0)
SEED = 5           # the gate's Philox seed in every gated row
K = 4              # replays per row
BUFFER_NAMES = ("proj.1.running_mean", "proj.1.running_var", "proj.1.num_batches_tracked")


def fmt_of(cl):
    return CL if cl else torch.contiguous_format


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the module-side reference
# ------------------------------------------------------------------------------------------------------------------------------------
def build_modules(block, shapes, hidden, seed=0):
    from mga_yolo_amd import MGAMaskHead, MaskCBAM, MaskECA, MaskSPADE
    heads, blocks = [], []
    for l, ((B, C_, H, W), hid) in enumerate(zip(shapes, hidden)):
        torch.manual_seed(seed + l)
        h = MGAMaskHead(C_, hid)
        h.proj[1].eps, h.proj[1].momentum = 1e-3, 0.03
        torch.manual_seed(seed + 10 + l)
        if block == "cbam":
            b = MaskCBAM(C_)
        elif block == "eca":
            b = MaskECA(C_)
        else:
            b = MaskSPADE(C_, hidden=hid, norm_type="bn" if l == 1 else "in")      # the middle level: batch norm, in training
        if block != "spade":
            with torch.no_grad():
                b.beta.fill_(0.2 * (l - 1))
        heads.append(h.cuda().train()); blocks.append(b.cuda().train())
    return heads, blocks


def block_args(block, blocks):
    """-> (per-level parameters as the plan takes them, configs, running buffers | None)"""
    if block == "cbam":
        return [b.block_params() for b in blocks], [b.block_config() for b in blocks], None
    if block == "eca":
        return [(b.conv1d.weight, b.beta) for b in blocks], [b.eca_config() for b in blocks], None
    running = [(b.norm.running_mean, b.norm.running_var, b.norm.num_batches_tracked) if b.spade_config().bn else None for b in blocks]
    return [b.spade_params() for b in blocks], [b.spade_config() for b in blocks], running


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old


def module_composition(heads, blocks, xs, gys, tgs, det, lv, resize, gate_fn=None):
    """The slice through the modules + autograd on the modules' current state.  gate_fn(level, logits) -> the mask the block reads (a gated
    slice); None: the block reads the logits.  -> xl (leaves: .grad = dL/dx), lvl (leaf: .grad = dL/dlog_vars), logits, masks, ys, total, logs;
    the parameters' .grad and the batch-norm buffers are left on the modules."""
    from mga_yolo_amd import SegLossConfig, SegmentationLoss, kendall_combine
    xl = [x.clone(memory_format=torch.preserve_format).requires_grad_(True) for x in xs]
    lvl = lv.clone().requires_grad_(True)
    logits = [h(x) for h, x in zip(heads, xl)]
    masks = logits if gate_fn is None else [gate_fn(l, m) for l, m in enumerate(logits)]
    ys = [b([x, m]) for b, x, m in zip(blocks, xl, masks)]
    crit = SegmentationLoss(SegLossConfig(scale_weights=SCALE_WEIGHTS))
    # MGA_PROB_MODE: the loss reads targets of another size bilinearly (segmentation.py:103-108)
    with _env("MGA_PROB_MODE", "1" if resize == "bilinear" else None):
        seg_total, logs = crit({k: m for k, m in zip(("p3", "p4", "p5"), logits)}, tgs)
    total = kendall_combine(det, seg_total, lvl)
    torch.autograd.backward([total.sum()] + ys, [None] + gys)
    torch.cuda.synchronize()
    return SimpleNamespace(xl=xl, lvl=lvl, logits=logits, masks=masks, ys=ys, total=total, logs=logs)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. rows, plans and their state
# ------------------------------------------------------------------------------------------------------------------------------------
def row(id, kind, shapes, **opts):
    """kind: 'cbam' | 'eca' | 'spade' (the pyramid plans) | 'slice'.  opts: dtype, cl, use_proj, gate (a GateConfig argument tuple), split (capture
    forward / backward_params / backward_inputs), mask_hw; spade: cases (rows of tests/spade_plan.py); slice: block, hidden, target_hw, resize."""
    o = dict(dtype=torch.float32, cl=False, use_proj=False, gate=None, split=False, mask_hw=None, cases=None, block=None, hidden=None,
             target_hw=None, resize="nearest")
    assert set(opts) <= set(o), opts
    o.update(opts)
    return SimpleNamespace(id=id, kind=kind, shapes=list(shapes), **o)


def block_of(plan):
    return getattr(plan, "block", plan)


def is_slice(plan):
    return hasattr(plan, "head_params")


def is_gated(plan):
    return getattr(block_of(plan), "gate", None) is not None


def _gate(r):
    from mga_yolo_amd import GateConfig
    return None if r.gate is None else [GateConfig(*r.gate)] * len(r.shapes)


def initial_state(r):
    """The modules' tensors as a state of the form snapshot() returns, and the constructor's configs -> (state, cfgs)"""
    state = dict(heads=None, running=None, log_vars=None, rng=None)
    if r.kind == "spade":
        from test_gpu_spade import live_case
        mods = []
        for c in r.cases:
            m = live_case(c.B, c.C, c.H, c.W, c.norm, seed=c.seed, hidden=c.hidden)[0]
            m.norm.eps = c.eps
            if c.norm == "bn":
                m.norm.momentum = c.momentum
            mods.append(m.cuda().train())
        state["params"], cfgs, state["running"] = block_args("spade", mods)
        return state, cfgs
    block = r.block if r.kind == "slice" else r.kind
    hidden = r.hidden if r.hidden is not None else [16, 32, 64][:len(r.shapes)]
    heads, blocks = build_modules(block, r.shapes, hidden)
    state["params"], cfgs, state["running"] = block_args(block, blocks)
    if r.kind == "slice":
        state["heads"] = [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in heads]
        state["log_vars"] = torch.tensor([0.3, -0.4]).cuda()
    return state, cfgs


def make_plan(r, cfgs, state):
    """The row's constructor call on `state`; the plan remembers (row, cfgs) for fresh_like."""
    from mga_yolo_amd import EcaPyramidPlan, PyramidPlan, SlicePlan, SpadePyramidPlan
    if r.kind == "cbam":
        kw = dict(dtype=r.dtype, use_proj=r.use_proj, gate=_gate(r), seed=SEED)
        plan = PyramidPlan.create(r.shapes, state["params"], cfgs, channels_last=True, **kw) if r.cl else PyramidPlan(r.shapes, state["params"], cfgs, **kw)
    elif r.kind == "eca":
        plan = EcaPyramidPlan(r.shapes, state["params"], cfgs, dtype=r.dtype, channels_last=r.cl)
    elif r.kind == "spade":
        plan = SpadePyramidPlan(r.shapes, state["params"], cfgs, dtype=r.dtype, channels_last=r.cl, running=state["running"], mask_hw=r.mask_hw)
    else:
        plan = SlicePlan.create(r.shapes, r.hidden, state["params"], cfgs, state["heads"], block=r.block, channels_last=r.cl,
                                block_running=state["running"], scale_weights=SCALE_WEIGHTS, target_hw=r.target_hw, target_resize=r.resize,
                                dtype=r.dtype, gate=_gate(r), seed=SEED)
        plan.log_vars.copy_(state["log_vars"])
    if state["rng"] is not None:
        block_of(plan).rng_state.copy_(state["rng"])                       # all four words
    plan._replay_row = (r, cfgs)
    return plan


def snapshot(plan):
    """Clones of everything a plan carries from one step to the next, in the form its constructor takes."""
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES
    blk = block_of(plan)
    st = dict(params=[[p.clone() for p in ps] for ps in blk.params], heads=None, running=None, log_vars=None, rng=None)
    if hasattr(blk, "running"):
        st["running"] = [None if run[0] is None else tuple(t.clone() for t in run) for run in blk.running]
    if is_slice(plan):
        st["heads"] = []
        for ps, bufs in zip(plan.head_params, plan.head_buffers):
            sd = {k: p.clone() for k, p in zip(HEAD_PARAM_NAMES, ps)}
            sd.update({k: b.clone() for k, b in zip(BUFFER_NAMES, bufs)})
            st["heads"].append(sd)
        st["log_vars"] = plan.log_vars.clone()
    if is_gated(plan):
        st["rng"] = blk.rng_state.clone()
    return st


def fresh_like(plan, state=None):
    """A new plan of the same constructor arguments on clones of `plan`'s current state: new zero-filled ctx, scratch, ws and sync state."""
    r, cfgs = plan._replay_row
    return make_plan(r, cfgs, snapshot(plan) if state is None else state)


def param_pairs(plan):
    """(name, parameter, its gradient view) of every parameter tensor the plan reads"""
    blk = block_of(plan)
    out = [(f"block{l}.{i}", p, g) for l in range(blk.n) for i, (p, g) in enumerate(zip(blk.params[l], blk.param_grads[l]))]
    if is_slice(plan):
        out += [(f"head{l}.{i}", p, g) for l in range(plan.n) for i, (p, g) in enumerate(zip(plan.head_params[l], plan.head_grads[l]))]
        out.append(("log_vars", plan.log_vars, plan.g_log_vars))
    return out


def update_params(plan):
    """p -= s * g in place with s = 0.05 * max(|p|_max, 0.1) / |g|_max: a perturbation, large and deterministic, not an optimiser.
    Asserts that every tensor moved by at least 1e-3 of its max-norm."""
    for name, p, g in param_pairs(plan):
        pmax, gmax = float(p.abs().max()), float(g.abs().max())
        assert math.isfinite(gmax) and gmax > 0 and math.isfinite(pmax), (name, pmax, gmax)
        old = p.clone()
        p.add_(g, alpha=-(0.05 * max(pmax, 0.1) / gmax))
        moved = float((p - old).abs().max())
        assert moved >= 1e-3 * pmax and moved > 0, (name, moved, pmax)


def make_inputs(r, index, t, gated):
    """Fresh inputs of step t of row `index`, on the device: x, gy scaled by 0.5 + 0.5 t so that pooled maxima, arg-max channels and statistics
    differ in size from step to step; masks randn, gate inputs rand * 1.4 - 0.2; nearest targets rand > 0.3 + 0.15 t, bilinear ones soft."""
    g = torch.Generator().manual_seed(1000 * index + t)
    s = 0.5 + 0.5 * t
    ins = dict(x=[], gy=[], m=[], targets=[], det_loss=None)
    for l, (B, C_, H, W) in enumerate(r.shapes):
        for k in ("x", "gy"):
            ins[k].append((torch.randn(B, C_, H, W, generator=g) * s).to(r.dtype).cuda().contiguous(memory_format=fmt_of(r.cl)))
        if r.kind == "slice":
            th, tw = (H, W) if r.target_hw is None else r.target_hw[l]
            u = torch.rand(B, 1, th, tw, generator=g)
            ins["targets"].append((u if r.resize == "bilinear" else (u > 0.3 + 0.15 * t).float()).cuda())
        else:
            h, w = (H, W) if r.mask_hw is None or r.mask_hw[l] is None else r.mask_hw[l]
            ins["m"].append((torch.rand(B, 1, h, w, generator=g) * 1.4 - 0.2 if gated else torch.randn(B, 1, h, w, generator=g)).cuda())
    if r.kind == "slice":
        ins["det_loss"] = (torch.rand(3, generator=g) * 2.0 + 0.5).cuda()
    return ins


def load_inputs(plan, ins):
    blk = block_of(plan)
    for l in range(blk.n):
        blk.x[l].copy_(ins["x"][l]); blk.gy[l].copy_(ins["gy"][l])
        if is_slice(plan):
            plan.targets[l].copy_(ins["targets"][l])
        elif is_gated(plan):
            blk.logits[l].copy_(ins["m"][l])
        elif getattr(blk, "mask_src", None) is not None and blk.mask_src[l] is not None:
            blk.mask_src[l].copy_(ins["m"][l])
        else:
            blk.mask[l].copy_(ins["m"][l])
    if is_slice(plan):
        plan.det_loss.copy_(ins["det_loss"])


NOT_FRESH = ("num_batches_tracked", "head.num_batches_tracked")     # (they do change; a counter says nothing about the data)


def outputs(plan):
    """[(level | -1, name, tensor)]: everything a step writes that a caller reads"""
    blk = block_of(plan)
    out = []
    for l in range(blk.n):
        for name in ("y", "gx", "gmask", "glogits", "gmask_src", "msoft"):
            seq = getattr(blk, name, None)
            if seq is not None and seq[l] is not None:
                out.append((l, name, seq[l]))
        if is_slice(plan):
            out.append((l, "logits", plan.logits[l]))                  # the heads' output
        elif is_gated(plan):
            out.append((l, "logits", blk.logits[l]))                   # (the gate's input)
        resampled = getattr(blk, "mask_src", None) is not None and blk.mask_src[l] is not None
        if is_gated(plan) or resampled:
            out.append((l, "mask", blk.mask[l]))                       # written by the gate / the resample
        if hasattr(blk, "running") and blk.running[l][0] is not None:
            out += [(l, n, t) for n, t in zip(("running_mean", "running_var", "num_batches_tracked"), blk.running[l])]
        if is_slice(plan):
            out += [(l, n, t) for n, t in zip(("head.running_mean", "head.running_var", "head.num_batches_tracked"), plan.head_buffers[l])]
    out.append((-1, "grad_bucket", plan.grad_bucket))
    if is_gated(plan):
        out.append((-1, "rng_state", blk.rng_state))
    if is_slice(plan):
        out += [(-1, n, getattr(plan, n)) for n in ("total", "seg_out", "g_log_vars", "g_det")]
    return out


def _storages(plan):
    blk = block_of(plan)
    ts = [p for ps in blk.params for p in ps] + list(blk.ctx) + list(blk.scratch) + [plan.grad_bucket]
    ts += [w for w in getattr(blk, "ws", []) if w is not None]
    if hasattr(blk, "running"):
        ts += [t for run in blk.running if run[0] is not None for t in run]
    if is_slice(plan):
        ts += [p for ps in plan.head_params for p in ps] + [b for bs in plan.head_buffers for b in bs]
        ts += list(plan.head_ctx) + list(plan.head_scratch) + [plan.log_vars, plan.seg_ws]
    if is_gated(plan):
        ts.append(blk.rng_state)
    return {t.data_ptr() for t in ts if t.numel() > 0}


def _diff(a, b):
    d = (a.double() - b.double()).abs()
    return float(d.max()), int((a != b).sum())


def run_step(plan, split=False):
    if is_slice(plan):
        plan.step()
    elif split:
        plan.forward(); plan.backward_params(); plan.backward_inputs()
    else:
        plan.forward(); plan.backward()


def check_handoff(plan):
    torch.cuda.synchronize()
    if hasattr(plan, "check_handoff"):           # MaskECA and MaskSPADE have no in-launch hand-off and no status word
        plan.check_handoff()


def run_row(r, index, anchor=False):
    """-> (mismatches [(step, level, name, max |diff|, differing elements)], stale [(step, level, name)], anchor misses [(name, error, bar)]).
    The row's own conditions are asserted on the way."""
    t0 = time.perf_counter()
    state, cfgs = initial_state(r)
    plan = make_plan(r, cfgs, state)
    blk = block_of(plan)
    gated = is_gated(plan)
    load_inputs(plan, make_inputs(r, index, 0, gated))                      # something real for the warm-up run (and for fold_active's step)
    if (r.kind == "cbam" or (r.kind == "slice" and r.block == "cbam")) and not r.cl:
        # k_gate does not save projection planes: a use_proj forward is k_chan + k_apply by design (api_fwd.hip)
        run_step(plan)
        ga, fa = blk.gate_active(), blk.fold_active()
        print(f"{r.id}: gate_active {ga} fold_active {fa}")
        assert ga == (not r.use_proj) and fa, (ga, fa)
    graph = plan.capture(plan.step if is_slice(plan) else (lambda: run_step(plan, r.split)))
    torch.cuda.synchronize()
    s0 = int(blk.rng_state[1]) if gated else None
    counters = [(l, n, t) for l, n, t in outputs(plan) if n in NOT_FRESH]
    n0 = [int(t) for _, _, t in counters]
    report, stale, misses, prev = [], [], [], {}
    for t in range(K):
        ins = make_inputs(r, index, t, gated)
        load_inputs(plan, ins)
        if t:
            update_params(plan)
        st = snapshot(plan)
        fresh = fresh_like(plan, st)
        assert not (_storages(plan) & _storages(fresh)), "the long-lived and the fresh plan share storage"
        load_inputs(fresh, ins)
        graph.replay()
        run_step(fresh)
        check_handoff(plan); check_handoff(fresh)
        for (l, name, a), (l2, name2, b) in zip(outputs(plan), outputs(fresh)):
            assert (l, name) == (l2, name2) and a.data_ptr() != b.data_ptr()
            if not torch.equal(a, b):
                report.append((t, l, name) + _diff(a, b))
            if t and name not in NOT_FRESH and torch.equal(a, prev[(l, name)]):
                stale.append((t, l, name))
            prev[(l, name)] = a.clone()
        if gated:
            assert blk.rng_state.tolist() == [SEED, s0 + t + 1, 0, 0], (t, blk.rng_state.tolist(), s0)
        for (l, n, c), c0 in zip(counters, n0):
            assert int(c) == c0 + t + 1, (t, l, n, int(c), c0)
        if anchor and t == K - 1:
            misses = slice_anchor(r, plan, st, ins)
        del fresh
    torch.cuda.synchronize()
    print(f"{r.id}: {K} replays, {len(report)} mismatches, {len(stale)} stale, {time.perf_counter() - t0:.2f} s")
    return report, stale, misses


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the independent anchor: the module composition on the last step's inputs and the state before that step
# ------------------------------------------------------------------------------------------------------------------------------------
def _uniforms(shape, seed, step, stream_id):
    import philox_ref as PR
    u1, u2 = PR.uniform_arrays(seed, step, stream_id, int(np.prod(shape)))
    return torch.from_numpy(u1).reshape(shape).cuda(), torch.from_numpy(u2).reshape(shape).cuda()


def slice_anchor(r, plan, st, ins):
    """The bars of test_slice_plan_equals_the_module_composition: 1e-6 for total, logits, y and the running statistics, 1e-5 for gx and every
    parameter gradient.  A gated row: the ungated composition with prob_mask_gate on the restatement's uniforms of that step between head and
    block, as test_gated_slice_plan_equals_the_module_composition does.  -> [(name, error, bar)] of the figures past their bar."""
    from mga_yolo_amd import prob_mask_gate
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES
    heads, blocks = build_modules(r.block, r.shapes, r.hidden)
    params, _, running = block_args(r.block, blocks)
    with torch.no_grad():
        for l in range(plan.n):
            sd = dict(heads[l].named_parameters())
            for k in HEAD_PARAM_NAMES:
                sd[k].copy_(st["heads"][l][k])
            bn = heads[l].proj[1]
            for buf, k in zip((bn.running_mean, bn.running_var, bn.num_batches_tracked), BUFFER_NAMES):
                buf.copy_(st["heads"][l][k])
            for p, v in zip(params[l], st["params"][l]):
                p.copy_(v)
            if running is not None and running[l] is not None:
                for buf, v in zip(running[l], st["running"][l]):
                    buf.copy_(v)
    gate_fn = None
    if r.gate is not None:
        mode, tau, p_min, thr = r.gate
        step = int(st["rng"][1])
        gate_fn = lambda l, m: prob_mask_gate(m.float(), *_uniforms(m.shape, SEED, step, l), tau, p_min, thr, hard=mode == "hard_st")
    c = module_composition(heads, blocks, ins["x"], ins["gy"], ins["targets"], ins["det_loss"], st["log_vars"], r.resize, gate_fn)
    misses = []

    def check(name, got, want, bar):
        e, scale = rel_err(got, want), float(want.abs().max())
        print(f"{r.id} anchor {name}: {e:.3e} (bar {bar:.0e}, |reference|_max {scale:.3e})")
        assert scale > 0, name                                          # an all-zero reference would pass any bar
        if not e < bar:
            misses.append((name, e, bar))
    blk = plan.block
    check("total", plan.total, c.total, 1e-6)
    check("g_log_vars", plan.g_log_vars, c.lvl.grad, 1e-5)
    print(f"{r.id} anchor seg_total: plan {float(plan.seg_out[0]):.7f} modules {c.logs['seg_total']:.7f}")
    for l in range(plan.n):
        check(f"logits{l}", plan.logits[l], c.logits[l], 1e-6)
        if r.gate is not None:
            check(f"mask{l}", blk.mask[l], c.masks[l], 1e-6)
        check(f"y{l}", plan.y[l], c.ys[l], 1e-6)
        check(f"gx{l}", plan.gx[l], c.xl[l].grad, 1e-5)
        sd = dict(heads[l].named_parameters())
        for k, gq in zip(HEAD_PARAM_NAMES, plan.head_grads[l]):
            check(f"head{l}.{k}", gq, sd[k].grad, 1e-5)
        for (name, gq), p in zip(blk.named_param_grads(l).items(), params[l]):
            check(f"block{l}.{name}", gq, p.grad, 1e-5)
        check(f"head{l}.running_mean", plan.head_buffers[l][0], heads[l].proj[1].running_mean, 1e-6)
        check(f"head{l}.running_var", plan.head_buffers[l][1], heads[l].proj[1].running_var, 1e-6)
        assert int(plan.head_buffers[l][2]) == int(heads[l].proj[1].num_batches_tracked)
        if running is not None and running[l] is not None:
            check(f"block{l}.running_mean", blk.running[l][0], running[l][0], 1e-6)
            check(f"block{l}.running_var", blk.running[l][1], running[l][1], 1e-6)
            assert int(blk.running[l][2]) == int(running[l][2])
    return misses
