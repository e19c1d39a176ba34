"""Call-composition invariance (-m gpu): a level's results must not depend on the levels that share its call, nor on the calls its
pooled ctx has seen before.  The hand-off counters in ctx.sync are never reset, so every launch derives the generation it waits for
from a counter's current value; that is only sound if the counters advance the same way under every composition of a call.  The
merged backward launch (k_bwd_r12) sizes its sweep channel groups with one cpt for the whole launch group (group_cpt sums
workgroups over ALL levels of the call), so the same level gets a different channel grouping alone (mask_cbam) than inside a
pyramid call (mask_cbam_pyramid), or when a mask.requires_grad flip regroups the levels -- on the same pooled ctx."""
import pytest
import torch

from conftest import elem_err, rel_err, synth
from oracle import maskcbam_oracle as O
from oracle import maskeca_oracle as E

pytestmark = pytest.mark.gpu

TOL = 1e-4          # fp32 vs the oracle, as test_gpu_parity.py
TOL_BF16 = 3e-2     # as test_gpu_parity.test_half_precision_io
GRADS = ("gx", "gmask", "gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta")
LEVELS = {"cfg2": [(32, 64, 80, 80), (32, 128, 40, 40), (32, 256, 20, 20)],       # BASELINE configs[1] / [2] widths at B = 32
          "cfg3": [(32, 128, 80, 80), (32, 256, 40, 40), (32, 512, 20, 20)]}


@pytest.fixture(scope="module")
def F():
    import mga_yolo_amd.functional as Fn
    from mga_yolo_amd import _lib
    _lib.load()                      # fail loudly if libmgacbam.so is missing
    return Fn


def _params(shapes):
    out = []
    for l, (B, C, H, W) in enumerate(shapes):
        p = O.Params.default_init(C, seed=40 + l)
        p.beta.fill_(0.3)
        out.append(p)
    return out


def _dev(p):
    return [t.cuda() for t in (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)]


def _pool_key(F, shape, hidden, dtype=torch.float32, k=7):
    from mga_yolo_amd import _lib
    dev = torch.device("cuda", torch.cuda.current_device())
    B, C, H, W = shape
    return (dev.index, F._raw_stream(dev), B, C, H, W, hidden, dtype, _lib.ENV_EPOCH, k)   # as _PyramidFn.forward builds it


def _sweep_cpb(shapes):
    """Channels per k_bwd_r12 sweep workgroup for one launch group of fp32 levels under the default knobs: choose_tune's pool_tx and
    group_cpt (host.cuh), restated."""
    def tx_of(H, W):
        nv = H * W // (4 if H * W % 4 == 0 else 1)
        t = 1
        while 2 * t <= max(nv // 4, 1):
            t *= 2
        return min(t, 256)
    cpt = 1
    for c in (4, 2):
        if sum(B * -(-C // ((256 // tx_of(H, W)) * c)) for B, C, H, W in shapes) >= 1536:
            cpt = c
            break
    return [(256 // tx_of(H, W)) * cpt for B, C, H, W in shapes]


def _fwd_bwd(F, shapes, params, seed, levels):
    lv, gys = [], []
    for l in levels:
        B, C, H, W = shapes[l]
        x, mask, gy = synth(B, C, H, W, seed=seed + l, mask_kind="sparse")
        lv.append((x.cuda().requires_grad_(True), mask.cuda().requires_grad_(True), [t.requires_grad_(True) for t in _dev(params[l])],
                   F.BlockConfig(hidden=params[l].w1.shape[0])))
        gys.append(gy.cuda())
    ys = (F.mask_cbam(lv[0][0], lv[0][1], *lv[0][2], lv[0][3]),) if len(lv) == 1 else F.mask_cbam_pyramid(lv)
    torch.autograd.backward(list(ys), gys)
    del ys, lv                       # the autograd ctx dies here: its pooled buffers go back to the pool
    torch.cuda.synchronize()


@pytest.mark.parametrize("order", ["single_first", "pyramid_first"])
@pytest.mark.parametrize("widths", ["cfg2", "cfg3"])
def test_sweep_generations_count_merged_launches_under_any_composition(F, widths, order):
    """P3 alone / P3+P4+P5 / P3 alone (or the reverse) on ONE pooled ctx: afterwards the generation every sweep of the next merged
    launch derives -- under either channel grouping -- must be 3, the number of merged launches the ctx has seen.  A counter per
    channel group lags wherever a grouping with fewer groups ran, and the next sweep of such a group stops waiting at once."""
    from mga_yolo_amd import _lib
    shapes = LEVELS[widths]
    params = _params(shapes)
    B, C, H, W = shapes[0]
    hidden = params[0].w1.shape[0]
    key = _pool_key(F, shapes[0], hidden)
    cpb_single, cpb_group = _sweep_cpb(shapes[:1])[0], _sweep_cpb(shapes)[0]
    assert cpb_single != cpb_group, "these widths no longer regroup P3: the test would not exercise a composition change"
    F._POOL.free.pop(key, None)      # a fresh zero-filled ctx: its counters count this test's launches only
    seq = [[0], [0, 1, 2], [0]] if order == "single_first" else [[0, 1, 2], [0], [0, 1, 2]]
    ptr = None
    for i, levels in enumerate(seq):
        _fwd_bwd(F, shapes, params, 500 + 10 * i, levels)
        free = F._POOL.free.get(key) or []
        assert len(free) == 1, f"call {i}: P3's ctx did not come back to the pool ({len(free)} buffers)"
        assert ptr is None or free[0].data_ptr() == ptr, f"call {i}: P3 did not reuse its pooled ctx -- the test would be vacuous"
        ptr = free[0].data_ptr()
    F.handoff_report()
    sync = F.ctx_views(F._POOL.free[key][0], B, C, H, W, hidden)["sync"].cpu()
    r = _lib.sync_slices(B, C, H, W)
    tiles = sync[r["merged_tiles"]]
    assert int(tiles.max()) == 3, "the backward did not run as the merged launch three times"
    sweeps = sync[r["sweeps"]].reshape(B, C)
    for name, cpb in (("alone", cpb_single), ("grouped", cpb_group)):
        gen = sweeps[:, ::cpb]                                   # a sweep of channel group cg reads the counter of channel cg * cpb
        lag = (gen != 3).nonzero().tolist()
        assert not lag, (f"{widths} P3 {name} (cpb {cpb}): {len(lag)} of {gen.numel()} sweep generations are not 3 "
                         f"(sample, group) {lag[:8]}, values {sorted(set(gen.flatten().tolist()))}")
    assert bool((sweeps == 3).all()), "every channel's counter counts the merged launches"


# ---------------------------------------------------------------------------------------------------------
# behaviour: fresh inputs at every call, so that a read of the previous call's hand-off data shows as a wrong number
# ---------------------------------------------------------------------------------------------------------
def _tied_samples(x, ca):
    """Samples with a channel arg-max decided by less than the last bits of ca (tests/fuzz/fuzz_pyramid.py): the routed
    sub-gradient may go to either channel on the device, so their gy is zeroed on both sides."""
    B, C = ca.shape
    if C < 2:
        return torch.zeros(B, dtype=torch.bool)
    u2 = (x * ca.reshape(B, C, 1, 1)).topk(2, dim=1).values
    return ((u2[:, 0] - u2[:, 1]) <= 2e-6 * u2[:, 0].abs()).flatten(1).any(dim=1)


class _Seq:
    """A sequence of MaskCBAM calls on the default stream.  calls[i] = [(level, mask_requires_grad), ...]; every call draws fresh
    x, mask and gy.  `oracle` = the (call, level) pairs checked against the fp64 oracle."""

    def __init__(self, shapes, calls, dtype, oracle):
        self.shapes, self.calls, self.dtype = shapes, calls, dtype
        self.params = _params(shapes)
        self.data, self.ref = [], {}
        for i, call in enumerate(calls):
            d = {}
            for l, _ in call:
                B, C, H, W = shapes[l]
                x, mask, gy = synth(B, C, H, W, seed=900 + 10 * i + l, mask_kind="sparse")
                x, gy = x.to(dtype).double(), gy.to(dtype).double()
                if (i, l) in oracle:
                    p64 = self.params[l].to(torch.float64)
                    y_o, c = O.forward(x, mask.double(), p64)
                    gy[_tied_samples(x, c.ca)] = 0
                    self.ref[(i, l)] = (y_o, c)
                d[l] = (x, mask, gy)
            self.data.append(d)

    def run(self, F):
        out = []
        for i, call in enumerate(self.calls):
            lv, gys = [], []
            for l, mg in call:
                x, mask, gy = self.data[i][l]
                lv.append((x.cuda().to(self.dtype).requires_grad_(True), mask.cuda().requires_grad_(mg),
                           [t.requires_grad_(True) for t in _dev(self.params[l])], F.BlockConfig(hidden=self.params[l].w1.shape[0])))
                gys.append(gy.cuda().to(self.dtype))
            ys = (F.mask_cbam(lv[0][0], lv[0][1], *lv[0][2], lv[0][3]),) if len(lv) == 1 else F.mask_cbam_pyramid(lv)
            torch.autograd.backward(list(ys), gys)
            F.handoff_report()                                   # the status word of every live ctx is clear
            res = {}
            for (l, _), (xd, md, ps, _), y in zip(call, lv, ys):
                res[l] = dict(y=y.detach(), gx=xd.grad, gmask=md.grad, gw1=ps[0].grad, gb1=ps[1].grad, gw2=ps[2].grad, gb2=ps[3].grad,
                              gwsa=ps[4].grad, gbeta=ps[5].grad)
            out.append(res)
            del ys, lv
        return out

    def per_level_forward(self, F, i, l):
        x, mask, _ = self.data[i][l]
        with torch.no_grad():
            return F.mask_cbam(x.cuda().to(self.dtype), mask.cuda(), *_dev(self.params[l]), F.BlockConfig(hidden=self.params[l].w1.shape[0]))

    def oracle_report(self, i, l, got):
        x, mask, gy = self.data[i][l]
        y_o, c = self.ref[(i, l)]
        p64 = self.params[l].to(torch.float64)
        g_o = O.backward(gy, x, mask.double(), p64, O.Config(), c)
        rep = []
        if self.dtype == torch.float32:
            checks = [("y", got["y"], y_o)] + [(k, got[k], g_o[k]) for k in GRADS if got[k] is not None]
            rep += [f"{k} {rel_err(a, b):.3e}" for k, a, b in checks if not rel_err(a, b) < TOL]
            rep += [f"{k} element-wise {elem_err(a, b):.3e}" for k, a, b in checks if k in ("y", "gx", "gmask") and not elem_err(a, b) < 1e-3]
        else:
            checks = [("y", got["y"].float(), y_o), ("gx", got["gx"].float(), g_o["gx"]), ("gw1", got["gw1"], g_o["gw1"]),
                      ("gbeta", got["gbeta"], g_o["gbeta"])] + ([("gmask", got["gmask"], g_o["gmask"])] if got["gmask"] is not None else [])
            rep += [f"{k} {rel_err(a, b):.3e}" for k, a, b in checks if not rel_err(a, b) < TOL_BF16]
        return [f"call {i} level {l}: {r}" for r in rep]


SINGLE, ALL = [(0, True)], [(0, True), (1, True), (2, True)]


@pytest.mark.parametrize("name,calls,dtype,oracle", [
    # single <-> 3-level pyramid: P3's sweeps regroup (cfg2: cpt 1 <-> 2)
    ("single_pyramid", [SINGLE, ALL, SINGLE, ALL, SINGLE], torch.float32, {(1, 0), (1, 1), (1, 2), (2, 0)}),
    # only P3's mask requires grad (P3 launches alone, P4+P5 together) <-> all masks do (one launch group of three)
    ("gmask_flip", [[(0, True), (1, False), (2, False)], ALL, [(0, True), (1, False), (2, False)], ALL], torch.float32, {(2, 0)}),
    # 2-level pyramid P3+P5 (cpt 1) <-> 3-level pyramid (cpt 2)
    ("two_three", [[(0, True), (2, True)], ALL, [(0, True), (2, True)], ALL], torch.float32, {(2, 0)}),
    ("single_pyramid_bf16", [SINGLE, ALL, SINGLE, ALL], torch.bfloat16, {(1, 0), (2, 0)}),
])
def test_results_do_not_depend_on_call_composition(F, name, calls, dtype, oracle, monkeypatch):
    """The same composition sequence with the merged backward launch and with the separate launches (MGACBAM_BWD_MERGE=0, a fresh
    epoch and so fresh ctxs): every gradient bit for bit; every y equals the level's forward alone; selected calls against the
    fp64 oracle (tied samples' gy zeroed); the hand-off status clear after every call."""
    from mga_yolo_amd import _lib
    seq = _Seq(LEVELS["cfg2"], calls, dtype, oracle)
    merged = seq.run(F)
    report = []
    for i, call in enumerate(calls):
        if len(call) > 1:
            for l, _ in call:
                if not torch.equal(merged[i][l]["y"], seq.per_level_forward(F, i, l)):
                    report.append(f"call {i} level {l}: y differs from the level's forward alone")
    for i, l in sorted(oracle):
        report += seq.oracle_report(i, l, merged[i][l])
    monkeypatch.setenv("MGACBAM_BWD_MERGE", "0")
    _lib.reload_env()
    try:
        split = seq.run(F)
    finally:
        monkeypatch.undo()
        _lib.reload_env()
    for i, call in enumerate(calls):
        for l, _ in call:
            for k in GRADS:
                a, b = merged[i][l][k], split[i][l][k]
                if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
                    d = float((a.double() - b.double()).abs().max()) if a is not None and b is not None else float("nan")
                    report.append(f"call {i} level {l}: {k} merged != split (max |diff| {d:.3e}, rel {d / max(float(b.abs().max()), 1e-30):.3e})")
    assert not report, f"{name}: " + "; ".join(report)


def test_eca_results_do_not_depend_on_call_composition(F):
    """mask_eca <-> mask_eca_pyramid at B = 32 (group_cpt is taken over the call here too; no hand-offs, so nothing is expected to
    drift -- this pins it): every level of every call against the fp64 ECA oracle, fresh inputs per call."""
    shapes = LEVELS["cfg2"]
    params = []
    for l, (B, C, H, W) in enumerate(shapes):
        p = E.EcaParams.default_init(C, seed=60 + l)
        with torch.no_grad():
            p.w.add_(0.3 * torch.randn(p.w.shape, generator=torch.Generator().manual_seed(l)))
        p.beta.fill_(0.4)
        params.append(p)
    report = []
    for i, levels in enumerate([[0], [0, 1, 2], [0], [0, 1, 2], [0]]):
        lv, gys, data = [], [], []
        for l in levels:
            B, C, H, W = shapes[l]
            x, mask, gy = synth(B, C, H, W, seed=1300 + 10 * i + l, mask_kind="mixed")
            data.append((x, mask, gy))
            lv.append((x.cuda().requires_grad_(True), mask.cuda().requires_grad_(True), params[l].w.cuda().requires_grad_(True),
                       params[l].beta.cuda().requires_grad_(True), F.EcaConfig(k=params[l].w.shape[-1])))
            gys.append(gy.cuda())
        ys = (F.mask_eca(*lv[0]),) if len(lv) == 1 else F.mask_eca_pyramid(lv)
        torch.autograd.backward(list(ys), gys)
        for l, (x, mask, gy), (xd, md, w, beta, _), y in zip(levels, data, lv, ys):
            p64 = E.EcaParams(params[l].w.double(), params[l].beta.double())
            y_o, t = E.forward(x.double(), mask.double(), p64)
            g_o = E.backward(gy.double(), x.double(), mask.double(), p64, E.EcaConfig(), t)
            floor = 1e-7 * float(gy.norm() * x.norm())           # gw / gbeta / gmask: long signed sums (tests/fuzz/fuzz_parity.py)
            for k, got, want in (("y", y, y_o), ("gx", xd.grad, g_o["gx"]), ("gmask", md.grad, g_o["gmask"]), ("gw", w.grad, g_o["gw"]),
                                 ("gbeta", beta.grad, g_o["gbeta"])):
                d = float((got.detach().double().cpu() - want).abs().max())
                bar = TOL * float(want.abs().max()) + (floor if k not in ("y", "gx") else 0.0)
                if not d <= bar:
                    report.append(f"call {i} level {l}: {k} |diff| {d:.3e} > {bar:.3e}")
        del ys, lv
    assert not report, "; ".join(report)
