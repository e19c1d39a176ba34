"""CPU side of the loss-side rows (tests/test_gpu_loss_rows.py runs the same tables on the device).
1. the fp64 resampler and the fp64 `forward` of oracle/segloss_oracle.py, pinned against F.interpolate and the reference's goldens;
2. a Python mirror of the loops of csrc/segloss.cuh / gater.cuh / resize.cuh (constants read from the sources) asserts that every row of
   the tables reaches the branch it is there for -- second outer trip, ragged batch, empty parts, second wave trip, grid-stride trip;
3. what fp32 itself costs on every ladder row (the module's host path against the same ops in fp64), with a factor 3 to spare under the
   element-wise bar the device rows use;
4. the conditions on the inputs that make fp32 and fp64 comparable at the decisions (t > 0.5, soft > threshold)."""
import pytest
import torch
import torch.nn.functional as F

from conftest import elem_err
from oracle import loss_rows as R
from oracle import maskcbam_oracle as MO
from oracle import segloss_oracle as O
from test_segloss import _check_against_golden, load_seg_golden, seg_golden_names

K = R.constants()
ELEM_BAR = 1e-3          # the element-wise gradient bar of the device rows (conftest.elem_err, floor 1e-3 of the tensor's maximum)


def _coord_bound(tsize, size):
    """fp32 against fp64 bilinear on targets in [0, 1]: the source coordinate in/out * (d + 0.5) - 0.5 is formed in fp32 from a rounded
    ratio, a rounded product and a rounded difference, each within half an ulp of a value below max(Ht, Wt) -- three half-ulps at
    2^-24 relative each; a weight error moves the result by at most that much per axis.  1e-6 for the lerps themselves."""
    return 1e-6 + 2 * 3 * max(tsize) * 2.0 ** -24


# ---- 1. the fp64 oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", seg_golden_names())
def test_resampler_matches_interpolate_on_the_goldens_targets(name):
    d = load_seg_golden(name)
    seen = 0
    for i, k in enumerate(("p3", "p4", "p5")):
        if k not in d["preds"] or i >= len(d["targets"]):
            continue
        x, t = d["preds"][k], d["targets"][i]
        seen += 1
        t4 = t if t.dim() == 4 else t.unsqueeze(1)
        size = tuple(x.shape[-2:])
        near = O.resample64(t4, *size, False)
        assert torch.equal(near, F.interpolate(t4.float(), size=size, mode="nearest").double())
        bil = O.resample64(t4, *size, True)
        want = F.interpolate(t4.float(), size=size, mode="bilinear", align_corners=False).double()
        assert float((bil - want).abs().max()) <= _coord_bound(t4.shape[-2:], size)
    assert seen


@pytest.mark.parametrize("row", R.TARGET_TABLE + R.UFL_BILINEAR, ids=lambda r: r[0])
@pytest.mark.parametrize("soft", [False, True], ids=["binary", "soft"])
def test_resampler_matches_interpolate_on_the_size_table(row, soft):
    name, B, size, tsize = row
    t = R.targets_for(B, tsize, soft, R.row_seed(name, soft))
    near = O.resample64(t, *size, False)
    assert torch.equal(near, F.interpolate(t, size=size, mode="nearest").double())
    assert torch.equal(near, MO.nearest_resize(t, *size).double())
    d = R.d_row(t, size)
    print(f"d_row {name} {'soft' if soft else 'binary'}: {d:.2e} (bound {_coord_bound(tsize, size):.2e})")
    assert d <= _coord_bound(tsize, size)
    if tsize == size:
        assert torch.equal(O.resample64(t, *size, True), t.double())


@pytest.mark.parametrize("name", seg_golden_names())
def test_fp64_forward_matches_the_reference_golden(name):
    """The bars of test_segloss.test_oracle_matches_the_reference_golden (1e-6 on every value, 1e-6 of the tensor's maximum on the
    gradient): fp64 logits on the goldens' stored fp32 targets -- the loss in double on the targets the reference saw.  (With the
    targets handed over in fp64 as well, `resample64` replaces the reference's fp32 source coordinates; `bilinear_odd`, d_row 1.1e-6,
    then sits 1.76e-6 from its golden's gradient, which is the golden's own rounding: see the test below.)"""
    d = load_seg_golden(name)
    cfg = O.SegLossConfig(**d["meta"]["cfg"])
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in d["preds"].items()}
    total, logs = O.forward(leaf, d["targets"], cfg, bilinear_targets=d["meta"]["prob_mode"])
    assert total.dtype == torch.float64
    total.backward()
    _check_against_golden(d, total.detach(), logs, {k: v.grad for k, v in leaf.items()}, tol_loss=1e-6, tol_grad=1e-6)


@pytest.mark.parametrize("name", [n for n in seg_golden_names() if load_seg_golden(n)["meta"]["prob_mode"]])
def test_fp64_targets_move_the_gradient_by_the_goldens_own_resample_error(name):
    """Whole evaluation in double (fp64 targets -> resample64) against the bilinear goldens.  The BCE gradient (p - t) / N carries a
    target error one to one relative to its maximum, so the distance from the golden is bounded by the level's d_row (what the
    reference's fp32 source coordinate cost, from torch alone) times the weights' share, here at most 2, plus the 1e-6 of the bar above."""
    d = load_seg_golden(name)
    cfg = O.SegLossConfig(**d["meta"]["cfg"])
    leaf = {k: v.double().clone().requires_grad_(True) for k, v in d["preds"].items()}
    total, _ = O.forward(leaf, [t.double() for t in d["targets"]], cfg, bilinear_targets=True)
    total.backward()
    for i, k in enumerate(("p3", "p4", "p5")):
        if k not in leaf:
            continue
        w = d["grads"][k].double()
        dr = R.d_row(d["targets"][i], tuple(w.shape[-2:]))
        rel = float((leaf[k].grad - w).abs().max()) / float(w.abs().max())
        print(f"{name} {k}: d_row {dr:.2e}, fp64 path against the golden's gradient {rel:.2e} of its maximum")
        assert rel <= 1e-6 + 2 * dr


# ---- 2. the mirror: which branch a row reaches ---------------------------------------------------------------------------
def test_constants_are_the_ones_the_tables_were_chosen_for():
    assert (K["parts"], K["block"], K["U"], K["wave"], K["max_levels"]) == (8, 256, 4, 64, 4)
    assert (K["pmg_cap"], K["resize_cap"], K["kendall_max"]) == (2048, 4096, 4096)


@pytest.mark.parametrize("n", sorted(set(R.LADDER_N + [1, 63, 64, 65, 6400, 2500, 12 * 9])))
def test_partial_loop_visits_every_position_once(n):
    assert R.seg_partial_map(n, K)["cover_once"]


def test_ladder_rows_reach_their_branches():
    slot, stride = K["parts"] * K["block"], K["U"] * K["parts"] * K["block"]
    want = {                                      # n: (outer trips, live slots, empty parts, ragged batch)
        255: (1, [0], 7, True), 256: (1, [0], 7, True), 257: (1, [0], 6, True),          # one part not full / exactly full / one position into part 1
        2047: (1, [0], 0, True), 2048: (1, [0], 0, True), 2049: (1, [0, 1], 0, True),    # slot 0 not full / full / first position of slot 1
        8191: (1, [0, 1, 2, 3], 0, True), 8192: (1, [0, 1, 2, 3], 0, False),             # last slot one short / every batch full
        8193: (2, [0, 1, 2, 3], 0, True),                                                 # SECOND OUTER TRIP, one position in it
        16385: (3, [0, 1, 2, 3], 0, True), 25600: (4, [0, 1, 2, 3], 0, True),            # config 5's 160 x 160
        24581: (4, [0, 1, 2, 3], 0, True),                                                # 3 x 8192 + 5
    }
    assert (slot, stride) == (2048, 8192)
    for n, shape in R.ladder_rows():
        assert shape[0] * shape[1] == n
        m = R.seg_partial_map(n, K)
        print(f"ladder {n:6d} as {shape}: {R.describe(n)}")
        assert (m["outer_trips"], m["live_slots"], m["empty_parts"], m["ragged_batch"]) == want[n], (n, m)
        assert m["bwd_trips"] == -(-n // slot)
    assert any(h > 2048 and w == 1 for _, (h, w) in R.ladder_rows())              # one column with H*W > 2048
    # what the suite reached before: the largest level was 80 x 80, the fuzzer stayed at 40 x 40
    assert R.seg_partial_map(6400, K)["outer_trips"] == 1 and R.seg_partial_map(1600, K)["live_slots"] == [0]
    assert R.seg_partial_map(1600, K)["empty_parts"] == 1


def test_target_table_reaches_its_branches():
    rows = {r[0]: r for r in R.TARGET_TABLE}
    for name, B, (H, W), (Ht, Wt) in R.TARGET_TABLE:
        print(f"target row {name}: level {H}x{W} <- {Ht}x{Wt}, B={B}: {R.describe(H * W)}")
    trips = lambda n: R.seg_partial_map(rows[n][2][0] * rows[n][2][1], K)["outer_trips"]
    assert trips("cfg5_160_from_1280") == 4 and trips("identity_160") == 4 and trips("three_trips_47x523") == 4
    assert rows["identity_160"][2] == rows["identity_160"][3]
    _, _, (H, W), _ = rows["one_column_2500"]
    assert W == 1 and H > K["parts"] * K["block"]
    for n in ("rows_equal_20_from_20x33", "cols_equal_20_from_33x20"):
        (H, W), (Ht, Wt) = rows[n][2], rows[n][3]
        assert (H == Ht) != (W == Wt)
    assert rows["from_one_pixel"][3] == (1, 1) and rows["to_one_pixel"][2] == (1, 1)
    (H, W), (Ht, Wt) = rows["up_40_from_13x9"][2:]
    assert H > Ht and W > Wt
    for n in ("odd_91_from_640", "odd_45x37_from_100x64"):
        (H, W), (Ht, Wt) = rows[n][2:]
        assert Ht % H and Wt % W


def test_batch_kendall_and_grid_rows_reach_their_trips():
    assert [R.seg_final_trips(b, K) for b in R.BATCH_LADDER] == [1, 1, 1, 2, 3]
    assert [R.kendall_trips(n, K) for n in R.KENDALL_N] == [(1, 1), (1, 1), (1, 1), (1, 2), (2, 5), (16, 64)]
    assert max(R.KENDALL_N) == K["kendall_max"]
    for name, shape in R.GATER_BIG:
        n = 1
        for s in shape:
            n *= s
        t = R.grid_stride_trips(n, K["pmg_cap"], K)
        print(f"gater row {name}: n={n}, grid-stride trips {t}")
        assert t == 2
    assert R.grid_stride_trips(K["pmg_cap"] * K["block"], K["pmg_cap"], K) == 1
    got = []
    for src, out in R.RESIZE_ROWS:
        n = src[0] * src[1] * out[0] * out[1]
        got.append(R.grid_stride_trips(n, K["resize_cap"], K))
        print(f"resize row {src} -> {out}: {n} outputs, grid-stride trips {got[-1]}")
    assert got == [7, 2, 1, 1]
    assert R.grid_stride_trips(2 * 80 * 80, K["resize_cap"], K) == 1                # the largest row tested before


# ---- 3. what fp32 itself costs --------------------------------------------------------------------------------------------
def ladder_case(n, shape, B=2, scale=2.0):
    """The ladder level rides as p3 next to a small p4: the second level's workgroups start where the ladder level's end, so the
    level lookup (`start[]`) is exercised at every size."""
    seed = R.row_seed("ladder", n, shape, B)
    preds = {"p3": R.logits_for(B, shape, seed, scale), "p4": R.logits_for(B, (5, 7), seed + 1, scale)}
    tg = [R.targets_for(B, shape, False, seed), R.targets_for(B, (5, 7), False, seed + 1)]
    return preds, tg


LADDER_KW = dict(scale_weights=(1.0, 0.5, 2.0), loss_lambda=0.7, bce_weight=0.9, dice_weight=1.1, smooth=1.0, ufl_lambda=0.4)


def _host_vs_fp64(preds, tg, ufl):
    from mga_yolo_amd.segloss import SegLossConfig, SegmentationLoss
    kw = dict(LADDER_KW, use_unified_focal=ufl)
    p32 = {k: v.clone().requires_grad_(True) for k, v in preds.items()}
    p64 = {k: v.double().requires_grad_(True) for k, v in preds.items()}
    t32, _ = SegmentationLoss(SegLossConfig(**kw))(p32, tg)
    t64, _ = O.forward(p64, [t.double() for t in tg], O.SegLossConfig(**kw))
    t32.backward(); t64.backward()
    return max(elem_err(p32[k].grad, p64[k].grad) for k in preds)


@pytest.mark.parametrize("ufl", [False, True], ids=["plain", "ufl"])
def test_fp32_host_path_leaves_a_factor_three_under_the_bar_on_every_ladder_row(ufl):
    worst = 0.0
    for n, shape in R.ladder_rows():
        e = _host_vs_fp64(*ladder_case(n, shape), ufl)
        print(f"ladder {n} as {shape} {'ufl' if ufl else 'plain'}: fp32 host vs fp64 elem_err {e:.2e}")
        assert e <= ELEM_BAR / 3, (n, shape, e)
        worst = max(worst, e)
    for B in R.BATCH_LADDER:
        e = _host_vs_fp64(*ladder_case(35, (5, 7), B=B), ufl)
        print(f"batch {B} {'ufl' if ufl else 'plain'}: fp32 host vs fp64 elem_err {e:.2e}")
        assert e <= ELEM_BAR / 3, (B, e)


@pytest.mark.parametrize("row", R.TARGET_TABLE, ids=lambda r: r[0])
def test_target_recovery_works_on_the_host_path(row):
    """The method of part 2 on the CPU: the BCE gradient gives back every element of the resampled target."""
    from mga_yolo_amd.segloss import SegLossConfig, SegmentationLoss
    name, B, size, tsize = row
    for bilinear in (False, True):
        t = R.targets_for(B, tsize, True, R.row_seed(name, True))
        x = R.logits_for(B, size, R.row_seed(name), scale=1.0).requires_grad_(True)
        mp = pytest.MonkeyPatch()
        try:
            mp.setenv("MGA_PROB_MODE", "1") if bilinear else mp.delenv("MGA_PROB_MODE", raising=False)
            total, _ = SegmentationLoss(SegLossConfig(dice_weight=0.0))({"p3": x}, [t])
        finally:
            mp.undo()
        total.backward()
        got = R.recover_target(x.detach(), x.grad, B, size[0] * size[1])
        err = float((got - O.resample64(t, *size, bilinear)).abs().max())
        assert err <= 1e-6 + (4 * R.d_row(t, size) if bilinear else 0.0), (name, bilinear, err)


# ---- 4. conditions on the inputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.UFL_BILINEAR, ids=lambda r: r[0])
def test_ufl_bilinear_targets_stay_clear_of_one_half(row):
    B, size, tsize, _, t = R.ufl_bilinear_inputs(row[0])
    d = R.d_row(t, size)
    r = O.resample64(t, *size, True)
    gap = float((r - 0.5).abs().min())
    print(f"{row[0]}: d_row {d:.2e}, margin {R.ufl_margin(d):.2e}, closest pixel to 0.5 at {gap:.2e}")
    assert gap >= R.ufl_margin(d)
    assert float(t.min()) >= 0.0 and float(t.max()) <= 1.0
    assert 0.3 < float((r > 0.5).double().mean()) < 0.7            # both sides of the decision are populated


def test_binary_targets_at_a_power_of_two_ratio_sit_exactly_on_one_half():
    """160 <- 1280: the source coordinate is 8 d + 3.5, weights 1/2 exactly, values k/4: fp32 and fp64 agree bit for bit, and
    thousands of pixels are exactly 0.5 -- the row that tells `t > 0.5` from `t >= 0.5`."""
    t = R.targets_for(1, (1280, 1280), False, R.row_seed("half_exact"))
    r64 = O.resample64(t, 160, 160, True)
    r32 = F.interpolate(t, size=(160, 160), mode="bilinear", align_corners=False)
    assert torch.equal(r32.double(), r64)
    n_half = int((r64 == 0.5).sum())
    print(f"pixels exactly 0.5: {n_half} of {r64.numel()}")
    assert n_half > 1000
    assert set(r64.unique().tolist()) <= {0.0, 0.25, 0.5, 0.75, 1.0}


@pytest.mark.parametrize("p_min", [0.0, 0.15])
def test_gater_gates_are_the_ones_torch_autograd_applies(p_min):
    """The analytic gate mask of R.gater_host64 against autograd of the module's host math in fp32, at a tau and uniforms where the
    sigmoid cannot saturate (|z| < 6): there a zero gradient is a closed gate and nothing else."""
    p, _, _ = R.gater_edge_grid(p_min)
    u = torch.full_like(p, 0.5)
    x = p.clone().requires_grad_(True)
    q = x.clamp(0.0, 1.0)
    if p_min > 0:
        q = q.clamp_min(p_min)
    qq = q.clamp(1e-6, 1.0 - 1e-6)
    noise = torch.log(-torch.log(u)) - torch.log(-torch.log(u))
    torch.sigmoid((torch.log(qq) - torch.log1p(-qq) + noise) / 2.5).sum().backward()
    ref = R.gater_host64(p, u, u, 2.5, p_min, 0.5, False, torch.ones_like(p))
    assert torch.equal(x.grad == 0, ~ref["gate_open"]) and torch.equal(ref["grad"] == 0, ~ref["gate_open"])
    assert 0 < int(ref["gate_open"].sum()) < p.numel()


@pytest.mark.parametrize("row", R.GATER_BIG, ids=lambda r: r[0])
@pytest.mark.parametrize("p_min,tau", [(0.0, 0.3), (0.15, 2.5)])
def test_gater_big_rows_have_few_decisions_near_the_threshold(row, p_min, tau):
    p, u1, u2, _ = R.gater_big_inputs(row[1], R.row_seed(row[0]))
    ref = R.gater_host64(p, u1, u2, tau, p_min, 0.5, True)
    near = int(((ref["soft"] - 0.5).abs() < 1e-6).sum())
    print(f"{row[0]} tau={tau} p_min={p_min}: {near} of {p.numel()} within 1e-6 of the threshold")
    assert near * 10000 <= p.numel()
