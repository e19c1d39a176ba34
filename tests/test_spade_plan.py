"""CPU-side checks of tests/spade_plan.py: the mirror of the MaskSPADE host plan against the built library's size query, every case
row against the paths it declares, the table's coverage as a whole, and the seed rule of the rows (no GPU anywhere)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spade_oracle as SO  # noqa: E402
import spade_plan as P  # noqa: E402
from test_gpu_spade import KEYS, live_case  # noqa: E402

IDS = [P.case_id(c) for c in P.CASES]


def test_mirror_reproduces_the_hand_computed_sizes():
    assert P.scratch_bytes(2, 16, 8, 8, 16) == 43520 and P.scratch_bytes(1, 64, 20, 20, 64) == 1503296      # tests/test_abi_spade.py
    assert P.tiling(8, 8)[:2] == (16, 8) and P.tiling(20, 20)[:2] == (32, 4)
    assert P.split_k(2, 16, 1).nchunk == 2 and P.split_k(1, 64, 5).nchunk == 5


def test_scratch_size_equals_the_library_at_every_small_shape(built_lib):
    """The scratch size is the one place the C ABI shows the plan: it has one term in nchunk and one in the tile count, so equality
    over the sweep pins both (and with them the tiling rule) to the library."""
    from mga_yolo_amd import _lib
    fn = _lib.load().mgaspade_scratch_bytes
    bad, n = [], 0
    for C in (16, 48, 256, 1024):
        for hidden in (16, 48, 64):
            for B in (1, 3):
                for H in range(1, 71):
                    for W in range(1, 71):
                        n += 1
                        got, want = P.scratch_bytes(B, C, H, W, hidden), fn(B, C, H, W, hidden)
                        if got != want and len(bad) < 10:
                            bad.append(((B, C, H, W, hidden), got, want))
    assert n == 70 * 70 * 4 * 3 * 2 and not bad, bad


def test_the_sweep_itself_reaches_every_tiling_and_both_split_k_regimes():
    seen_tw, seen_tpc = set(), set()
    for H in range(1, 71):
        for W in range(1, 71):
            t = P.tiling(H, W)
            assert t.TW * t.TH == P.PX and t.tiles == t.tiles_x * t.tiles_y and t.tiles_x * t.TW >= W and t.tiles_y * t.TH >= H
            for other in (5, 4, 3, 2):                         # no tiling has fewer tiles; among equals the widest was kept
                n = P.cdiv(W, 1 << other) * P.cdiv(H, P.PX >> other)
                assert n > t.tiles or (n == t.tiles and other <= t.ltw)
            seen_tw.add(t.TW)
            for C in (16, 1024):
                k = P.split_k(3, C, t.tiles)
                assert (k.nchunk - 1) * k.tpc < 3 * t.tiles <= k.nchunk * k.tpc and 1 <= k.last_len <= k.tpc
                seen_tpc.add(min(k.tpc, 2))
    assert seen_tw == {4, 8, 16, 32} and seen_tpc == {1, 2}


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_every_row_takes_the_paths_it_declares(c):
    got = P.plan_of(c)
    want = {k: getattr(c, k) for k in got}
    assert got == want, {k: (want[k], got[k]) for k in got if got[k] != want[k]}
    assert c.C % 16 == 0 and c.C <= 1024 and c.hidden % 16 == 0 and c.hidden <= 64          # inside the kernels' limits
    assert c.B * c.H * c.W <= 2000                                                          # a few launches over a small grid


def test_the_table_covers_every_tiling_width_and_split():
    shapes = [(c.B, c.C, c.H, c.W) for c in P.CASES]
    assert len(set(shapes)) == len(shapes)
    for tw in (32, 16, 8, 4):
        assert any(c.tw == tw and min(c.tiles) >= 2 and c.ragged == (True, True) for c in P.CASES), f"TW = {tw}: no ragged multi-tile row"
        assert any(c.tw == tw and c.tiles == (1, 1) for c in P.CASES), f"TW = {tw}: no single-tile row"
    assert {c.hidden for c in P.CASES} == {16, 32, 48, 64}
    assert {c.norm for c in P.CASES} == {"in", "bn"}
    assert any(c.fwd[1] >= 2 and c.fwd[2] < c.fwd[0] for c in P.CASES)                      # a last channel block smaller than cblk
    assert any(c.tpc >= 2 and c.crosses and c.last_len < c.tpc for c in P.CASES)
    assert any(c.C == 1024 and c.fwd[1] == 16 and c.dh[0] == 32 and c.nchunk == 8 for c in P.CASES)
    assert any(c.c16 and c.dh[0] >= 2 for c in P.CASES)                                     # a last k_spade_dh round of 16 channels
    assert {c.tw for c in P.CASES if c.hidden == 48} == {4, 8, 32}
    assert any(c.H == 1 for c in P.CASES) and any(c.W == 1 for c in P.CASES)
    assert any((c.H * c.W) % 4 == 0 and c.H * c.W <= 4 for c in P.CASES) and any((c.H * c.W) % 4 for c in P.CASES)
    assert any(c.eps != 1e-6 and c.momentum != 0.1 and c.norm == "bn" for c in P.CASES)


def test_locate_names_the_tile_and_the_place_in_it():
    assert P.locate(60, 10, 0, 0) == ((0, 0), (0, 0))
    assert P.locate(60, 10, 33, 9) == ((1, 2), (1, 1))                                      # 4 x 32 tiles
    assert P.locate(30, 22, 29, 16) == ((1, 2), (13, 0))                                    # 8 x 16 tiles
    assert P.locate(7, 60, 6, 59) == ((1, 1), (2, 27))                                      # 32 x 4 tiles


@pytest.mark.parametrize("c", P.CASES, ids=IDS)
def test_no_row_has_a_pre_activation_at_the_relu_edge(c):
    """The generator's rule: with min |pre| >= 1e-5 in fp64 no ReLU branch can differ on the device, so the plain bars hold unwidened."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    m, x, mask, gy = live_case(c.B, c.C, c.H, c.W, c.norm, seed=c.seed, hidden=c.hidden)
    params = {k: v.detach() for k, v in m.state_dict().items() if k in KEYS}
    runs = (m.norm.running_mean.clone(), m.norm.running_var.clone()) if c.norm == "bn" else None
    _, ctx = SO.forward(x, mask, params, c.norm, True, True, c.eps, runs, c.momentum)
    lo = SO.min_abs_pre(ctx)
    print(f"{P.case_id(c)} seed {c.seed}: min |pre| {lo:.3e}")
    assert lo >= 1e-5
