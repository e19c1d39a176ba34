"""Replay t of a long-lived, captured plan == a fresh plan given the same state, bit for bit (tests/plan_replays.py: run_row).

Every other test that replays a plan replays it on the same inputs and parameters, where anything a replay wrongly takes from the step before is
bit-identical to what it should have computed.  Here every one of the K = 4 replays of a row sees inputs that are new in size and content
(x, gy scaled by 0.5 + 0.5 t) and parameters that moved in place by 5 % of their scale along the last step's gradients, without a
re-capture; before each replay a fresh plan with new zero-filled ctx / scratch / ws / sync state is built from clones of the long-lived
plan's state, run once eagerly on the same inputs, and every output, the whole gradient bucket, every running buffer and the gate's state
are compared with torch.equal.  The kernels are fixed-order, so bit equality is the bar; a mismatch at step t >= 1 that
is absent at t = 0 is state that crossed a replay.  All mismatches of a row go into one report (step, level, name, max |diff|, differing
elements) asserted once, so a failure shows its pattern: tile-shaped = a hand-off, one level = a level table, equal to step t - 1 = a launch
that did not write.

Each row asserts about itself: the NCHW MaskCBAM rows that k_gate and the folded backward really run (a use_proj forward is k_chan + k_apply by
design, k_gate saves no projection planes: fold only), every parameter moved by >= 1e-3 of its max-norm, no output equals its value of the
step before, the gate's state is [seed, s0 + t + 1, 0, 0], every num_batches_tracked is n0 + t + 1, and the two plans share no storage.

The fp32 SlicePlan rows end with an anchor outside the plans: the module composition on the last step's inputs, with the parameters and
running buffers of the state before that step, at the bars of test_slice_plan_equals_the_module_composition."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_replays as R  # noqa: E402
import test_gpu_static_plans as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NCHW2 = [(4, 64, 40, 40), (4, 128, 20, 20)]       # test_fold_counters_survive_a_half_finished_backward's shapes: fold_active (and gate_active)
P345 = S.SHAPES                                    # [(4,64,16,16), (4,128,8,8), (4,256,4,4)]
GUMBEL = ("gumbel", 0.5, 0.2, 0.5)                 # mode, tau, p_min, threshold
HARD_ST = ("hard_st", 0.5, 0.05, 0.5)
SLICE_GUMBEL = ("gumbel", 0.5, 0.05, 0.5)          # test_gated_slice_plan_equals_the_module_composition's gate
SPADE_SHAPES = [(c.B, c.C, c.H, c.W) for c in S.ROWS]
MASK_HW = [(10, 6), None, (16, 12)]


def _lay(cl):
    return "channels_last" if cl else "nchw"


ROWS = [
    # 1. PyramidPlan, NCHW: k_gate's hand-off flags, the folded / merged backward's generation counters, scratch partial sums
    R.row("cbam-nchw-fp32", "cbam", NCHW2),
    R.row("cbam-nchw-bf16", "cbam", NCHW2, dtype=BF16),
    R.row("cbam-nchw-fp32-use_proj", "cbam", NCHW2, use_proj=True),                 # the projection planes parked in ctx
    R.row("cbam-nchw-fp32-gumbel", "cbam", NCHW2, gate=GUMBEL),                     # msoft, {seed, step}
    R.row("cbam-nchw-fp32-split", "cbam", NCHW2, split=True),                       # forward(); backward_params(); backward_inputs()
    # 2. PyramidPlan.create(channels_last=True): the pooling partials ws
    R.row("cbam-channels_last-fp32", "cbam", P345, cl=True),
    R.row("cbam-channels_last-fp32-hard_st", "cbam", P345, cl=True, gate=HARD_ST),
    # 3. EcaPyramidPlan
    R.row("eca-nchw-fp32", "eca", P345),
    R.row("eca-channels_last-fp32", "eca", P345, cl=True),
]
# 4. SpadePyramidPlan: gamma kept in ctx, the weight pack as a launch of the forward, running statistics, the resample; channels_last: the
#    batch-norm level parks four wave sums per channel in the ctx weight-pack area
ROWS += [R.row(f"spade-{_lay(cl)}-{n}", "spade", SPADE_SHAPES, cases=S.ROWS, mask_hw=MASK_HW, cl=cl, dtype=dt)
         for cl in (False, True) for n, dt in (("fp32", F32), ("fp16", F16))]
# 5. SlicePlan.create: head_ctx / head_scratch, head_params as MFMA operands, seg_ws, log_vars, the heads' running statistics
_P, _B = S.SLICE_ROWS
ROWS += [R.row(f"slice-p3p4p5-{b}-{_lay(cl)}", "slice", _P[0], block=b, cl=cl, hidden=_P[1], target_hw=_P[2], resize=_P[3])
         for b, cl in S.COMBOS + [("cbam", False)]]
ROWS += [R.row(f"slice-two-levels-bilinear-{b}-{_lay(cl)}", "slice", _B[0], block=b, cl=cl, hidden=_B[1], target_hw=_B[2], resize=_B[3])
         for b, cl in [("spade", True), ("cbam", False)]]
ROWS += [R.row(f"slice-p3p4p5-cbam-{_lay(cl)}-gumbel", "slice", _P[0], block="cbam", cl=cl, hidden=_P[1], target_hw=_P[2], resize=_P[3],
               gate=SLICE_GUMBEL) for cl in (False, True)]


@pytest.mark.parametrize("index", range(len(ROWS)), ids=[r.id for r in ROWS])
def test_replays_equal_a_fresh_plan_on_the_same_state(built_lib, index):
    r = ROWS[index]
    report, stale, misses = R.run_row(r, index, anchor=r.kind == "slice" and r.dtype == F32)
    assert not report and not stale and not misses, dict(mismatches=report, unchanged_since_the_step_before=stale, anchor=misses)
