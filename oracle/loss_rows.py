"""TEST INFRASTRUCTURE -- the tables behind the loss-side rows (tests/test_loss_rows_tables.py on the CPU, tests/test_gpu_loss_rows.py on
the device): which sizes are run, a Python mirror of the loop arithmetic of csrc/segloss.cuh, csrc/gater.cuh and csrc/resize.cuh that
says which branch of those loops a size reaches, the seeded inputs, and fp64 references (gater host math, recovered targets).
The kernels' constants are READ from the sources by regex: a retune changes what the mirror computes, and the CPU test that asserts
"this row reaches a second outer trip" then fails instead of silently testing nothing.  Only tests/ may import this."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from . import segloss_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mga_yolo_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _int(pattern, text, what):
    m = re.search(pattern, text)
    assert m, f"constant not found: {what}"
    return int(m.group(1))


def constants():
    seg, common, eca, api_seg = _src("segloss.cuh"), _src("common.cuh"), _src("api_eca.hip"), _src("api_seg.hip")
    k = dict(
        block=_int(r"constexpr int kBlock = (\d+);", common, "kBlock"),
        wave=_int(r"constexpr int kWave = (\d+);", common, "kWave"),
        parts=_int(r"constexpr int kSegParts = (\d+);", seg, "kSegParts"),
        max_levels=_int(r"constexpr int kSegMaxLevels = (\d+);", seg, "kSegMaxLevels"),
        U=_int(r"constexpr int U = (\d+);", seg, "U of k_seg_partial"),
        pmg_cap=_int(r"pmg_grid\(size_t n\).*?g > (\d+) \?", eca, "pmg grid cap"),
        resize_cap=_int(r"if \(grid > (\d+)\) grid = \d+;", eca, "resize grid cap"),
        kendall_max=_int(r"n_det > (\d+)\)", api_seg, "kendall n_det limit"),
    )
    # the loop forms the mirror below restates
    assert "i0 < HW; i0 += U * kSegParts * kBlock" in seg and "const int i = i0 + u * kSegParts * kBlock;" in seg
    assert "i < HW; i += kSegParts * kBlock" in seg and "b < L.B; b += kWave" in seg
    assert "i < A.kd.n; i += kBlock" in seg and "i < A.kd.n; i += kWave" in seg
    assert re.search(r"kSegEps = 1e-6f", seg) and re.search(r"kGateEps = 1e-6f", _src("gater.cuh"))
    return k


# ---------------------------------------------------------------------------------------------------------------------------
# mirror of the loops
# ---------------------------------------------------------------------------------------------------------------------------
def seg_partial_map(HW, k=None):
    """k_seg_partial over one sample: every (part, thread, outer trip, slot u) -> position, exactly as the kernel forms it.
    -> dict(cover_once, outer_trips, live_slots, empty_parts, ragged_batch, bwd_trips)."""
    k = k or constants()
    parts, block, U = k["parts"], k["block"], k["U"]
    slot, stride = parts * block, U * parts * block
    seen = np.zeros(HW, dtype=np.int64)
    part_load = np.zeros(parts, dtype=np.int64)
    live = set()
    ragged, trips = False, 0
    i0 = np.arange(slot)                                   # part * kBlock + threadIdx.x
    while (i0 < HW).any():
        trips += 1
        act = i0 < HW
        alive = []
        for u in range(U):
            i = i0 + u * slot
            ok = act & (i < HW)
            np.add.at(seen, i[ok], 1)
            np.add.at(part_load, (np.arange(slot) // block)[ok], 1)
            if ok.any():
                live.add(u)
            alive.append(ok)
        # a thread whose batch holds both a live and a dead slot: the `if (i < HW)` inside the batch decides
        ragged |= bool((alive[0] & ~alive[U - 1]).any())
        i0 = i0 + stride
    return dict(cover_once=bool((seen == 1).all()), outer_trips=trips, live_slots=sorted(live),
                empty_parts=int((part_load == 0).sum()), ragged_batch=ragged, bwd_trips=-(-HW // slot),
                partial_wave=HW % k["wave"] != 0)


def seg_final_trips(B, k=None):
    return -(-B // (k or constants())["wave"])


def kendall_trips(n, k=None):
    """(trips of the workgroup loop in k_seg_final's epilogue, trips of the lane loop in k_seg_bwd's prologue)."""
    k = k or constants()
    return -(-n // k["block"]), -(-n // k["wave"])


def grid_stride_trips(n, cap, k=None):
    k = k or constants()
    grid = min(-(-n // k["block"]), cap)
    return -(-n // (grid * k["block"]))


def describe(HW):
    m = seg_partial_map(HW)
    return (f"outer trips {m['outer_trips']}, live slots {m['live_slots']}, empty parts {m['empty_parts']}, "
            f"ragged batch {'yes' if m['ragged_batch'] else 'no'}, bwd trips {m['bwd_trips']}")


# ---------------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------------
# part 2: (name, B, (H, W) of the level, (Ht, Wt) of the target)
TARGET_TABLE = [
    ("cfg5_160_from_1280", 2, (160, 160), (1280, 1280)),
    ("cfg2_80_from_640", 2, (80, 80), (640, 640)),
    ("identity_160", 2, (160, 160), (160, 160)),            # identity branch at H*W > 8192
    ("odd_91_from_640", 2, (91, 91), (640, 640)),
    ("odd_45x37_from_100x64", 3, (45, 37), (100, 64)),
    ("up_40_from_13x9", 2, (40, 40), (13, 9)),
    ("rows_equal_20_from_20x33", 2, (20, 20), (20, 33)),
    ("cols_equal_20_from_33x20", 2, (20, 20), (33, 20)),
    ("from_one_pixel", 2, (12, 9), (1, 1)),
    ("to_one_pixel", 3, (1, 1), (37, 29)),
    ("one_column_2500", 2, (2500, 1), (700, 3)),            # W = 1 with H*W > 2048
    ("three_trips_47x523", 2, (47, 523), (100, 300)),       # 3 * 8192 + 5 pixels, non-square target
    ("pow2_17x23_from_68x92", 2, (17, 23), (68, 92)),
]
assert 47 * 523 == 3 * 8192 + 5

LADDER_N = [255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 16385, 25600, 24581]
BATCH_LADDER = [1, 63, 64, 65, 130]
KENDALL_N = [1, 3, 64, 65, 257, 4096]
# Unified Focal with bilinear soft targets (part 4): (name, B, level, target)
UFL_BILINEAR = [
    ("ufl_17x23_from_68x92", 2, (17, 23), (68, 92)),
    ("ufl_45x37_from_100x64", 2, (45, 37), (100, 64)),
    ("ufl_20_from_20x33", 2, (20, 20), (20, 33)),
    ("ufl_160_from_1280", 1, (160, 160), (1280, 1280)),
]


def near_square(n):
    """(h, w) with h * w == n and h <= w as close as the factors allow; a prime gives (n, 1): one column."""
    h = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return (h, n // h) if h > 1 else (n, 1)


def ladder_rows():
    rows = []
    for n in LADDER_N:
        rows.append((n, (1, n)))
        rows.append((n, near_square(n)))
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def row_seed(*key):
    s = 0
    for v in key:
        for ch in str(v):
            s = (s * 131 + ord(ch)) % 1000003
    return s


def targets_for(B, tsize, soft, seed, dim3=False):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, 1, *tsize, generator=g)
    t = r if soft else (r > 0.7).float()
    return t.squeeze(1) if dim3 else t


def logits_for(B, size, seed, scale=2.0):
    return torch.randn(B, 1, *size, generator=torch.Generator().manual_seed(seed + 77)) * scale


def d_row(t, size):
    """max |F.interpolate (fp32, bilinear) - fp64 resampler| of a row: what fp32 rounding of the source coordinate costs there."""
    t4 = t if t.dim() == 4 else t.unsqueeze(1)
    if tuple(t4.shape[-2:]) == tuple(size):
        return 0.0
    f32 = F.interpolate(t4.float(), size=size, mode="bilinear", align_corners=False)
    return float((f32.double() - SO.resample64(t4, *size, True)).abs().max())


def recover_target(logits, grad, B, HW, gout=1.0):
    """With dice_weight = 0, bce_weight = 1, plain mode: g_i = gout (p_i - t_i) / (B HW)  =>  t_i = sigmoid(x_i) - g_i B HW / gout."""
    return torch.sigmoid(logits.double()) - grad.double() * (float(B) * float(HW) / gout)


def soft_targets_clear_of_half(B, tsize, size, seed, margin):
    """Uniform soft targets whose fp64 bilinear resample has no pixel within `margin` of 0.5 (Unified Focal decides t > 0.5 per pixel;
    fp32 and fp64 may only be compared where they cannot decide differently).  Offending pixels get their upper-left tap nudged."""
    t = targets_for(B, tsize, True, seed)
    y0, _, _ = SO.resample_index64(size[0], tsize[0], True)
    x0, _, _ = SO.resample_index64(size[1], tsize[1], True)
    for _ in range(200):
        r = SO.resample64(t, *size, True)
        bad = ((r - 0.5).abs() < margin).nonzero()
        if bad.numel() == 0:
            return t
        for b, _, y, x in bad.tolist():
            v = t[b, 0, y0[y], x0[x]]
            t[b, 0, y0[y], x0[x]] = v + 0.03 if v < 0.9 else v - 0.03
    raise AssertionError("could not clear the 0.5 band")


def ufl_margin(d):
    return 10.0 * (1e-6 + 4.0 * d)


def ufl_bilinear_inputs(name):
    _, B, size, tsize = next(r for r in UFL_BILINEAR if r[0] == name)
    seed = row_seed(name)
    # the margin depends on d_row, which depends on the targets: two passes (d_row moves by rounding noise only)
    t = targets_for(B, tsize, True, seed)
    t = soft_targets_clear_of_half(B, tsize, size, seed, 1.5 * ufl_margin(d_row(t, size)))
    return B, size, tsize, logits_for(B, size, seed), t


# ---------------------------------------------------------------------------------------------------------------------------
# ProbMaskGater: the edge grid and the host math in fp64
# ---------------------------------------------------------------------------------------------------------------------------
def _f32(v):
    return np.float32(v)


def gater_edge_grid(p_min):
    """Every p edge against every (u1, u2) edge: three fp32 tensors of shape (1, 1, n_p, 36)."""
    up, dn = lambda v: np.nextafter(_f32(v), _f32(np.inf)), lambda v: np.nextafter(_f32(v), _f32(-np.inf))
    hi = _f32(1.0) - _f32(1e-6)                      # the upper clamp bound as an fp32 program forms it
    assert hi == _f32(1.0 - 1e-6)                    # ... which is also the double 1 - 1e-6 rounded to fp32 (torch's scalar path)
    pm = _f32(p_min)
    ps = [_f32(-1e-3), _f32(-0.0), _f32(0.0), _f32(1e-7), _f32(1e-6), up(1e-6), dn(1e-6), pm, up(pm), dn(pm), _f32(0.5), hi, up(hi), dn(hi),
          _f32(1.0), up(1.0), _f32(1.4)]
    us = [_f32(0.0), _f32(1e-7), _f32(1e-6), _f32(0.5), hi, _f32(1.0)]
    p = torch.from_numpy(np.array(ps, dtype=np.float32))[:, None].expand(len(ps), 36).contiguous()
    u1 = torch.from_numpy(np.array(us, dtype=np.float32)).repeat_interleave(6)[None, :].expand(len(ps), 36).contiguous()
    u2 = torch.from_numpy(np.array(us, dtype=np.float32)).repeat(6)[None, :].expand(len(ps), 36).contiguous()
    sh = (1, 1, len(ps), 36)
    return p.reshape(sh), u1.reshape(sh), u2.reshape(sh)


def gater_host64(p, u1, u2, tau, p_min, threshold, hard, gout=None):
    """ProbMaskGater's host path (module.py: clamp, clamp_min, logistic noise, sigmoid, straight-through) on fp32 inputs, every op in
    fp64.  The parameters are the values an fp32 program holds: eps = fp32(1e-6), 1 - eps = fp32(1 - 1e-6), fp32(p_min), fp32(tau) --
    fp32(1 - 1e-6) is 1 - 1.0133e-6, and a logit formed at 1 - 1e-6 instead differs by 0.013.
    -> dict(out, soft, grad (None without gout), gate_open)."""
    lo, hi = float(_f32(1e-6)), float(_f32(1.0) - _f32(1e-6))
    pm, tau = float(_f32(p_min)), float(_f32(tau))
    x = p.double().clone().requires_grad_(True)
    q = x.clamp(0.0, 1.0)
    if p_min > 0:
        q = q.clamp_min(pm)
    noise = torch.log(-torch.log(u2.double().clamp(lo, hi))) - torch.log(-torch.log(u1.double().clamp(lo, hi)))
    qq = q.clamp(lo, hi)
    soft = torch.sigmoid((torch.log(qq) - torch.log1p(-qq) + noise) / tau)
    out = (soft > float(_f32(threshold))).double() + (soft - soft.detach()) if hard else soft
    grad = None
    if gout is not None:
        out.backward(gout.double())
        grad = x.grad
    # the clamps' gates, as exact comparisons on the fp32 inputs (torch passes the gradient at a bound, bounds included)
    pd = p.double()
    qd = pd.clamp(0.0, 1.0)
    gate = (pd >= 0.0) & (pd <= 1.0)
    if p_min > 0:
        gate &= qd >= pm
        qd = qd.clamp_min(pm)
    gate &= (qd >= lo) & (qd <= hi)
    return dict(out=out.detach(), soft=soft.detach(), grad=grad, gate_open=gate)


def gater_big_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g) * 1.8 - 0.4
    return p, torch.rand(shape, generator=g), torch.rand(shape, generator=g), torch.randn(shape, generator=g)


GATER_BIG = [("b32_160x160", (32, 1, 160, 160)), ("one_past_the_grid", (1, 1, 1, 524288 + 1))]
RESIZE_ROWS = [((4, 1, 640, 640), (1280, 1280)), ((2, 1, 1280, 1280), (900, 700)), ((2, 1, 33, 47), (33, 47)), ((3, 1, 1, 1), (7, 5))]
