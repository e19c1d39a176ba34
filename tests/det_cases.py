"""Cases of the detection criterion past the sizes of the six stored ones (tests/golden/det_*.npz): boxes over more than one kDetChunk of
cells, more than kBlock label rows, more than kBlock partials, 1 / 2 / 4 levels, topk 1 and 16 (include/mgadet.h, csrc/det.cuh).

Their features are too large to store, so they are rebuilt here from a seed: numpy.random.RandomState (a frozen stream) and arithmetic
only, the "trained-like" recipe of tools/gen_golden_det.make_inputs -- background 0.5 n with the classes at -3; inside a box the bin logits
of a side -(j - t)^2 / 1.5 + 0.3 n around the true distance t moved by up to a cell, and the label's class logit 1.5 + n -- rounded once to
fp32.  tests/golden/detx_<name>.npz (tools/gen_golden_det.py --shapes) records the seed the generator accepted, the SHA-256 of the features,
the labels, and what the reference's own criterion gave on exactly these values; load() refuses features whose digest differs.

Per-row options (the 7th entry of a row, a dict):
  collapsed  share of the box's anchors, drawn per anchor, whose four sides peak sharply at bin 0: a predicted box of almost no size,
             CIoU <= 0 against a box tens of cells wide, overlap and metric exactly 0
  mute       levels on which the row's anchors are taken out of the race for its top-k, except at
  boost      cells (y, x) of level 0, whose class logit is set to BOOST: the top-k then comes from these cells, wherever they lie in the
             kernel's visiting order
  how        "class" (default): a muted anchor's class logit is MUTE, its metric some 1e-9 of what it was.  sigmoid(MUTE) and the class
             gradient that comes of it, some 1e-18, lie far below fp16's smallest subnormal, so no case with this option runs in fp16.
             "box": a muted anchor's sides peak at bin 0 like a collapsed one's, overlap and metric exactly 0, every value in fp16's range
"""
import hashlib
import json
import math
import os

import numpy as np
import torch

import det_oracle as O

GAINS = (7.5, 0.5, 1.5)
UPSTREAM = (0.7, -1.3, 2.1)
MUTE, BOOST = -40.0, 6.0
CHUNK, BLOCK = 2048, 256                       # kDetChunk, kBlock of csrc/det.cuh


def _crowd_rows():
    """300 rows over three images of 128^2, interleaved: 298 boxes 6 to 14 px on a side, the all-zero row, a box without an anchor centre."""
    rs = np.random.RandomState(7)
    rows = []
    for i in range(298):
        w, h = rs.uniform(6.0, 14.0, 2)
        x1, y1 = rs.uniform(0.0, 128.0 - w), rs.uniform(0.0, 128.0 - h)
        rows.append((i % 3, int(rs.randint(0, 3)), round(float(x1), 2), round(float(y1), 2), round(float(x1 + w), 2), round(float(y1 + h), 2)))
    rows.append((2, 0, 0.0, 0.0, 0.0, 0.0))
    rows.append((1, 1, 17.1, 17.2, 19.7, 19.5))
    return [rows[i] for i in rs.permutation(len(rows))]


_B2_64 = [(0, 2, 5.2, 7.3, 38.6, 44.9), (0, 1, 30.5, 20.2, 60.9, 45.1), (1, 0, 20.3, 18.6, 43.8, 33.1), (1, 2, 2.7, 40.2, 61.4, 62.9),
          (1, 1, 10.4, 5.7, 52.6, 30.3)]
# every anchor of the oversized boxes is muted on every level, the boosted cells apart: they alone can win (at stride 8 a side reaches
# 15 cells at the most, so the best level-0 overlap with a box 53 cells wide is some 0.3, far below a coarse cell's)
_ALL = (0, 1, 2)
CASES = {
    # image 0: a box over all 3024 cells whose winners are the boosted cells, six in chunk 0 (level-0 rows < 40) and six in chunk 1
    # (rows >= 44), and an ordinary box over it; image 1: a box just inside the image, left alone (its winners are coarse cells)
    "chunk2": dict(B=2, hw=(384, 384), nc=2, strides=(8, 16, 32), topk=10, rows=[
        (0, 0, -20.5, -18.2, 404.7, 402.3, dict(mute=_ALL, how="box", boost=[(6, 40), (12, 8), (20, 44), (27, 5), (33, 41), (38, 12),
                                                                   (44, 30), (45, 6), (45, 42), (46, 18), (47, 36), (47, 2)])),
        (0, 1, 150.3, 120.6, 300.9, 260.2),
        (1, 1, 6.3, 5.1, 378.4, 379.2)]),
    # 576 wide x 512 high, 6048 cells, three chunks: level-0 rows < 28, 29 .. 56 and >= 57 (with levels 1 and 2)
    "chunk3": dict(B=1, hw=(512, 576), nc=1, strides=(8, 16, 32), topk=10, rows=[
        (0, 0, -14.5, -22.2, 590.7, 530.3, dict(mute=_ALL, boost=[(5, 10), (14, 60), (22, 33), (26, 5), (31, 50), (38, 20), (45, 64),
                                                                   (54, 36), (58, 12), (59, 58), (61, 30), (62, 44)]))]),
    # all but a handful of the anchors predict a box of no size: fewer than topk positive metrics, the rest of the picks are zeros
    "chunk_zero": dict(B=1, hw=(384, 384), nc=1, strides=(8, 16, 32), topk=10, rows=[
        (0, 0, -20.5, -18.2, 404.7, 402.3, dict(collapsed=0.998))]),
    # B * A = 66 528: 260 workgroups of partials.  Labels in three images only
    "wide": dict(B=22, hw=(384, 384), nc=1, strides=(8, 16, 32), topk=10, rows=[
        (0, 0, 40.3, 60.2, 200.7, 310.4), (0, 0, 180.9, 30.6, 360.2, 170.3), (13, 0, -30.5, -12.2, 420.7, 400.3),
        (13, 0, 100.4, 90.7, 250.6, 280.3), (21, 0, 12.4, 200.3, 160.8, 370.6), (21, 0, 220.3, 210.6, 330.8, 300.1),
        (21, 0, 60.9, 20.2, 140.1, 110.7)]),
    "crowd": dict(B=3, hw=(128, 128), nc=3, strides=(8, 16, 32), topk=10, rows=_crowd_rows()),
    "lv1": dict(B=2, hw=(64, 64), nc=3, strides=(8,), topk=10, rows=_B2_64),
    "lv2": dict(B=2, hw=(64, 64), nc=3, strides=(8, 16), topk=10, rows=_B2_64),
    "lv4": dict(B=2, hw=(96, 128), nc=2, strides=(4, 8, 16, 32), topk=10, rows=[
        (0, 0, 10.3, 12.2, 20.7, 25.4), (0, 1, 30.9, 8.6, 118.2, 90.3), (0, 0, 60.4, 40.7, 100.6, 80.3),
        (1, 1, 70.4, 10.3, 82.8, 24.6), (1, 0, 4.3, 30.6, 90.8, 88.1, dict(mute=(0, 1), how="box"))]),     # the last box's winners: strides 16 and 32
    "topk1": dict(B=2, hw=(64, 64), nc=3, strides=(8, 16, 32), topk=1, rows=_B2_64),
    "topk16": dict(B=2, hw=(128, 128), nc=2, strides=(8, 16, 32), topk=16, rows=[
        (0, 1, 12.3, 20.4, 44.6, 60.7), (0, 0, 2.3, 1.6, 126.4, 125.2), (1, 0, 40.6, 30.3, 100.2, 110.8), (1, 1, 8.9, 70.4, 50.3, 120.6),
        (1, 0, 60.2, 8.3, 120.7, 50.9)]),
}
HALF_CASES = ("chunk2", "crowd", "lv4", "topk16")


def shapes(name):
    c = CASES[name]
    return [(c["hw"][0] // s, c["hw"][1] // s) for s in c["strides"]]


def anchors(name):
    return sum(h * w for h, w in shapes(name))


def labels(name):
    """The case's rows in the batch's form: batch_idx (n), cls (n), bboxes (n, 4) normalised xywh, fp32."""
    c = CASES[name]
    H, W = c["hw"]
    r = np.array([row[:6] for row in c["rows"]], dtype=np.float64).reshape(-1, 6)
    xywh = np.stack(((r[:, 2] + r[:, 4]) / 2 / W, (r[:, 3] + r[:, 5]) / 2 / H, (r[:, 4] - r[:, 2]) / W, (r[:, 5] - r[:, 3]) / H), 1)
    return tuple(torch.from_numpy(a.astype(np.float32)) for a in (r[:, 0], r[:, 1], xywh))


def build_feats(name, seed):
    """The case's feature maps (B, 64 + nc, H_l, W_l), fp32, from RandomState(seed)."""
    c = CASES[name]
    rs = np.random.RandomState(seed)
    B, nc = c["B"], c["nc"]
    j = np.arange(16, dtype=np.float64)
    feats = []
    for l, (s, (h, w)) in enumerate(zip(c["strides"], shapes(name))):
        f = 0.5 * rs.standard_normal((B, 64 + nc, h, w))
        f[:, 64:] -= 3.0
        py, px = np.meshgrid((np.arange(h) + 0.5) * s, (np.arange(w) + 0.5) * s, indexing="ij")
        for row in c["rows"]:
            b, k, x1, y1, x2, y2 = row[:6]
            opt = row[6] if len(row) > 6 else {}
            if x2 <= x1:
                continue
            ys, xs = np.nonzero((x1 < px) & (px < x2) & (y1 < py) & (py < y2))
            m = ys.size
            t = np.stack((px[ys, xs] - x1, py[ys, xs] - y1, x2 - px[ys, xs], y2 - py[ys, xs]), 1) / s
            t = np.clip(t + (rs.random_sample((m, 4)) * 2 - 1), 0.0, 15.0)
            bins = -(j[None, None] - t[:, :, None]) * (j[None, None] - t[:, :, None]) / 1.5 + 0.3 * rs.standard_normal((m, 4, 16))
            logit = 1.5 + rs.standard_normal(m)
            if "collapsed" in opt:
                gone = rs.random_sample(m) < opt["collapsed"]
                bins[gone] = -4.0 * j * j
            if l in opt.get("mute", ()):
                quiet = np.ones(m, dtype=bool)
                if l == 0:
                    for y, x in opt.get("boost", ()):
                        quiet[(ys == y) & (xs == x)] = False
                if opt.get("how", "class") == "box":
                    bins[quiet] = -4.0 * j * j
                else:
                    logit[quiet] = MUTE
                logit[~quiet] = BOOST
            f[b, :64, ys, xs] = bins.reshape(m, 64)
            f[b, 64 + k, ys, xs] = logit
        feats.append(torch.from_numpy(f.astype(np.float32)))
    return feats


def digest(feats):
    d = hashlib.sha256()
    for f in feats:
        d.update(np.ascontiguousarray(f.numpy(), dtype="<f4").tobytes())
    return d.hexdigest()


def path(name):
    return os.path.join(O.GOLDEN, f"detx_{name}.npz")


def load(name):
    """The record of tests/golden/detx_<name>.npz with the features rebuilt from its seed; fails if they are not the recorded ones."""
    z = np.load(path(name))
    c = {k: z[k] for k in z.files}
    spec = CASES[name]
    feats = build_feats(name, int(c["seed"]))
    assert digest(feats) == str(c["sha256"]), f"{name}: the rebuilt features are not the ones the record was made from"
    lab = labels(name)
    for got, key in zip(lab, ("batch_idx", "cls", "bboxes")):
        assert np.array_equal(got.numpy(), c[key]), f"{name}: {key} differs from the record"
    assert tuple(c["strides"]) == tuple(spec["strides"]) and int(c["topk"]) == spec["topk"] and json.loads(str(c["options"])) == options(name)
    B, A, nc = spec["B"], anchors(name), spec["nc"]
    ts = np.zeros(B * A * nc, dtype=np.float64)
    ts[c["ts_index"]] = c["ts_value"]
    fg = np.zeros(B * A, dtype=bool)
    fg[c["fg_index"]] = True
    c.update(name=name, B=B, nc=nc, feats=feats, labels=lab, target_scores_f64=ts.reshape(B, A, nc), fg_mask_f64=fg.reshape(B, A),
             upstream=np.array(UPSTREAM), kw=dict(nc=nc, strides=tuple(spec["strides"]), gains=tuple(float(g) for g in c["gains"]), topk=spec["topk"]))
    return c


def options(name):
    """The rows' builder options in the form the record keeps (JSON: lists for tuples)."""
    return json.loads(json.dumps({str(i): r[6] for i, r in enumerate(CASES[name]["rows"]) if len(r) > 6}))


# the existing K, or twice the reference's own fp32-against-fp64 ratio over these cases where that is larger
K = {}
_RATIOS = os.path.join(O.GOLDEN, "det_ratios_shapes.json")
if os.path.exists(_RATIOS) and O.K:                            # absent only while the generator writes it
    with open(_RATIOS) as _f:
        _W = json.load(_f)["worst"]
    K = dict(loss=max(O.K["loss"], 2 * _W["loss"]), target_scores=max(O.K["target_scores"], 2 * _W["target_scores"]),
             grad=max(O.K["grad"], 2 * max(_W["g1"], _W["gnu"])))


# ---- the kernel's visiting order ---------------------------------------------------------------------------------------------------------
def visit_order(name, row):
    """k_det_assign's order of the cells of label row `row`: level after level, each level's clipped rectangle (one cell of margin) row-major.
    Returns the anchor index of every visited cell; a cell's position in it is its cell index, position // CHUNK its chunk."""
    c = CASES[name]
    f = np.float32
    bb = labels(name)[2].numpy()[row]
    img_w, img_h = f(c["hw"][1]), f(c["hw"][0])
    cx, cy, hw_, hh = bb[0] * img_w, bb[1] * img_h, bb[2] * img_w * f(0.5), bb[3] * img_h * f(0.5)
    x1, y1, x2, y2 = cx - hw_, cy - hh, cx + hw_, cy + hh
    out, a0 = [], 0
    for s, (H, W) in zip(c["strides"], shapes(name)):
        s = f(s)
        ix0 = int(min(max(math.floor(x1 / s - f(0.5)) - 1, 0), W - 1)); iy0 = int(min(max(math.floor(y1 / s - f(0.5)) - 1, 0), H - 1))
        ix1 = int(max(min(math.ceil(x2 / s - f(0.5)) + 1, W - 1), 0)); iy1 = int(max(min(math.ceil(y2 / s - f(0.5)) + 1, H - 1), 0))
        for y in range(iy0, iy1 + 1):
            out.extend(a0 + y * W + x for x in range(ix0, ix1 + 1))
        a0 += H * W
    return np.array(out, dtype=np.int64)


def built_for(name, o):
    """What the case was built to hold, from the oracle's result `o` (with its `picks`) and the kernel's visiting order.  Returns the
    reasons it does not (empty: it does) -- the generator re-seeds on them, tests/test_det_cases.py asserts there are none."""
    c = CASES[name]
    why = []
    bidx = labels(name)[0].numpy()

    def picked_cells(row):
        b = int(bidx[row])
        rows, pos, met = o["picks"][b]
        g = rows.index(row)
        order = visit_order(name, row)
        where = {int(a): i for i, a in enumerate(order)}
        sel = torch.nonzero(pos[g]).flatten().tolist()
        return order, np.array([where[a] for a in sel]), met[g][sel].numpy(), np.array(sel)

    if name in ("chunk2", "chunk3"):
        nchunk = 2 if name == "chunk2" else 3
        order, cells, _, _ = picked_cells(0)
        if not order.size > CHUNK * (nchunk - 1):
            why.append(f"T_ = {order.size}")
        if set((cells // CHUNK).tolist()) != set(range(nchunk)):
            why.append(f"picks in chunks {sorted(set((cells // CHUNK).tolist()))}")
    if name == "chunk_zero":
        order, cells, met, sel = picked_cells(0)
        rows, pos, allmet = o["picks"][0]
        npos = int((allmet[0] > 0).sum())
        if not 0 < npos < c["topk"]:
            why.append(f"{npos} positive metrics")
        if not (cells[met > 0] >= CHUNK).any():
            why.append("no positive pick past the first chunk")
        zeros = np.sort(sel[met == 0])
        if zeros.size != c["topk"] - npos or not np.array_equal(zeros, np.arange(zeros.size)):   # every anchor is inside this box
            why.append(f"zero picks {zeros.tolist()}")
        if not float(o["weight"].sum()) > 0:
            why.append("no positive weight")
    if name == "wide":
        if not -(-c["B"] * anchors(name) // BLOCK) > BLOCK:
            why.append("nblk <= 256")
    if name == "crowd":
        counts = np.bincount(bidx.astype(np.int64), minlength=c["B"])
        contested = sum(int((pos.sum(0) > 1).sum()) for rows, pos, met in o["picks"].values())
        if not (bidx.size > BLOCK and counts.min() > 64 and counts.max() <= 256):
            why.append(f"rows per image {counts.tolist()}")
        if not (np.diff(bidx) < 0).any():
            why.append("rows sorted by image")
        if contested < 50:
            why.append(f"{contested} contested anchors")
    if name in HALF_CASES:
        # a class channel's gradient term is its own magnitude: below 2^-15 half of fp16's subnormal spacing (2^-25) exceeds eps_fp16 * terms
        # and the element type's range, not the kernel, would decide the fp16 run
        for l in range(len(c["strides"])):
            t = O.grad_terms(o["terms"], l, UPSTREAM)[:, 64:]
            if bool((t > 0).any()) and float(t[t > 0].min()) < 2.0 ** -15:
                why.append(f"a class gradient term of {float(t[t > 0].min()):.1e} on level {l}: below fp16's range")
    if name == "lv4":
        a0 = np.cumsum([0] + [h * w for h, w in shapes(name)])
        fg = (o["fg"] & (o["weight"] > 0)).any(0).numpy()
        if not all(fg[a0[l]:a0[l + 1]].any() for l in range(4)):
            why.append("a level without a foreground anchor")
    return why
