"""What the target-pyramid tests share (tests/test_targets_host.py, tests/test_gpu_targets.py, tests/test_gpu_targets_edges.py,
tests/test_gpu_slice_targets.py).  Not a test.

The stored results (tests/golden/targets_*.npz, written by tools/gen_golden_targets.py) are the reference's own MaskUtils on the masks stored
beside them.  `compose` is the second oracle: torch's avg_pool2d / max_pool2d of the binarised, zero-padded mask -- an implementation of the
same definition that shares nothing with mask_pyramid's CPU path (block sums of integers).  Both hold integer counts scaled by a power of
two, so every comparison against either is torch.equal.

For the edges (EDGE_SHAPES, EDGE_PATTERNS): guarded_outs / guarded_src put NaN sentinels around the destinations and foreign foreground
around the source; close3_loops and seam_masks state the closing a second and a third time, as loops and in closed form."""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

SHAPES = [(1, 8, 8), (1, 7, 5), (2, 64, 64), (2, 72, 136), (2, 100, 76), (3, 33, 95), (1, 544, 544)]
PATTERNS = ("zero", "one", "sparse", "dense", "corner", "f32vals", "u8vals")
# the edge fixtures (tools/gen_golden_targets.py: EDGE_SHAPES, EDGE_PATTERNS), every stride 2 .. 64 stored:
#   (2, 36, 72)   W % 8 == 0, H % 8 == 4: wide loads for both element types, a half cell at the bottom, two wave tiles across
#   (3, 61, 128)  odd H, W exactly two tiles; 6 waves: the second workgroup has two live waves
#   (5, 40, 64)   one tile per sample, 5 waves: one live wave in the last workgroup
#   (2, 70, 136)  W % 8 == 0, H % 8 == 6; levels of 35 x 68 .. 3 x 5 cells: the closing's tiles seam at 16 and 32
EDGE_SHAPES = [(2, 36, 72), (3, 61, 128), (5, 40, 64), (2, 70, 136)]
EDGE_PATTERNS = PATTERNS + ("u8all", "f32special", "ramp", "lastrow")
F32_PATTERNS = ("f32vals", "f32special")
KEY_BYTES = (0x00, 0x01, 0x7F, 0x80, 0x81, 0xFE, 0xFF)          # what tgt_nonzero_bytes' carry trick turns on; u8all holds each at every byte position
ALL_STRIDES = (2, 4, 8, 16, 32, 64)
METHODS = ("avgpool", "maxpool")
MODEL_STRIDES = (8, 16, 32)


def shape_id(shape):
    return "%dx%dx%d" % tuple(shape)


@functools.lru_cache(maxsize=None)
def load(shape):
    """-> (meta, {key: tensor}) of one stored shape; loaded once per session and shared: the tests never write into these tensors"""
    z = np.load(os.path.join(GOLDEN, f"targets_{shape_id(shape)}.npz"), allow_pickle=False)
    meta = json.loads(bytes(z["meta"]).decode())
    return meta, {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}


def compose(mask, strides, method, bridge=False):
    """(B,H,W) uint8 | fp32 -> per stride (B,1,ceil(H/s),ceil(W/s)) fp32: binarise with > 0, zero-pad bottom and right, pool; bridge: the
    closing as -max_pool2d(-max_pool2d(m, 3, 1, 1), 3, 1, 1), whose -inf padding ignores what lies outside."""
    B, H, W = mask.shape
    m = (mask > 0).to(torch.float32).unsqueeze(1)
    out = []
    for s in strides:
        p = F.pad(m, (0, -W % s, 0, -H % s))
        lvl = F.avg_pool2d(p, s) if method == "avgpool" else F.max_pool2d(p, s)
        if bridge:
            lvl = -F.max_pool2d(-F.max_pool2d(lvl, 3, 1, 1), 3, 1, 1)
        out.append(lvl)
    return out


def diagonal_mask(shape, step=8):
    """Sparse diagonal lines: one foreground pixel per `step` x `step` cell, on the cell diagonal of every third cell column -- after the max
    pool at stride 8 the lines are 8-connected only, which is what a 3 x 3 closing fills in."""
    B, H, W = shape
    m = torch.zeros(shape, dtype=torch.uint8)
    for b in range(B):
        for cy in range(-(-H // step)):
            for off in (0, 3, 6):
                cx = (cy + off + b) % max(-(-W // step), 1)
                y, x = min(cy * step + 1, H - 1), min(cx * step + 2, W - 1)
                m[b, y, x] = 1
    return m


def guarded_outs(shapes, device, guard=64):
    """-> (views, check): the levels as views into ONE flat fp32 buffer of NaN, `guard` (+ 0 or 1) sentinel floats before, between and
    after them, every level at an odd float offset -- 4-byte aligned and no more, which is all the C ABI asks of a destination.  A cell
    that is never written stays NaN and equals no expected value; check() asserts that every sentinel is still NaN."""
    assert guard >= 64
    offs, off = [], guard
    for shp in shapes:
        off += 1 - off % 2
        offs.append(off)
        off += math.prod(shp) + guard
    buf = torch.full((off,), float("nan"), dtype=torch.float32, device=device)
    views = [buf[o:o + math.prod(shp)].view(shp) for o, shp in zip(offs, shapes)]
    sentinel = torch.ones(off, dtype=torch.bool, device=device)
    for o, shp in zip(offs, shapes):
        sentinel[o:o + math.prod(shp)] = False
    assert all(v.data_ptr() % 8 == 4 and v.is_contiguous() for v in views) and int(sentinel.sum()) >= guard * (len(shapes) + 1)

    def check():
        bad = (~torch.isnan(buf)) & sentinel
        assert not bool(bad.any()), ("written outside the levels, at floats", bad.nonzero().flatten()[:8].tolist(), "levels at", offs)

    return views, check


def guarded_src(mask, device, align):
    """The (B,H,W) mask as a contiguous view inside a larger buffer of foreground (255 | 7.0): a lead in front, at least 7 rows behind,
    so that a read before the first or past the last sample stays inside the buffer and counts.  align=16: the view starts on a 16-byte
    boundary (the wide loads); anything else: off it -- uint8 at % 8 == 3, fp32 at % 16 == 4 (the element loads)."""
    B, H, W = mask.shape
    n = mask.numel()
    u8 = mask.dtype == torch.uint8
    assert u8 or mask.dtype == torch.float32
    lead = (16 if u8 else 4) if align == 16 else (19 if u8 else 5)
    buf = torch.full((lead + n + 7 * W + 16,), 255 if u8 else 7.0, dtype=mask.dtype, device=device)
    view = buf[lead:lead + n].view(B, H, W)
    view.copy_(mask)
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0
    if align == 16:
        assert view.data_ptr() % 16 == 0
    else:
        assert view.data_ptr() % 8 == 3 if u8 else view.data_ptr() % 16 == 4
    return view


def close3_loops(level):
    """The 3 x 3 closing of a (B,1,h,w) level as plain loops over the nine neighbours, those outside the level skipped: a cell of the
    dilation is the largest neighbour, a cell of the result the smallest neighbour of the dilation.  Shares nothing with max_pool2d."""
    a = level.numpy()
    B, _, h, w = a.shape

    def sweep(src, pick):
        out = np.empty_like(src)
        for b in range(B):
            for y in range(h):
                for x in range(w):
                    out[b, 0, y, x] = pick(src[b, 0, yy, xx] for yy in (y - 1, y, y + 1) for xx in (x - 1, x, x + 1) if 0 <= yy < h and 0 <= xx < w)
        return out

    return torch.from_numpy(sweep(sweep(a, max), min))


def close1d(points, n):
    """The closing by a window of three of a set of cells on a line of n, outside ignored, in closed form: the dilation covers one cell on
    either side of a cell, the erosion asks nothing of what lies outside -- so a gap of at most two cells between two cells is filled, a
    gap of three is not, and a cell with at most one cell between it and an end of the line reaches that end."""
    pts = sorted(set(points))
    keep = set(pts)
    for a, b in zip(pts, pts[1:]):
        if b - a - 1 <= 2:
            keep.update(range(a, b))
    if pts and pts[0] <= 1:
        keep.update(range(pts[0]))
    if pts and n - 1 - pts[-1] <= 1:
        keep.update(range(pts[-1], n))
    return sorted(keep)


def seam_masks(shape, stride):
    """-> [(name, mask, closed, seam)]: full-resolution uint8 masks whose level at `stride` is known in closed form, before and after the
    closing.  A chosen cell gets one pixel, the last of the cell that lies inside the image.  Every feature is a product rows x cols (or a
    union of two that do not meet), and the closing by a square of a product is the product of the closings on a line (close1d).
    Per seam s in {16, 32} of k_tgt_close3's 16 x 16 tiles that the level has: across it along a row (h), along a column (v) -- cells s-1
    and s+1 (a gap of one: filled), s-2 and s+1 (a gap of two: filled as well, the dilations of the two touch), s-2 and s+2 (a gap of
    three: not filled); the two cells (s-1, s-1) and (s+1, s+1) on the diagonal (d: nothing is filled, the square around (s, s) holds two
    cells no dilation reaches) and the four cells (s+-1, s+-1) (q: the 3 x 3 block between them is filled, (s, s) from all four tiles).
    Then: a cell in each corner; an all-ones level; an all-ones level with one hole on the border.
    seam: a cell the closing fills in, where the case has one."""
    B, H, W = shape
    oh, ow = -(-H // stride), -(-W // stride)
    cases = []

    def add(name, products, seam=None, closed=None):
        mask = torch.zeros(shape, dtype=torch.uint8)
        want = torch.zeros(B, 1, oh, ow)
        for rows, cols in products:
            for cy in rows:
                for cx in cols:
                    mask[:, min(cy * stride + stride - 1, H - 1), min(cx * stride + stride - 1, W - 1)] = 1
            for cy in close1d(rows, oh):
                for cx in close1d(cols, ow):
                    want[:, 0, cy, cx] = 1.0
        cases.append((name, mask, want if closed is None else closed, seam))

    for s in (16, 32):
        for g, (lo, hi) in {1: (s - 1, s + 1), 2: (s - 2, s + 1), 3: (s - 2, s + 2)}.items():
            if hi < ow and oh != 2:
                add(f"h{s}gap{g}", [([oh // 2], [lo, hi])], seam=(oh // 2, s) if g < 3 else None)
            if hi < oh and ow != 2:
                add(f"v{s}gap{g}", [([lo, hi], [ow // 2])], seam=(s, ow // 2) if g < 3 else None)
        if s + 1 < min(oh, ow):
            add(f"d{s}", [([s - 1], [s - 1]), ([s + 1], [s + 1])])
            add(f"q{s}", [([s - 1, s + 1], [s - 1, s + 1])], seam=(s, s))
    add("corners", [([0, oh - 1], [0, ow - 1])])
    ones = torch.ones(B, 1, oh, ow)
    add("ones", [(range(oh), range(ow))], closed=ones)
    if oh * ow > 1:
        hole = [(range(1, oh), range(ow)), ([0], [c for c in range(ow) if c != ow // 2])]
        add("hole", hole, seam=(0, ow // 2), closed=ones)
    return cases


def random_mask(shape, share=0.08, seed=3):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < share).to(torch.uint8)
