"""What the target-pyramid tests share (tests/test_targets_host.py, tests/test_gpu_targets.py, tests/test_gpu_slice_targets.py).  Not a test.

The stored results (tests/golden/targets_*.npz, written by tools/gen_golden_targets.py) are the reference's own MaskUtils on the masks stored
beside them.  `compose` is the second oracle: torch's avg_pool2d / max_pool2d of the binarised, zero-padded mask -- an implementation of the
same definition that shares nothing with mask_pyramid's CPU path (block sums of integers).  Both hold integer counts scaled by a power of
two, so every comparison against either is torch.equal."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN

SHAPES = [(1, 8, 8), (1, 7, 5), (2, 64, 64), (2, 72, 136), (2, 100, 76), (3, 33, 95), (1, 544, 544)]
PATTERNS = ("zero", "one", "sparse", "dense", "corner", "f32vals", "u8vals")
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
