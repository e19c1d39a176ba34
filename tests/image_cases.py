"""The cases of the image batch (include/ext/mgaimage.h, mga_yolo_amd/image.py), each with what it is built for, and their seeded sources.
tests/test_image_oracle.py, tests/test_gpu_image.py and tools/gen_golden_image.py all read this table."""
import os
from collections import namedtuple

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20261021

# ---- no resize: (name, (B,C,H,W), what it is built for).  Sizes are set against the kernel's constants: a lane takes 4 elements, the flat
# form 4096 elements a workgroup, the tile form 1024 pixels a workgroup.
Plain = namedtuple("Plain", "name shape why")
PLAIN = [
    Plain("ramp256", (1, 1, 16, 16), "all 256 byte values, once each: the quotient's bits in the three types"),
    Plain("one_px", (2, 3, 1, 1), "a plane of one pixel: nothing but the element path, runs shorter than a vector"),
    Plain("row17", (1, 3, 1, 17), "H*W = 17: planar runs that start at every alignment, a one-element tail"),
    Plain("odd5x3", (2, 3, 5, 3), "H*W = 15, 90 elements: sample and channel bases off every vector boundary"),
    Plain("c4_7x15", (2, 4, 7, 15), "four channels (the interleaved pixel is one 4-byte load), H*W = 105"),
    Plain("c1_3x67", (1, 1, 3, 67), "one channel: every layout and the reversal are the flat stream; 201 elements, one ragged tail"),
    Plain("sq16", (2, 3, 16, 16), "H*W a multiple of the vector: the vector path alone"),
    Plain("wide70x130", (2, 3, 70, 130), "9100 pixels a sample: nine tiles of the tile form, the last ragged (908 pixels); 54600 elements: 14 "
                                        "workgroups of the flat form, the last ragged; H*W not a multiple of 16"),
]
PLAIN_BY_NAME = {c.name: c for c in PLAIN}

# ---- resize: (name, B, C, in_hw, out_hw, what it is built for).  A tile is up to 64 rows x 1024 columns and about 2048 pixels.
Resize = namedtuple("Resize", "name B C in_hw out_hw why")
MULTI_SCALE = dict(imgsz=64, stride=32, shape=(2, 3, 40, 56), seeds={0: (64, 64), 1: (32, 32), 5: (96, 96)})    # what the reference picks
RESIZE = [
    Resize("ms64", 2, 3, (40, 56), (64, 64), "the reference's multi_scale pick of seed 0; two tiles of 32 rows"),
    Resize("ms32", 2, 3, (40, 56), (32, 32), "its pick of seed 1: a downscale, one tile"),
    Resize("ms96", 2, 3, (40, 56), (96, 96), "its pick of seed 5: five tiles of 21 rows, the last ragged"),
    Resize("from1x1", 2, 3, (1, 1), (5, 7), "a one-pixel source: both taps of both axes are that pixel"),
    Resize("col7", 2, 1, (7, 1), (3, 9), "a source one pixel wide, one channel"),
    Resize("down_odd", 2, 4, (37, 53), (19, 27), "odd sizes both ways, four channels, a run that is no multiple of the vector"),
    Resize("up_3x5", 2, 3, (3, 5), (64, 96), "a 20-fold upscale: long runs of equal taps, three tiles of 21 rows and a ragged one"),
    Resize("half70x130", 2, 3, (70, 130), (35, 65), "exactly 2:1: every coordinate lands on .5, lam = 0.5"),
    Resize("seams70x130", 2, 3, (70, 130), (105, 195), "eleven tiles of 10 rows of 195 pixels (the last of 5): ten seams, runs that are no multiple of the vector"),
    Resize("strip", 2, 1, (6, 700), (6, 1400), "wider than a tile: column strips of 1024 and 376 pixels in tiles of two rows, one run per row"),
]
RESIZE_BY_NAME = {c.name: c for c in RESIZE}
IDENTITY = Resize("same33x17", 2, 3, (33, 17), (33, 17), "size equal to the source's: must be the no-resize result, bit for bit")


def source(shape, seed=SEED, ramp=False):
    """uint8 (B,C,H,W), a function of the shape and the seed alone.  The top-left quarter (rounded up) of sample 0 is black, and in a batch of
    more than one sample so is the whole of its channel 0, so that a resize of however small a source has destinations whose whole footprint -- the taps and the neighbours a
    coordinate one ulp away would reach -- is 0.  ramp: the 256 values in order instead (shape (1,1,16,16))."""
    if ramp:
        return torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)
    B, Cc, H, W = shape
    rs = np.random.RandomState((seed + 7919 * B + 104729 * Cc + 1299709 * H + 15485863 * W) % (2 ** 31))
    v = rs.randint(0, 256, size=shape).astype(np.uint8)
    v[0, :, :(H + 1) // 2, :(W + 1) // 2] = 0
    if B > 1:
        v[0, 0] = 0
    return torch.from_numpy(v)


def plain_source(c: Plain):
    return source(c.shape, ramp=c.name == "ramp256")


def resize_source(c: Resize):
    return source((c.B, c.C) + tuple(c.in_hw))


def path(name):
    return os.path.join(GOLDEN, f"image_{name}.npz")


RATIOS = os.path.join(GOLDEN, "image_ratios.json")
SIZES_SEEDS = 32                  # image_sizes.npz: the reference's output shapes over seeds 0 .. 31
SIZES_HW = [(40, 56), (48, 64)]   # (48, 64): the draw 64 gives sf == 1 -- no resize
