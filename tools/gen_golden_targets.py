"""Write tests/golden/targets_*.npz from the REFERENCE's own MaskUtils (data only -- no reference text is copied).

    python tools/gen_golden_targets.py --reference <checkout of the reference project> [--check]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
stand-ins of tools/gen_golden_opt.py (a stand-in ``cv2``, an answered ``torchvision`` version): ``downsample_mask_prob(method="avgpool")`` and
``downsample_mask`` under ``MGA_MASK_METHOD=maxpool`` are numpy only and never reach cv2.  ``MGA_MASK_METHOD=maxpool`` is set in this
process's environment before the reference is imported; the closing (MGA_MASK_BRIDGE) is cv2's and is not recorded.

One file per mask shape.  Per fill pattern p: ``mask.<p>`` (uint8, or fp32 for f32vals) and, per stride s, ``avgpool.<p>.<s>`` and
``maxpool.<p>.<s>`` -- the reference's per-sample results stacked to (B,1,Hs,Ws) fp32, i.e. masks_multi after collate_fn.  The pattern
``u8vals`` holds uint8 values in {0, 1, 255}: the reference does not binarise a uint8 mask (dataset.py:89 does, before the call), so its
results are those of the reference on ``mask > 0``.

A second list, EDGE_SHAPES x EDGE_PATTERNS (mirrored in tests/targets_cases.py), holds the smallest shapes that reach a ragged bottom row
under the wide loads and a last workgroup with one or two live waves, and four more patterns: ``u8all`` (every byte value; given to the
reference as ``mask > 0`` like ``u8vals``), ``f32special`` (NaN, infinities, signed zeros, subnormals, FLT_MIN), ``ramp`` (a known count
per 8 x 8 cell) and ``lastrow`` (foreground in the last row and column only).  Every stride 2 .. 64 is stored for them."""
import argparse
import importlib.metadata as md
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 8, 8), (1, 7, 5), (2, 64, 64), (2, 72, 136), (2, 100, 76), (3, 33, 95), (1, 544, 544)]
PATTERNS = ("zero", "one", "sparse", "dense", "corner", "f32vals", "u8vals")
EDGE_SHAPES = [(2, 36, 72), (3, 61, 128), (5, 40, 64), (2, 70, 136)]
EDGE_PATTERNS = PATTERNS + ("u8all", "f32special", "ramp", "lastrow")
BINARISED = ("u8vals", "u8all")                  # uint8 patterns with values past 1: the reference is given mask > 0
KEY_BYTES = (0x00, 0x01, 0x7F, 0x80, 0x81, 0xFE, 0xFF)
F32_SPECIAL = (np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.17549435e-38, -1.17549435e-38, 1e-38, 0.3, 1.0)
MODEL_STRIDES = (8, 16, 32)
ALL_STRIDES = (2, 4, 8, 16, 32, 64)              # every stride the library takes, for the shapes below LARGE
LARGE = 100000                                   # pixels per sample from which only the model's strides are recorded


def import_reference(ref_root):
    os.environ["MGA_MASK_METHOD"] = "maxpool"
    cv2 = MagicMock(name="cv2")                            # absent from the build image; nothing of it runs on this path
    cv2.__version__, cv2.__spec__ = "4.10.0", None
    sys.modules["cv2"] = cv2
    real = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else real(n)
    sys.path.insert(0, ref_root)
    import mga_yolo  # noqa: F401  (puts the vendored detector on the path)
    from mga_yolo.utils.mask_utils import MaskUtils
    return MaskUtils


def make_mask(pattern, shape, rng):
    B, H, W = shape
    if pattern == "zero":
        return np.zeros(shape, np.uint8)
    if pattern == "one":
        return np.ones(shape, np.uint8)
    if pattern == "sparse":
        return (rng.random(shape) < 0.02).astype(np.uint8)
    if pattern == "dense":
        return (rng.random(shape) < 0.5).astype(np.uint8)
    if pattern == "corner":                                 # one foreground pixel, in the last row and column: inside the padded cells
        m = np.zeros(shape, np.uint8)
        m[:, H - 1, W - 1] = 1
        return m
    if pattern == "f32vals":
        return rng.choice(np.array([-1.0, 0.0, 0.3, 1.0], np.float32), size=shape)
    if pattern == "u8vals":
        return rng.choice(np.array([0, 1, 255], np.uint8), size=shape)
    if pattern == "u8all":
        # half zeros, half random bytes; then, from the start of sample 0, two aligned 8-byte words per key byte k and byte position j: k at
        # j among seven 0x00 and k at j among seven 0xff; and 0 .. 255 once from the start of the last sample
        assert W % 8 == 0 and H * W >= 2 * 8 * 8 * len(KEY_BYTES) and B >= 2
        m = (rng.integers(0, 256, size=shape) * (rng.random(shape) < 0.5)).astype(np.uint8)
        words = np.empty((len(KEY_BYTES), 8, 2, 8), np.uint8)
        words[:, :, 0, :], words[:, :, 1, :] = 0x00, 0xFF
        for i, k in enumerate(KEY_BYTES):
            for j in range(8):
                words[i, j, :, j] = k
        m[0].reshape(-1)[:words.size] = words.reshape(-1)
        m[B - 1].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        return m
    if pattern == "f32special":
        return rng.choice(np.array(F32_SPECIAL, np.float32), size=shape)
    if pattern == "ramp":                                   # cell (cy, cx) of the 8 x 8 grid: its first (cy * 9 + cx * 5) % 65 pixels, row-major
        y, x = np.mgrid[0:H, 0:W]
        m = ((y % 8) * 8 + x % 8 < ((y // 8) * 9 + (x // 8) * 5) % 65).astype(np.uint8)
        return np.broadcast_to(m, shape).copy()
    if pattern == "lastrow":                                # what a read past the image would add is missing from every result
        m = np.zeros(shape, np.uint8)
        m[:, H - 1, :] = 1
        m[:, :, W - 1] = 1
        return m
    raise ValueError(pattern)


def patterns_of(shape):
    return EDGE_PATTERNS if shape in EDGE_SHAPES else PATTERNS


def strides_of(shape):
    return MODEL_STRIDES if shape[1] * shape[2] >= LARGE else ALL_STRIDES


def build(MaskUtils, shape):
    rng = np.random.default_rng(1000 * shape[1] + shape[2])
    arrays = {}
    for p in patterns_of(shape):
        m = make_mask(p, shape, rng)
        arrays[f"mask.{p}"] = m
        given = (m > 0).astype(np.uint8) if p in BINARISED else m
        for s in strides_of(shape):
            avg = np.stack([MaskUtils.downsample_mask_prob(given[b], s, method="avgpool")[None] for b in range(shape[0])])
            mx = np.stack([MaskUtils.downsample_mask(given[b], s)[None] for b in range(shape[0])])
            assert avg.dtype == np.float32 and avg.shape == mx.shape == (shape[0], 1, -(-shape[1] // s), -(-shape[2] // s))
            arrays[f"avgpool.{p}.{s}"] = avg
            arrays[f"maxpool.{p}.{s}"] = mx.astype(np.float32)
    meta = dict(shape=list(shape), patterns=list(patterns_of(shape)), strides=list(strides_of(shape)), numpy=np.__version__)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--check", action="store_true", help="compare with the stored fixtures instead of writing them")
    a = ap.parse_args()
    MaskUtils = import_reference(a.reference)
    for shape in SHAPES + EDGE_SHAPES:
        arrays = build(MaskUtils, shape)
        path = os.path.join(OUT, "targets_%dx%dx%d.npz" % shape)
        if a.check:
            z = np.load(path)
            assert sorted(z.files) == sorted(arrays), shape
            for k in z.files:
                if k != "meta":
                    assert z[k].dtype == arrays[k].dtype and np.array_equal(z[k], arrays[k], equal_nan=z[k].dtype.kind == "f"), (shape, k)
            print(shape, "reproduced")
        else:
            np.savez_compressed(path, **arrays)
            size = os.path.getsize(path)
            assert size <= 1 << 20, (path, size)
            print(shape, size, "bytes,", len(arrays) - 1, "arrays")


if __name__ == "__main__":
    main()
