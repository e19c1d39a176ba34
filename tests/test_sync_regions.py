"""CPU-side check of the Python mirror of the ctx hand-off region (_lib.sync_regions): regions are only ever appended, so a ctx written
under an older layout keeps every counter where it was, and the last region ends the region's length."""
import pytest

from mga_yolo_amd import _lib

# name -> (offset, length) in int32 words, for nf = B * (ceil(H*W / 16) + 1) tile flags: the layout before the arrival words were added
OLD = ("gate", "status", "ca", "tiles", "conv_tiles", "merged_tiles", "merged_conv_tiles", "wsa_tiles", "sweeps")


@pytest.mark.parametrize("shape", [(32, 64, 80, 80), (9, 128, 8, 8), (1, 48, 17, 17), (3, 8, 9, 7)])
def test_arrival_words_are_appended_inside_sync_len(shape):
    B, C, H, W = shape
    r = _lib.sync_regions(B, C, H, W)
    nf = B * ((H * W + 15) // 16 + 1)
    want, o = {}, 0
    for name, n in zip(OLD, (nf, 4, B, nf, nf, nf, nf, nf, B * C)):
        want[name] = (o, n)
        o += n
    assert {k: r[k] for k in OLD} == want, "an existing region moved"
    assert list(r)[:len(OLD)] == list(OLD) and list(r)[len(OLD):] == ["arrive"]
    assert r["arrive"] == (o, B * _lib.ARRIVE_STRIDE), "one arrival word per sample, a stride apart, behind everything that was there"
    assert r["arrive"][0] + r["arrive"][1] == _lib.sync_len(B, C, H, W)
    ends = sorted((a, a + n) for a, n in r.values())
    assert all(e0 == s1 for (_, e0), (s1, _) in zip(ends, ends[1:])), "regions overlap or leave a gap"
