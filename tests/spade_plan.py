"""A plain restatement of the host-side plan of mga_yolo_amd/csrc/api_spade.hip, and the table of MaskSPADE cases chosen with it.
Not a test: tests/test_spade_plan.py pins it to the built library and to what every row declares, tests/test_gpu_spade_paths.py runs the
rows on the device.  Each function names the one it mirrors.

What the C ABI shows of the plan is the scratch size (mgaspade_scratch_bytes), which is a function of the tiling's tile count and of
the split-K chunk count; the size sweep of the CPU test pins those two.  The forward channel block (cblk) is NOT visible through the
ABI: it is mirrored from the source of sp_level alone, and only a change of that source read side by side with this file shows a drift.
"""
from collections import namedtuple

from abi_header import a16

PX = 128           # kSpPx: pixels of a tile
DW_TARGET = 512    # kSpDwTarget
DH_CC = 32         # kSpDhCC: channels staged per round of k_spade_dh
GROUP_MAX = 4      # kGroupMax (args.cuh): levels of one signature per launch
MAX_LEVELS = 8     # MGACBAM_MAX_LEVELS


def cdiv(a, b):
    return (a + b - 1) // b


Tiling = namedtuple("Tiling", "TW TH ltw tiles_x tiles_y tiles")


def tiling(H, W):
    """sp_tiling: ltw = 5, 4, 3, 2 in that order, the strictly smallest tile count wins (so the widest rows win a tie)."""
    best = None
    for ltw in (5, 4, 3, 2):
        TW = 1 << ltw
        TH = PX // TW
        tx, ty = cdiv(W, TW), cdiv(H, TH)
        if best is None or tx * ty < best.tiles:
            best = Tiling(TW, TH, ltw, tx, ty, tx * ty)
    return best


Fwd = namedtuple("Fwd", "cblk ncb last")


def fwd_blocks(B, C, tiles):
    """sp_level: channels per forward workgroup, halved while the grid is small; the last block holds what is left of C.
    Mirrored from the source only (see the module's docstring)."""
    cblk = min(C, 256)
    while cblk > 64 and B * tiles * cdiv(C, cblk) < 512:
        cblk = (cblk // 2 + 15) & ~15
    ncb = cdiv(C, cblk)
    return Fwd(cblk, ncb, C - (ncb - 1) * cblk)


SplitK = namedtuple("SplitK", "nchunk tpc crosses last_len")


def split_k(B, C, tiles):
    """sp_scratch_layout: pixel chunks of k_spade_dw.  crosses: some chunk holds tiles of two samples; last_len: tiles of the last chunk."""
    total = B * tiles
    nchunk = max(1, min(total, DW_TARGET // (C // 16)))
    tpc = cdiv(total, nchunk)
    nchunk = cdiv(total, tpc)
    crosses = any((ch * tpc) // tiles != (min(total, (ch + 1) * tpc) - 1) // tiles for ch in range(nchunk))
    return SplitK(nchunk, tpc, crosses, total - (nchunk - 1) * tpc)


def dh_rounds(C):
    """k_spade_dh: channel rounds of min(C, kSpDhCC) and the channels of the last one (16 when C % 32 == 16)."""
    cc = min(C, DH_CC)
    n = cdiv(C, cc)
    return n, C - (n - 1) * cc


def scratch_bytes(B, C, H, W, hidden):
    """sp_scratch_layout (Carver: every part rounded up to 16 bytes): 4 + 2 plane sums | dW partials | 9 tap planes | dW0 partials."""
    t = tiling(H, W)
    k = split_k(B, C, t.tiles)
    BC = B * C
    return (a16(16 * BC) + a16(8 * BC) + a16(4 * k.nchunk * 2 * C * hidden * 9) + a16(4 * B * 9 * H * W)
            + a16(4 * B * t.tiles * hidden * 10))


def locate(H, W, y, x):
    """-> ((ty, tx), (row, column)): the tile of pixel (y, x) and its place inside the tile (sp_tile read backwards)."""
    t = tiling(H, W)
    return (y // t.TH, x // t.TW), (y % t.TH, x % t.TW)


# The cases.  B, C, H, W, norm, hidden and seed go to live_case (tests/test_gpu_spade.py); eps and momentum to the module and the
# oracle.  Everything after them is what the row is there for, as the plan gives it TODAY: test_spade_plan.py asserts that the mirror
# still yields it, so a change of the host rule fails there instead of moving the coverage silently.
#   tw, tiles = (tiles_x, tiles_y), ragged = (right edge, bottom edge) cut by the image, fwd = (cblk, ncb, last block),
#   dh = (rounds, channels of the last), nchunk, tpc, crosses (a split-K chunk over two samples), last_len, c16 (C % 32 == 16).
# Seeds: the smallest-effort ones for which the fp64 oracle has no pre-activation with |pre| < 1e-5 (the generator's rule of
# tests/test_gpu_spade.py: no ReLU branch can differ on the device, so no bound is widened).
Case = namedtuple("Case", "B C H W norm hidden seed eps momentum tw tiles ragged fwd dh nchunk tpc crosses last_len c16 what")


def _c(B, C, H, W, norm, hidden, seed, tw, tiles, ragged, fwd, dh, nchunk, tpc, crosses, last_len, c16, what, eps=1e-6, momentum=0.1):
    return Case(B, C, H, W, norm, hidden, seed, eps, momentum, tw, tiles, ragged, fwd, dh, nchunk, tpc, crosses, last_len, c16, what)


CASES = [
    _c(2, 32, 16, 8, "in", 16, 60, 8, (1, 1), (False, False), (32, 1, 32), (1, 32), 2, 1, False, 1, False, "exact single tile, TW = 8"),
    _c(2, 48, 30, 22, "bn", 48, 39, 8, (3, 2), (True, True), (48, 1, 48), (2, 16), 12, 1, False, 1, True,
       "ragged both ways at TW = 8, hidden 48, C % 32 == 16, eps 1e-3, momentum 0.3", eps=1e-3, momentum=0.3),
    _c(2, 112, 30, 22, "in", 32, 72, 8, (3, 2), (True, True), (64, 2, 48), (4, 16), 12, 1, False, 1, True, "cblk 64 + last block 48"),
    _c(2, 64, 32, 4, "in", 32, 60, 4, (1, 1), (False, False), (64, 1, 64), (2, 32), 2, 1, False, 1, False, "exact single tile, TW = 4"),
    _c(2, 80, 60, 10, "in", 64, 60, 4, (3, 2), (True, True), (48, 2, 32), (3, 16), 12, 1, False, 1, True,
       "ragged both ways at TW = 4, 48 + 32 blocks, three dh rounds, the last of 16"),
    _c(2, 144, 60, 10, "bn", 48, 91, 4, (3, 2), (True, True), (48, 3, 48), (5, 16), 12, 1, False, 1, True, "48 x 3 blocks, hidden 48"),
    _c(3, 1024, 32, 20, "bn", 16, 67, 4, (5, 1), (False, False), (64, 16, 64), (32, 32), 8, 2, True, 1, False,
       "C limit, 16 blocks, 32 dh rounds, nchunk 8, tpc 2, chunk over two samples, last chunk 1 tile, eps 1e-3, momentum 0.3",
       eps=1e-3, momentum=0.3),
    _c(3, 1024, 20, 20, "in", 48, 69, 32, (1, 5), (True, False), (64, 16, 64), (32, 32), 8, 2, True, 1, False,
       "the same at TW = 32 and hidden 48"),
    _c(2, 64, 20, 44, "in", 32, 17, 16, (3, 3), (True, True), (64, 1, 64), (2, 32), 18, 1, False, 1, False, "ragged both ways at TW = 16"),
    _c(2, 32, 7, 60, "bn", 32, 10, 32, (2, 2), (True, True), (32, 1, 32), (1, 32), 8, 1, False, 1, False, "ragged both ways at TW = 32"),
    _c(2, 16, 1, 37, "in", 16, 1, 32, (2, 1), (True, True), (16, 1, 16), (1, 16), 4, 1, False, 1, True, "one image row"),
    _c(2, 16, 37, 1, "bn", 16, 2, 4, (1, 2), (True, True), (16, 1, 16), (1, 16), 4, 1, False, 1, True, "one image column"),
    _c(1, 16, 2, 2, "bn", 16, 1, 32, (1, 1), (True, True), (16, 1, 16), (1, 16), 1, 1, False, 1, True, "B = 1, HW = 4 (vector statistics path)"),
    _c(3, 32, 5, 3, "in", 32, 1, 16, (1, 1), (True, True), (32, 1, 32), (1, 32), 3, 1, False, 1, False, "odd HW (scalar statistics path)"),
]


def case(B, C, H, W):
    """The table's row of that shape (shapes are unique in the table)."""
    (row,) = [c for c in CASES if (c.B, c.C, c.H, c.W) == (B, C, H, W)]
    return row


def case_id(c):
    return f"{c.B}x{c.C}x{c.H}x{c.W}-{c.norm}-h{c.hidden}"


def plan_of(c):
    """What the mirror yields for a row, in the row's own columns."""
    t = tiling(c.H, c.W)
    k = split_k(c.B, c.C, t.tiles)
    return dict(tw=t.TW, tiles=(t.tiles_x, t.tiles_y), ragged=(c.W % t.TW != 0, c.H % t.TH != 0), fwd=tuple(fwd_blocks(c.B, c.C, t.tiles)),
                dh=dh_rounds(c.C), nchunk=k.nchunk, tpc=k.tpc, crosses=k.crosses, last_len=k.last_len, c16=c.C % 32 == 16)
