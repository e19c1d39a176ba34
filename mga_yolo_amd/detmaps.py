"""The Detect head's maps as the criterion (detloss.py) and the post-process (detpost.py) take them: level l is (B, 4 * REG_MAX + nc, H_l, W_l),
the anchors are the cells' centres, level after level.  What both say about that input is said here once (csrc/detmaps.cuh: the kernels' side).
The two host paths keep their own arithmetic on the bins: they round differently and each is pinned by its stored results."""
import torch

from ._binding import DTYPES
from ._lib import DET_REG_MAX as REG_MAX


def anchor_grid(feats, strides, dtype, device):
    """The anchors' centres (A, 2) as (x, y) in grid units and their strides (A, 1); every value is exact in any float type."""
    pts, st = [], []
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        yy, xx = torch.meshgrid(torch.arange(h, dtype=dtype, device=device) + 0.5, torch.arange(w, dtype=dtype, device=device) + 0.5, indexing="ij")
        pts.append(torch.stack((xx, yy), -1).view(-1, 2))
        st.append(torch.full((h * w, 1), float(s), dtype=dtype, device=device))
    return torch.cat(pts), torch.cat(st)


def check_maps(who: str, feats, nc: int, strides) -> None:
    if any(f.dim() != 4 or f.shape[1] != 4 * REG_MAX + nc or f.shape[0] != feats[0].shape[0] for f in feats):
        raise ValueError(f"{who}: every feature map must be (B, {4 * REG_MAX + nc}, H, W)")
    if len(strides) != len(feats):
        raise ValueError(f"{who}: one stride per feature map")


def kernel_maps(tensors):
    """The tensors as the kernels read them: one element type the library has (else fp32), NCHW contiguous (channels_last included)."""
    if len({t.dtype for t in tensors}) != 1 or tensors[0].dtype not in DTYPES:
        tensors = [t.float() for t in tensors]
    return [t.contiguous() for t in tensors]


def zero_maps(shapes, nc: int, dtype, device):                # a static plan's own maps; shapes: per level (B, H, W)
    return [torch.zeros(B, 4 * REG_MAX + nc, H, W, dtype=dtype, device=device) for B, H, W in shapes]


def raise_on_status(status: torch.Tensor, message: str) -> None:      # a plan's status word is set (a host read: not inside a capture)
    if not torch.cuda.is_current_stream_capturing() and int(status.item()) != 0:
        raise RuntimeError(message)
