"""The Detect head's maps as the criterion (detloss.py) and the post-process (detpost.py) take them: level l is (B, 4 * REG_MAX + nc, H_l, W_l),
the anchors are the cells' centres, level after level.  What both say about that input is said here once (csrc/detmaps.cuh: the kernels' side).
The kernels read the maps in place in either memory layout: NCHW contiguous, or torch.channels_last on every level (`maps_layout`).
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


def _nchw(t) -> bool:
    return t.is_contiguous()


def _nhwc(t) -> bool:
    return t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)


def maps_layout(tensors) -> str:
    """How the kernels can read the maps in place: "nhwc" when every level is dense channels_last and not every one is NCHW contiguous as
    well (a 1 x 1 level is both at once: it goes with whatever the other levels are), "nchw" when every level is NCHW contiguous, else
    "copy": levels of different layouts, strided views and mixed or unknown element types take `kernel_maps`."""
    tensors = list(tensors)
    if len({t.dtype for t in tensors}) != 1 or tensors[0].dtype not in DTYPES:
        return "copy"
    if all(_nchw(t) for t in tensors):
        return "nchw"
    if all(_nhwc(t) for t in tensors):
        return "nhwc"
    return "copy"


def device_maps(tensors):
    """The maps as a device call takes them, and that call's layout flag: channels_last maps as they are with MAPS_LAYOUT_NHWC, everything
    else through kernel_maps with 0."""
    from ._lib import MAPS_LAYOUT_NHWC
    if maps_layout(tensors) == "nhwc":
        return list(tensors), MAPS_LAYOUT_NHWC
    return kernel_maps(tensors), 0


def plan_maps(who: str, feats, channels_last: bool):
    """A static plan's external maps: they are read in place on every replay, so they must have the plan's layout.  Returns the flag."""
    from ._lib import MAPS_LAYOUT_NHWC
    want = "nhwc" if channels_last else "nchw"
    for l, f in enumerate(feats):
        ok = f.dtype in DTYPES and f.dtype == feats[0].dtype and (_nhwc(f) if channels_last else _nchw(f))
        if not ok:
            raise ValueError(f"{who}: feats[{l}] (shape {tuple(f.shape)}, strides {f.stride()}, {f.dtype}) is not a dense "
                             f"{'channels_last' if channels_last else 'NCHW contiguous'} map of one element type (channels_last={channels_last})")
    return MAPS_LAYOUT_NHWC if want == "nhwc" else 0


def zero_maps(shapes, nc: int, dtype, device, channels_last: bool = False):      # a static plan's own maps; shapes: per level (B, H, W)
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return [torch.empty(B, 4 * REG_MAX + nc, H, W, dtype=dtype, device=device, memory_format=fmt).zero_() for B, H, W in shapes]


def raise_on_status(status: torch.Tensor, message) -> None:
    """A plan's status word is set (a host read: not inside a capture).  message: the text for any non-zero status, or {code: text} where
    the codes mean different things (a code it does not name passes)."""
    s = 0 if torch.cuda.is_current_stream_capturing() else int(status.item())
    text = message.get(s) if isinstance(message, dict) else message
    if s != 0 and text:
        raise RuntimeError(text)
