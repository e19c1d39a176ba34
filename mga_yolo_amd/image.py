"""A batch of uint8 images prepared for the network in one launch (include/ext/mgaimage.h): the division by 255, the element type, the memory
format, the channel order and the bilinear resize of multi-scale training -- what the reference's trainer, validator and predictor do with a
chain of torch operators over the largest tensor of the step (ultralytics/models/yolo/detect/train.py: preprocess_batch,
ultralytics/models/yolo/detect/val.py: preprocess, ultralytics/engine/predictor.py: preprocess).

The rule.  Without a resize the result is bit for bit ``v.float() / 255``, ``v.half() / 255`` and ``v.to(torch.bfloat16) / 255`` as torch
evaluates them where the bytes live.  On the host that is round_to_dtype(fp32(v) / 255), a correctly rounded division.  On the device torch
multiplies a tensor by the fp32 reciprocal of a host scalar it is divided by, so there it is round_to_dtype(fp32(v) * (1.0f / 255.0f)): in
fp16 and bf16 the same bits as the quotient for all 256 bytes, in fp32 one ulp away for 126 of them -- measured on an MI355X, and the kernel
follows it, since the call stands in for that composition.  With a resize,
``F.interpolate(v.float() / 255, size=size, mode="bilinear", align_corners=False)`` rounded once to the output type, the taps being the fp32
quotients of the four bytes; no full-size fp32 image exists at any point.

uint8 tensors on the device go through ``mgaimg_run``: one launch on the current stream, no allocation beyond the result and no host
synchronisation, so ``ImagePlan.run`` can sit in a captured graph in front of a ``SlicePlan``'s step.  uint8 tensors on the host take
``_host_batch``: the same rule in torch operators.

Not built: LetterBox and every cv2 augmentation, antialiasing, other interpolation modes, a resize of the masks (the reference does not resize
them either), more than 4 channels, a gradient (the input is bytes).
"""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from ._binding import DTYPES, call, fill_image

__all__ = ["image_batch", "multi_scale_size", "ImagePlan", "preprocess_batch", "preprocess"]

_LAYOUTS = ("nchw", "nhwc")


def _geometry(shape, src_layout: str, size) -> Tuple[int, int, int, int, int, int]:
    """-> B, C, H, W of the source and the destination's (H', W'), checked"""
    if src_layout not in _LAYOUTS:
        raise ValueError(f"image_batch: src_layout={src_layout!r} (one of {_LAYOUTS})")
    if len(shape) != 4:
        raise ValueError(f"image_batch: img must have 4 dimensions, (B,C,H,W) or (B,H,W,C) with src_layout='nhwc'; got {tuple(shape)}")
    B, Cc, H, W = (shape[0], shape[3], shape[1], shape[2]) if src_layout == "nhwc" else tuple(shape)
    if not 1 <= Cc <= _lib.IMG_MAX_C:
        raise ValueError(f"image_batch: {Cc} channels (1 .. {_lib.IMG_MAX_C})")
    if min(B, H, W) < 1:
        raise ValueError(f"image_batch: an empty batch or image, shape {tuple(shape)}")
    if size is None:
        oh, ow = H, W
    else:
        oh, ow = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if oh < 1 or ow < 1:
            raise ValueError(f"image_batch: size={size} (each at least 1)")
    if B * Cc * max(H * W, oh * ow) >= 1 << 31:
        raise ValueError(f"image_batch: B * C * max(H * W, H' * W') = {B * Cc * max(H * W, oh * ow)} is not below 2^31")
    return B, Cc, H, W, oh, ow


def _check_src(img) -> None:
    if not isinstance(img, torch.Tensor):
        raise TypeError(f"image_batch: img must be a torch.Tensor, not {type(img).__name__}")
    if img.dtype != torch.uint8:
        raise TypeError(f"image_batch: img must be uint8, not {img.dtype} (a float batch is already prepared)")


def _check_out(out, shape, dtype, channels_last: bool, device) -> None:
    if not isinstance(out, torch.Tensor):
        raise TypeError(f"image_batch: out must be a torch.Tensor, not {type(out).__name__}")
    if out.dtype != dtype:
        raise TypeError(f"image_batch: out is {out.dtype}, dtype={dtype} was asked for")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"image_batch: out has shape {tuple(out.shape)}, the result has {tuple(shape)}")
    if out.device != device:
        raise ValueError(f"image_batch: out lives on {out.device}, img on {device}")
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    if not out.is_contiguous(memory_format=fmt):
        raise ValueError(f"image_batch: out is not contiguous in {fmt} (strides {tuple(out.stride())})")


def _empty(shape, dtype, channels_last: bool, device) -> torch.Tensor:
    return torch.empty(shape, dtype=dtype, device=device, memory_format=torch.channels_last if channels_last else torch.contiguous_format)


def _host_batch(img, dtype, size, src_layout: str, reverse_channels: bool) -> torch.Tensor:
    """The rule in torch operators, (B,C,H',W') in `dtype`; runs where `img` lives."""
    v = img.permute(0, 3, 1, 2) if src_layout == "nhwc" else img
    if reverse_channels:
        v = v.flip(1)
    if size is None or tuple(size) == tuple(v.shape[2:]):
        return v.to(dtype) / 255
    return F.interpolate(v.float() / 255, size=tuple(size), mode="bilinear", align_corners=False).to(dtype)


def image_batch(img: torch.Tensor, *, dtype: torch.dtype = torch.float32, channels_last: bool = False, size=None, src_layout: str = "nchw",
                reverse_channels: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prepare a batch of uint8 images: (B,C,H,W) contiguous, or (B,H,W,C) contiguous with ``src_layout="nhwc"`` (a predictor's stacked
    arrays); C is 1 .. 4.  Returns (B,C,H',W') in `dtype` (fp32, fp16 or bf16), contiguous or -- ``channels_last=True`` -- in
    torch.channels_last.  ``size``: None, an int or (H', W'): the bilinear resize of F.interpolate(align_corners=False); None or the source's
    own size: no resize, and the result is bit for bit ``img.to(dtype) / 255`` as torch evaluates it where `img` lives.
    ``reverse_channels``: destination channel c is source channel C - 1 - c (BGR to RGB).  ``out``: write there (its shape, dtype, device and memory format are checked) and return it.
    A device tensor is one launch on the current stream; a host tensor takes the torch composition.  Not differentiable: the input is bytes."""
    _check_src(img)
    if dtype not in DTYPES:
        raise TypeError(f"image_batch: dtype={dtype} (torch.float32, torch.float16 or torch.bfloat16)")
    B, Cc, H, W, oh, ow = _geometry(img.shape, src_layout, size)
    if not img.is_contiguous():
        raise ValueError(f"image_batch: img is not contiguous (shape {tuple(img.shape)}, strides {tuple(img.stride())}); "
                         "pass the stacked array as it is with src_layout='nhwc' instead of a permuted view")
    shape = (B, Cc, oh, ow)
    if out is not None:
        _check_out(out, shape, dtype, channels_last, img.device)
    if not img.is_cuda:
        res = _host_batch(img, dtype, (oh, ow), src_layout, reverse_channels)
        if out is None:
            return res.contiguous(memory_format=torch.channels_last) if channels_last else res.contiguous()
        out.copy_(res)
        return out
    if out is None:
        out = _empty(shape, dtype, channels_last, img.device)
    D = _lib.ImageDesc()
    fill_image(D, img, out, src_layout == "nhwc", reverse_channels)
    call("mgaimg_run", img.device, C.byref(D))
    return out


def multi_scale_size(imgsz: int, stride: int, hw, rng=random) -> Optional[Tuple[int, int]]:
    """The size the reference's trainer resizes a batch of shape (.., H, W) = hw to under ``multi_scale``: ONE draw
    ``rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride)) // stride * stride``, the factor sf = sz / max(hw), and per axis
    ``ceil(x * sf / stride) * stride``.  None when sf == 1 (the reference does not resize then).  A seeded run picks the sizes the reference
    picks: exactly one draw per call, from `rng` (the `random` module, or a random.Random)."""
    sz = rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride)) // stride * stride
    sf = sz / max(hw)
    if sf == 1:
        return None
    return tuple(math.ceil(x * sf / stride) * stride for x in hw)


class ImagePlan:
    """image_batch on static buffers, for a captured graph: the loop copies the batch's bytes into ``src`` (``plan.src.copy_(batch,
    non_blocking=True)``), ``run()`` is one launch with no allocation, ``out`` holds the result -- alone under torch.cuda.graph or in front of
    a SlicePlan's step.  The size is fixed at creation; the changing shapes of ``multi_scale`` are for the eager call."""

    def __init__(self, src: torch.Tensor, out: torch.Tensor, src_layout: str, reverse_channels: bool):
        self.src, self.out = src, out
        self.src_layout, self.reverse_channels = src_layout, reverse_channels
        self.desc = _lib.ImageDesc()
        fill_image(self.desc, src, out, src_layout == "nhwc", reverse_channels)

    @classmethod
    def create(cls, B: int, C: int, H: int, W: int, *, dtype: torch.dtype = torch.float32, channels_last: bool = False, size=None,
               src_layout: str = "nchw", reverse_channels: bool = False, device="cuda") -> "ImagePlan":
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"ImagePlan: device={device} (the plan owns device buffers; host tensors take image_batch)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in DTYPES:
            raise TypeError(f"ImagePlan: dtype={dtype} (torch.float32, torch.float16 or torch.bfloat16)")
        shape = (B, H, W, C) if src_layout == "nhwc" else (B, C, H, W)
        B, C, H, W, oh, ow = _geometry(shape, src_layout, size)
        src = torch.zeros(shape, dtype=torch.uint8, device=device)
        return cls(src, _empty((B, C, oh, ow), dtype, channels_last, device), src_layout, reverse_channels)

    def run(self) -> torch.Tensor:
        call("mgaimg_run", self.src.device, C.byref(self.desc))
        return self.out

    def launches(self) -> int:
        return 1


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's two methods (install(preprocess=True) binds them on its classes)
# ---------------------------------------------------------------------------------------------------------------------------
_ORIGINALS: dict = {}        # (class, method name) -> the method install() replaced: what a batch that is not bytes goes to


def _original(self, name: str):
    for klass in type(self).__mro__:
        fn = _ORIGINALS.get((klass, name))
        if fn is not None:
            return fn
    raise RuntimeError(f"mga_yolo_amd.image: no original {name} recorded for {type(self).__name__}")


def _is_bytes(batch) -> bool:
    img = batch.get("img") if hasattr(batch, "get") else None
    return isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and img.dim() == 4 and 1 <= img.shape[1] <= _lib.IMG_MAX_C


def preprocess_batch(self, batch):
    """DetectionTrainer.preprocess_batch: the bytes go to the device, then ONE image_batch call -- fp32, under ``args.multi_scale`` at the
    size the reference draws (multi_scale_size: one `random.randrange`).  A batch whose ``img`` is not uint8 takes the method this replaced."""
    if not _is_bytes(batch):
        return _original(self, "preprocess_batch")(self, batch)
    img = batch["img"].to(self.device, non_blocking=True).contiguous()
    size = multi_scale_size(self.args.imgsz, self.stride, tuple(img.shape[2:])) if self.args.multi_scale else None
    batch["img"] = image_batch(img, dtype=torch.float32, size=size)
    return batch


def preprocess(self, batch):
    """DetectionValidator.preprocess: the bytes go to the device, then ONE image_batch call in fp16 (``args.half``) or fp32; the three label
    tensors are moved as before.  A batch whose ``img`` is not uint8 takes the method this replaced."""
    if not _is_bytes(batch):
        return _original(self, "preprocess")(self, batch)
    img = batch["img"].to(self.device, non_blocking=True).contiguous()
    batch["img"] = image_batch(img, dtype=torch.float16 if self.args.half else torch.float32)
    for k in ("batch_idx", "cls", "bboxes"):
        batch[k] = batch[k].to(self.device)
    return batch
