"""TEST INFRASTRUCTURE — CPU restatement of the reference's multi-scale segmentation loss, default mode.

Follows mga_yolo/nn/losses/segmentation.py: `_dice_probs` :38-42, `forward` :87-151 (BCEWithLogitsLoss(reduction="mean") :36,
soft Dice on sigmoid(pred) :135, scale weights :112, nearest target resize :103-110, loss_lambda :149).  Only tests/,
__graft_entry__.smoke() and the benchmarks' CPU-baseline leg may import this.

PINNED by outputs of the reference itself: ``oracle/gen_golden_segloss.py`` imported the reference's own ``SegmentationLoss`` in the
build container (its module-scope LOGGER import needs cv2, absent here; the in-process stand-in of SURVEY appendix A2 satisfies it and
is never executed) and stored logits, targets, total, every log entry and d total / d logits for 16 cases -- both modes, nearest and
bilinear (MGA_PROB_MODE) target resize, 3-D targets, missing levels, weights -- in ``tests/golden/segloss_*.npz``; the Kendall combine
of ``MGAModel.loss`` (model/model.py:204-206), evaluated by the reference model, in ``tests/golden/kendall_*.npz``.
``tests/test_segloss.py`` checks this restatement against them; fp64 logits select an evaluation in double, fp64 targets an explicit fp64
resampler (`resample64`): together the reference of the loss-side rows (tests/test_loss_rows_tables.py pins it).  Unified-Focal mode (`_lmf` :44-63, `_lmft` :65-85) is restated too.
"""
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F


@dataclass
class SegLossConfig:                       # segmentation.py:9-21
    bce_weight: float = 1.0
    dice_weight: float = 1.0
    scale_weights: Sequence[float] = (1.0, 1.0, 1.0)
    smooth: float = 1.0
    loss_lambda: float = 1.0
    enabled: bool = True
    use_unified_focal: bool = False
    ufl_lambda: float = 0.5
    ufl_delta: float = 0.6
    ufl_gamma: float = 0.5


def dice_probs(probs, tgt, smooth):        # segmentation.py:38-42
    inter = (probs * tgt).sum(dim=(1, 2, 3))
    denom = probs.sum(dim=(1, 2, 3)) + tgt.sum(dim=(1, 2, 3)) + smooth
    return 1.0 - (2.0 * inter + smooth) / denom


def _fp(t):
    """The reference's ``.float()``; an fp64 tensor stays fp64, so the whole loss can be evaluated in double."""
    return t if t.dtype == torch.float64 else t.float()


def resample_index64(out_size: int, in_size: int, bilinear: bool):
    """One axis of the target resize, coordinates and weights in fp64 -> (i0, i1, w1) with out[d] = (1 - w1) in[i0] + w1 in[i1].
    nearest: F.interpolate(mode="nearest")'s index rule, which ATen evaluates in fp32 (maskcbam_oracle.nearest_src_index: the index
    is part of the definition, not a rounding error), w1 = 0.  bilinear, align_corners=False: src = max(in/out * (d + 0.5) - 0.5, 0),
    i0 = min(floor(src), in - 1), i1 = min(i0 + 1, in - 1), w1 = src - i0  (ATen area_pixel_compute_source_index, in double here)."""
    if not bilinear:
        from .maskcbam_oracle import nearest_src_index
        i0 = torch.from_numpy(nearest_src_index(out_size, in_size))
        return i0, i0, torch.zeros(out_size, dtype=torch.float64)
    d = torch.arange(out_size, dtype=torch.float64)
    src = ((float(in_size) / float(out_size)) * (d + 0.5) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp_max(in_size - 1)
    i1 = (i0 + 1).clamp_max(in_size - 1)
    return i0, i1, src - i0.double()


def resample64(tgt: torch.Tensor, out_h: int, out_w: int, bilinear: bool) -> torch.Tensor:
    """(..., Ht, Wt) -> (..., out_h, out_w) in fp64: an explicit gather with two clamped taps per axis (segmentation.py:103-110)."""
    t = tgt.double()
    y0, y1, wy = resample_index64(out_h, t.shape[-2], bilinear)
    x0, x1, wx = resample_index64(out_w, t.shape[-1], bilinear)
    top = t[..., y0, :][..., x0] * (1.0 - wx) + t[..., y0, :][..., x1] * wx
    bot = t[..., y1, :][..., x0] * (1.0 - wx) + t[..., y1, :][..., x1] * wx
    return top * (1.0 - wy)[:, None] + bot * wy[:, None]


def lmf(logits, tgt, delta, gamma, eps=1e-6):          # segmentation.py:44-63
    x, t = _fp(logits), _fp(tgt)
    probs = torch.sigmoid(x)
    pt = torch.where(t > 0.5, probs, 1.0 - probs).clamp(eps, 1.0 - eps)
    ce = _fp(F.binary_cross_entropy_with_logits(x, t, reduction="none"))
    w = torch.where(t > 0.5, delta, 1.0 - delta).to(x.dtype)
    base = (1.0 - pt).clamp_min(eps)
    return (base.pow(1.0 - gamma) * ce * w).mean()


def lmft(logits, tgt, delta, gamma, smooth, eps=1e-6):  # segmentation.py:65-85
    x, t = _fp(logits), _fp(tgt)
    p = torch.sigmoid(x)
    tp = (p * t).sum(dim=(1, 2, 3))
    fn = (t * (1.0 - p)).sum(dim=(1, 2, 3))
    fp = ((1.0 - t) * p).sum(dim=(1, 2, 3))
    denom = (tp + delta * fn + (1.0 - delta) * fp + smooth).clamp_min(eps)
    mti = (tp + smooth) / denom
    return (1.0 - mti).clamp_min(eps).pow(gamma).mean()


def forward(preds: Dict[str, torch.Tensor], targets: List[torch.Tensor], cfg: SegLossConfig, bilinear_targets: bool = False
            ) -> Tuple[torch.Tensor, Dict[str, float]]:
    """segmentation.py:87-151.  `bilinear_targets` stands for the MGA_PROB_MODE environment switch (:103-108).
    Each input is processed at its own precision.  fp64 logits: every op of the loss runs in double.  fp64 targets at another resolution:
    resampled by `resample64`, coordinates and weights in double.  Targets of any other type are resampled as the reference resamples
    them (F.interpolate on `.float()`), so fp64 logits with stored fp32 targets give the loss in double on the targets the reference saw
    -- what the goldens pin; fp64 logits AND targets give the whole evaluation in double -- the reference of the loss-side rows."""
    first = next(iter(preds.values()))
    if not cfg.enabled:
        return torch.zeros((), device=first.device), {}
    f64 = first.dtype == torch.float64
    total = torch.zeros((), device=first.device, dtype=torch.float64 if f64 else torch.float32)
    logs: Dict[str, float] = {}
    for i, sk in enumerate(["p3", "p4", "p5"]):
        if sk not in preds or i >= len(targets):
            continue
        pred, tgt = preds[sk], targets[i]
        if tgt.dim() == 3:
            tgt = tgt.unsqueeze(1)
        if f64 and (tgt.dtype == torch.float64 or tgt.shape[-2:] == pred.shape[-2:]):
            tgt = tgt.double() if tgt.shape[-2:] == pred.shape[-2:] else resample64(tgt, *pred.shape[-2:], bilinear_targets)
        elif tgt.shape[-2:] != pred.shape[-2:]:
            if bilinear_targets:
                tgt = F.interpolate(tgt.float(), size=pred.shape[-2:], mode="bilinear", align_corners=False)
            else:
                tgt = F.interpolate(tgt.float(), size=pred.shape[-2:], mode="nearest")
        w_scale = cfg.scale_weights[i] if i < len(cfg.scale_weights) else 1.0
        if cfg.use_unified_focal:
            a = lmf(_fp(pred), _fp(tgt), cfg.ufl_delta, cfg.ufl_gamma)
            b = lmft(_fp(pred), _fp(tgt), cfg.ufl_delta, cfg.ufl_gamma, cfg.smooth)
            combined = w_scale * (cfg.ufl_lambda * a + (1.0 - cfg.ufl_lambda) * b)
        else:
            a = F.binary_cross_entropy_with_logits(pred, _fp(tgt), reduction="mean")
            b = dice_probs(torch.sigmoid(pred), _fp(tgt), cfg.smooth).mean()
            combined = w_scale * (cfg.bce_weight * a + cfg.dice_weight * b)
        logs[f"{sk}_bce"], logs[f"{sk}_dice"] = float(a.detach()), float(b.detach())
        if not torch.isfinite(combined):
            raise FloatingPointError("Segmentation loss became non-finite.")
        total = total + _fp(combined)
        logs[f"{sk}_combined"] = float(combined.detach())
    total = total * cfg.loss_lambda
    logs["seg_total"] = float(total.detach())
    return total, logs


def kendall_combine(det_loss: torch.Tensor, seg_total: torch.Tensor, log_vars: torch.Tensor) -> torch.Tensor:
    """mga_yolo/model/model.py:204-206: L = e^{-s_det} L_det + s_det + e^{-s_seg} L_seg + s_seg (det_loss is the criterion's vector)."""
    s_det, s_seg = log_vars[0], log_vars[1]
    return torch.exp(-s_det) * det_loss + s_det + torch.exp(-s_seg) * seg_total + s_seg
