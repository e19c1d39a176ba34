"""The detection criterion of the training step (include/mgadet.h): task-aligned assignment, CIoU, DFL and BCE on the Detect head's three
feature maps, behind the interface of the reference's `v8DetectionLoss` (ultralytics/utils/loss.py:194-297).

Device tensors go through `mgamaps_det_forward` / `mgamaps_det_backward` (include/ext/mgamaps.h: `mgadet_forward` / `mgadet_backward` with the
maps' layout as a flag): four launches forward, one backward, no host synchronisation, so the criterion can sit inside a captured graph
(`DetLossPlan`).  Maps that are torch.channels_last on every level are read in place and their gradients come back channels_last, bit for bit
what NCHW maps of the same values give; NCHW contiguous maps likewise; anything else is made NCHW contiguous first (detmaps.maps_layout).
Host tensors take `_host_loss`, the same semantics stated in torch ops.

Not built: levels of different layouts in one call (they are made contiguous here), reg_max other than 16, the rotated and the segmentation criteria, and
the reference's own half-precision arithmetic under autocast: half features are read, and everything is accumulated, in fp32.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from ._binding import call, fill_det
from .detlabels import LabelBuffers, as_labels, loss_boxes, rows_per_image, sized_ws
from .detmaps import REG_MAX, anchor_grid, check_maps, device_maps, plan_maps, raise_on_status, zero_maps

EPS = 1e-7


# ---------------------------------------------------------------------------------------------------------------------------
# torch ops (host tensors): the project's own statement of the criterion
# ---------------------------------------------------------------------------------------------------------------------------
def _ciou(p: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """Complete IoU of xyxy boxes p and q (broadcast over the leading dimensions); both heights carry eps, the trade-off factor alpha is a
    constant for the gradient."""
    px1, py1, px2, py2 = p.unbind(-1)
    qx1, qy1, qx2, qy2 = q.unbind(-1)
    w1, h1, w2, h2 = px2 - px1, py2 - py1 + EPS, qx2 - qx1, qy2 - qy1 + EPS
    inter = (torch.minimum(px2, qx2) - torch.maximum(px1, qx1)).clamp(min=0) * (torch.minimum(py2, qy2) - torch.maximum(py1, qy1)).clamp(min=0)
    union = w1 * h1 + w2 * h2 - inter + EPS
    iou = inter / union
    cw, ch = torch.maximum(px2, qx2) - torch.minimum(px1, qx1), torch.maximum(py2, qy2) - torch.minimum(py1, qy1)
    c2 = cw * cw + ch * ch + EPS
    rho2 = ((qx1 + qx2 - px1 - px2) ** 2 + (qy1 + qy2 - py1 - py2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = (v / (v - iou + (1 + EPS))).detach()
    return iou - (rho2 / c2 + v * alpha)


def _ground_truths(batch_idx, cls, bboxes, B: int, img_wh, dtype):
    """Per image its label rows in order: boxes (B, M, 4) xyxy in pixels, labels (B, M) int64, valid (B, M), rows (B, M) (-1: none)."""
    rows, has, _ = rows_per_image(batch_idx, B, integral=False)
    safe = rows.clamp(min=0)
    boxes = torch.where(has[..., None], loss_boxes(bboxes.to(dtype), *img_wh)[safe], torch.zeros((), dtype=dtype, device=bboxes.device))
    labels = cls.to(torch.int64)[safe] * has
    return boxes, labels, boxes.sum(-1) > 0, rows


def _assign(scores, pred_px, anc_px, boxes, labels, valid, nc: int, topk: int, lowest_first: bool = True):
    """Task-aligned assignment on detached quantities.  scores (B, A, nc) logits, pred_px (B, A, 4), anc_px (A, 2), boxes (B, M, 4).
    Returns fg (B, A) bool, slot (B, A) int64, norm (B, A): the anchor's target score at its ground truth's class.  lowest_first: ties
    of the metric go to the lowest anchor index (the kernels' rule); False: to the highest (the results that matter do not depend on it)."""
    B, A = scores.shape[:2]
    M = boxes.shape[1]
    if M == 0:
        z = torch.zeros(B, A, dtype=scores.dtype, device=scores.device)
        return z.bool(), z.long(), z
    deltas = torch.cat((anc_px[None, None] - boxes[:, :, None, :2], boxes[:, :, None, 2:] - anc_px[None, None]), -1)
    cand = (deltas.amin(-1) > 1e-9) & valid[:, :, None]                                  # (B, M, A)
    ov = _ciou(boxes[:, :, None, :], pred_px[:, None]).clamp(min=0) * cand
    lab = labels.clamp(0, nc - 1)
    sc = scores.sigmoid().permute(0, 2, 1).gather(1, lab[:, :, None].expand(-1, -1, A))
    met = torch.where(cand, sc.sqrt() * ov ** 6, -torch.ones_like(ov))
    key = met if lowest_first else met.flip(-1)
    order = key.sort(dim=-1, descending=True, stable=True).indices[..., :topk]
    if not lowest_first:
        order = A - 1 - order
    pos = torch.zeros_like(cand).scatter_(-1, order, True) & cand
    multi = pos.sum(1) > 1
    best = F.one_hot(ov.argmax(1), M).permute(0, 2, 1).bool()
    pos = torch.where(multi[:, None], best, pos)
    met0 = met.clamp(min=0) * pos
    pos_m, pos_o = met0.amax(-1, keepdim=True), (ov * pos).amax(-1, keepdim=True)
    norm = (met0 * pos_o / (pos_m + 1e-9)).amax(1)
    return pos.any(1), pos.float().argmax(1), norm


def _host_loss(feats, batch_idx, cls, bboxes, nc, strides, gains, topk, lowest_first: bool = True):
    """The criterion in torch ops, on whatever device its arguments live (the host path; on the device it is what tools/bench_det.py
    times the kernels against).  Returns (loss * B, loss.detach(), assignment)."""
    B = feats[0].shape[0]
    dtype = feats[0].dtype
    no = 4 * REG_MAX + nc
    x = torch.cat([f.reshape(B, no, -1) for f in feats], 2).permute(0, 2, 1)             # (B, A, no)
    A = x.shape[1]
    dist, scores = x[..., :4 * REG_MAX].reshape(B, A, 4, REG_MAX), x[..., 4 * REG_MAX:]
    anc, st = anchor_grid(feats, strides, dtype, x.device)
    dev = x.device
    d = dist.softmax(-1) @ torch.arange(REG_MAX, dtype=dtype, device=dev)
    pred = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)                           # grid units
    img_wh = (feats[0].shape[3] * strides[0], feats[0].shape[2] * strides[0])
    boxes, labels, valid, rows = _ground_truths(batch_idx, cls, bboxes, B, img_wh, dtype)
    with torch.no_grad():
        fg, slot, norm = _assign(scores, pred * st, anc * st, boxes, labels, valid, nc, topk, lowest_first)
    M = boxes.shape[1]
    bi = torch.arange(B, device=dev)[:, None]
    if M:
        t_lab, t_box = labels.clamp(0, nc - 1)[bi, slot], boxes[bi, slot]
        t_row = torch.where(fg, rows[bi, slot], -torch.ones_like(slot))
    else:
        t_lab, t_box = torch.zeros(B, A, dtype=torch.int64, device=dev), torch.zeros(B, A, 4, dtype=dtype, device=dev)
        t_row = -torch.ones(B, A, dtype=torch.int64, device=dev)
    t_scores = F.one_hot(t_lab, nc).to(dtype) * (norm * fg)[..., None]
    tss = t_scores.sum().clamp(min=1)
    l_cls = F.binary_cross_entropy_with_logits(scores, t_scores, reduction="none").sum() / tss
    w = norm[fg]
    tb = (t_box / st)[fg]
    l_box = ((1 - _ciou(pred[fg], tb)) * w).sum() / tss
    a_fg = anc[None].expand(B, -1, -1)[fg]
    ltrb = torch.cat((a_fg - tb[:, :2], tb[:, 2:] - a_fg), -1).clamp(0, REG_MAX - 1 - 0.01)
    tl = ltrb.long()
    wl = (tl + 1).to(dtype) - ltrb
    logp = dist[fg].log_softmax(-1)                                                      # (n_fg, 4, 16)
    ce = -(logp.gather(-1, tl[..., None]).squeeze(-1) * wl + logp.gather(-1, tl[..., None] + 1).squeeze(-1) * (1 - wl))
    l_dfl = (ce.mean(-1) * w).sum() / tss
    loss = torch.stack((l_box, l_cls, l_dfl)) * torch.tensor([float(g) for g in gains], dtype=dtype, device=dev)
    assignment = dict(fg=fg, target_gt=t_row, target_scores=t_scores.detach(), target_bboxes=t_box * fg[..., None],
                      weight=(norm * fg).detach(), status=torch.zeros(1, dtype=torch.int32, device=dev))
    return loss * B, loss.detach(), assignment


# ---------------------------------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------------------------------
class _DetState:
    """The buffers of one criterion call and its descriptor: outputs of the forward the backward reads again."""

    def __init__(self, feats, strides, nc, topk, m_cap, gains, batch_idx, cls, bboxes, n, out=None, g_feats=None, upstream=None, flags=0):
        dev = feats[0].device
        self.flags = int(flags)                                  # 0 or _lib.MAPS_LAYOUT_NHWC: how feats and g_feats lie in memory
        B, A = feats[0].shape[0], sum(f.shape[2] * f.shape[3] for f in feats)
        i32, f32 = torch.int32, torch.float32
        self.assign_gt = torch.empty(B, A, dtype=i32, device=dev)
        self.assign_score = torch.empty(B, A, dtype=f32, device=dev)
        self.out = out if out is not None else torch.empty(3, dtype=f32, device=dev)
        self.items = torch.empty(3, dtype=f32, device=dev)
        self.status = torch.empty(1, dtype=i32, device=dev)
        self.args = (feats, strides, nc, topk, m_cap, gains, batch_idx, cls, bboxes, n, self.assign_gt, self.assign_score, self.out,
                     self.items, self.status)
        self.desc, self.ws = sized_ws(_lib.DetDesc(), fill_det, _lib.det_ws_bytes, self.args, dev, g_feats=g_feats, upstream=upstream)

    def bind(self, g_feats, upstream):
        fill_det(self.desc, *self.args, ws=self.ws, g_feats=g_feats, upstream=upstream)

    def forward(self, dev):
        call("mgamaps_det_forward", dev, C.byref(self.desc), self.flags)

    def backward(self, dev):
        call("mgamaps_det_backward", dev, C.byref(self.desc), self.flags)


class _DetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cfg, batch_idx, cls, bboxes, *feats):
        nc, strides, gains, topk, m_cap, flags = cfg
        st = _DetState(feats, strides, nc, topk, m_cap, gains, batch_idx, cls, bboxes, None, flags=flags)
        st.forward(feats[0].device)
        ctx.st = st
        ctx.mark_non_differentiable(st.items, st.assign_gt, st.assign_score, st.status)
        return st.out, st.items, st.assign_gt, st.assign_score, st.status

    @staticmethod
    def backward(ctx, g_out, *_):
        st = ctx.st
        feats = st.args[0]
        fmt = torch.channels_last if st.flags & _lib.MAPS_LAYOUT_NHWC else torch.contiguous_format
        g_feats = [torch.empty_like(f, memory_format=fmt) for f in feats]           # the maps' own layout (a 1 x 1 level is both: said outright)
        up = g_out.to(torch.float32).contiguous()
        st.bind(g_feats, up)
        st.backward(feats[0].device)
        return (None, None, None, None, *g_feats)


def detection_loss(feats: Sequence[torch.Tensor], batch_idx: torch.Tensor, cls: torch.Tensor, bboxes: torch.Tensor, *, nc: int,
                   strides: Sequence[int] = (8, 16, 32), gains: Sequence[float] = (7.5, 0.5, 1.5), topk: int = 10,
                   m_cap: Optional[int] = None, return_assignment: bool = False):
    """The detection criterion on the Detect maps `feats` (level l: (B, 64 + nc, H_l, W_l)) and the batch's labels (`batch_idx` (n),
    `cls` (n), `bboxes` (n, 4) xywh normalised): returns (gains * (box, cls, dfl) * B, its detached per-image form), as the reference's
    criterion does, differentiable with respect to the features.  `m_cap`: the ground truths an image may have; None sizes it from the
    labels with one host read, a given value reads nothing back (an image with more rows then sets the status word and makes the loss
    NaN).  return_assignment adds a dict: fg (B, A), target_gt (B, A: the label row, -1 background), target_scores (B, A, nc),
    target_bboxes (B, A, 4 in pixels), weight (B, A), status (1)."""
    feats = list(feats)
    check_maps("detection_loss", feats, nc, strides)
    dev = feats[0].device
    b_, c_, x_ = as_labels(batch_idx, cls, bboxes, dev)
    if not feats[0].is_cuda:
        if any(f.is_cuda for f in feats):
            raise RuntimeError("detection_loss: the feature maps must all live on the GPU or all on the host")
        loss, items, asg = _host_loss([f.float() for f in feats], b_, c_, x_, nc, strides, gains, topk)
        return (loss, items, asg) if return_assignment else (loss, items)
    feats, flags = device_maps(feats)
    if m_cap is None:                                        # the criterion's own sizing (detlabels.py: not detlabels.size_m_cap's rule)
        m_cap = int(torch.bincount(b_.long().clamp(0, feats[0].shape[0] - 1)).max()) if b_.numel() else 1
        m_cap = max(m_cap, 1)
    out, items, gt, score, status = _DetFn.apply((int(nc), tuple(int(s) for s in strides), tuple(float(g) for g in gains), int(topk),
                                                  int(m_cap), flags), b_, c_, x_, *feats)
    if not return_assignment:
        return out, items
    return out, items, assignment_views(gt, score, status, c_, x_, nc, feats[0].shape[3] * strides[0], feats[0].shape[2] * strides[0])


def assignment_views(gt, score, status, cls, bboxes, nc: int, img_w: float, img_h: float) -> Dict[str, torch.Tensor]:
    """The kernels' per-anchor assignment (label row, target score) in the reference's terms."""
    fg = gt >= 0
    if cls.numel():
        row = gt.clamp(min=0).long()
        lab = cls.long().clamp(0, nc - 1)[row]
        boxes = loss_boxes(bboxes, img_w, img_h)[row] * fg[..., None]
    else:
        lab, boxes = torch.zeros_like(gt, dtype=torch.int64), torch.zeros(*gt.shape, 4, device=gt.device)
    t_scores = F.one_hot(lab, nc).float() * (score * fg)[..., None]
    return dict(fg=fg, target_gt=gt.long(), target_scores=t_scores, target_bboxes=boxes, weight=score * fg, status=status)


class V8DetectionLoss:
    """`criterion(preds, batch)` as the reference's v8DetectionLoss: `preds` is the list of Detect maps, or a tuple whose [1] is that
    list; `batch` holds batch_idx, cls and bboxes.  Returns (loss * B, loss.detach()), so it can be assigned to `MGAModel.det_criterion`."""

    def __init__(self, nc: int, strides: Sequence[int] = (8, 16, 32), gains: Sequence[float] = (7.5, 0.5, 1.5), topk: int = 10,
                 m_cap: Optional[int] = None):
        self.nc, self.strides, self.gains, self.topk, self.m_cap = int(nc), tuple(int(s) for s in strides), tuple(gains), int(topk), m_cap

    def __call__(self, preds, batch) -> Tuple[torch.Tensor, torch.Tensor]:
        feats = preds[1] if isinstance(preds, tuple) else preds
        return detection_loss(feats, batch["batch_idx"], batch["cls"], batch["bboxes"], nc=self.nc, strides=self.strides,
                              gains=self.gains, topk=self.topk, m_cap=self.m_cap)


class DetLossPlan:
    """The criterion on static buffers, for a captured step: fill `feats`, `batch_idx`, `cls`, `bboxes` and the int32 word `n` (the live
    label rows, <= n_cap), call forward() -- `out` (3) and `items` (3) are written -- then backward(): `g_feats` = dL/dfeats for the
    upstream gradient in `g_out` (3, device memory).  With out=plan.det_loss and g_out=plan.g_det of a slice.SlicePlan the order is
    criterion forward -> SlicePlan.forward -> SlicePlan.backward -> criterion backward, all four in one capture."""

    def __init__(self, shapes, nc, n_cap, m_cap, dtype, out, g_out, strides, gains, topk, device, channels_last=False):
        dev = torch.device(device)
        f32 = torch.float32
        self.device, self.nc, self.strides, self.channels_last = dev, int(nc), tuple(int(s) for s in strides), bool(channels_last)
        self.feats = zero_maps(shapes, nc, dtype, dev, channels_last)
        self.g_feats = zero_maps(shapes, nc, dtype, dev, channels_last)
        self.labels = lab = LabelBuffers(n_cap, dev)
        self.batch_idx, self.cls, self.bboxes, self.n = lab.batch_idx, lab.cls, lab.bboxes, lab.n
        self.g_out = g_out if g_out is not None else torch.ones(3, dtype=f32, device=dev)
        self._st = _DetState(self.feats, self.strides, nc, topk, m_cap, gains, self.batch_idx, self.cls, self.bboxes, self.n, out=out,
                             g_feats=self.g_feats, upstream=self.g_out, flags=plan_maps("DetLossPlan", self.feats, channels_last))
        self.out, self.items, self.status = self._st.out, self._st.items, self._st.status
        self.assign_gt, self.assign_score = self._st.assign_gt, self._st.assign_score

    @classmethod
    def create(cls, shapes, nc: int, *, n_cap: int, m_cap: int, dtype=torch.float32, out=None, g_out=None, strides=(8, 16, 32),
               gains=(7.5, 0.5, 1.5), topk: int = 10, device="cuda", channels_last: bool = False):
        """shapes: per level (B, H, W).  out / g_out: fp32 (3) device tensors to write the loss vector to / read its gradient from.
        channels_last: the plan's `feats` and `g_feats` are torch.channels_last (the layout a channels_last model leaves its Detect maps in)."""
        _lib.load()
        return cls(list(shapes), nc, int(n_cap), int(m_cap), dtype, out, g_out, strides, gains, topk, device, channels_last)

    def set_labels(self, batch_idx, cls, bboxes):
        """Copy a batch's labels into the static buffers and write their count (outside a capture)."""
        self.labels.set(batch_idx, cls, bboxes, "DetLossPlan")

    def forward(self):
        self._st.forward(self.device)

    def backward(self):
        self._st.backward(self.device)

    def check_status(self):
        """Raise if the last forward met an image with more label rows than m_cap (a host read: not inside a capture)."""
        raise_on_status(self.status, "DetLossPlan: an image has more ground truths than m_cap; the loss of that call is NaN")

    def assignment(self):
        return assignment_views(self.assign_gt, self.assign_score, self.status, self.cls, self.bboxes, self.nc,
                                self.feats[0].shape[3] * self.strides[0], self.feats[0].shape[2] * self.strides[0])
