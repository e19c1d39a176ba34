"""The detection post-process of validation and predict (include/mganms.h): Detect decode, candidate selection and greedy non-maximum
suppression on the Detect head's feature maps or on an already decoded prediction, behind the call form of the reference's
`non_max_suppression` (ultralytics/utils/ops.py:192-338) after `Detect._inference` (ultralytics/nn/modules/head.py:150-185).

Device tensors go through `mgamaps_nms_run` (include/ext/mgamaps.h: `mganms_run` with the maps' layout as a flag; maps that are
torch.channels_last on every level are read in place, bit for bit what NCHW maps of the same values give): two launches, fixed-size outputs, no host synchronisation and no allocation, so the post-process can
sit inside a captured graph behind the forward (`DetPostPlan`).  Host tensors take `_host_postprocess`, the same semantics stated in torch
ops.

Two departures from the reference: classes are compared instead of being moved apart by `cls * max_wh` (which rounds the coordinates and
lets very wide boxes meet across classes), and half features are read and everything is computed in fp32.

Not built: the `classes=` filter and `labels=` (autolabelling); `rotated`, `end2end` and extra mask channels (`nc` is taken as `C - 4`);
reg_max other than 16; levels of different layouts in one call (they are made contiguous here).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._binding import call, fill_nms
from .detmaps import REG_MAX, anchor_grid, check_maps, device_maps, kernel_maps, plan_maps, raise_on_status, zero_maps


# ---------------------------------------------------------------------------------------------------------------------------
# torch ops (host tensors): the project's own statement of the post-process
# ---------------------------------------------------------------------------------------------------------------------------
def _decode(feats, strides, nc: int):
    """The Detect maps -> boxes (B, A, 4) xyxy in pixels and probabilities (B, A, nc), in the maps' element type."""
    B = feats[0].shape[0]
    dtype, dev = feats[0].dtype, feats[0].device
    x = torch.cat([f.reshape(B, 4 * REG_MAX + nc, -1) for f in feats], 2)                # (B, no, A)
    A = x.shape[2]
    d = (x[:, :4 * REG_MAX].reshape(B, 4, REG_MAX, A).softmax(2) * torch.arange(REG_MAX, dtype=dtype, device=dev).view(1, 1, -1, 1)).sum(2)
    anc, st = anchor_grid(feats, strides, dtype, dev)
    ax, ay, st = anc[:, 0], anc[:, 1], st[:, 0]
    boxes = torch.stack(((ax - d[:, 0]) * st, (ay - d[:, 1]) * st, (ax + d[:, 2]) * st, (ay + d[:, 3]) * st), -1)
    return boxes, x[:, 4 * REG_MAX:].sigmoid().permute(0, 2, 1)


def _from_pred(pred):
    """A decoded (B, 4 + nc, A) prediction -> boxes (B, A, 4) xyxy (ops.xywh2xyxy) and probabilities (B, A, nc)."""
    cx, cy, w2, h2 = pred[:, 0], pred[:, 1], pred[:, 2] / 2, pred[:, 3] / 2
    return torch.stack((cx - w2, cy - h2, cx + w2, cy + h2), -1), pred[:, 4:].permute(0, 2, 1)


def _greedy(boxes, scores, cls, iou_thres: float, max_det: int, by_class: bool) -> List[int]:
    """Greedy suppression over candidates already in visiting order; returns the positions kept."""
    n = boxes.shape[0]
    alive = torch.ones(n, dtype=torch.bool)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    kept: List[int] = []
    for i in range(n):
        if not alive[i]:
            continue
        kept.append(i)
        if len(kept) == max_det:
            break
        r = boxes[i + 1:]
        iw = (torch.minimum(boxes[i, 2], r[:, 2]) - torch.maximum(boxes[i, 0], r[:, 0])).clamp(min=0)
        ih = (torch.minimum(boxes[i, 3], r[:, 3]) - torch.maximum(boxes[i, 1], r[:, 1])).clamp(min=0)
        inter = iw * ih
        hit = inter / (area[i] + area[i + 1:] - inter) > iou_thres
        if by_class:
            hit &= cls[i + 1:] == cls[i]
        alive[i + 1:] &= ~hit
    return kept


def _host_postprocess(feats, pred, nc: int, strides, conf_thres: float, iou_thres: float, max_det: int, max_nms: int, multi_label: bool,
                      agnostic: bool, lowest_first: bool = True):
    """The post-process in torch ops.  Returns dets (B, max_det, 6), count (B) int32, keep (B, max_det) int32.  lowest_first: equal scores
    are visited lowest candidate index first (the kernels' rule); False: highest first."""
    boxes, prob = _decode(feats, strides, nc) if pred is None else _from_pred(pred)
    boxes, prob = boxes.cpu(), prob.cpu()
    B, A = prob.shape[:2]
    multi = bool(multi_label) and nc > 1
    dets = torch.zeros(B, max_det, 6, dtype=boxes.dtype)
    count = torch.zeros(B, dtype=torch.int32)
    keep = torch.full((B, max_det), -1, dtype=torch.int32)
    for b in range(B):
        if multi:
            a_i, c_i = torch.nonzero(prob[b] > conf_thres, as_tuple=True)                # row-major: anchor first, then class
        else:
            best = prob[b].amax(1)
            c_all = (prob[b] == best[:, None]).to(torch.int8).argmax(1)                  # the lowest class among equal probabilities
            a_i = torch.nonzero(best > conf_thres).flatten()
            c_i = c_all[a_i]
        sc = prob[b][a_i, c_i]
        if not lowest_first:
            a_i, c_i, sc = a_i.flip(0), c_i.flip(0), sc.flip(0)
        order = sc.sort(descending=True, stable=True).indices[:max_nms]
        a_i, c_i, sc = a_i[order], c_i[order], sc[order]
        bx = boxes[b][a_i]
        k = _greedy(bx, sc, c_i, iou_thres, max_det, not agnostic and nc > 1)
        n = len(k)
        if n:
            k = torch.tensor(k)
            dets[b, :n, :4], dets[b, :n, 4], dets[b, :n, 5] = bx[k], sc[k], c_i[k].to(boxes.dtype)
            keep[b, :n] = a_i[k].to(torch.int32)
        count[b] = n
    return dets, count, keep


# ---------------------------------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------------------------------
def _flags(multi_label: bool, agnostic: bool) -> int:
    return (_lib.NMS_MULTI_LABEL if multi_label else 0) | (_lib.NMS_AGNOSTIC if agnostic else 0)


class _PostState:
    """The buffers of one post-process call and its descriptor."""

    def __init__(self, feats, pred, strides, nc, conf_thres, iou_thres, max_det, max_nms, multi_label, agnostic, cand_cap, dets=None, layout=0):
        src = feats[0] if feats is not None else pred
        self.layout = int(layout)                                # 0 or _lib.MAPS_LAYOUT_NHWC: how feats lie in memory
        dev, B = src.device, src.shape[0]
        A = sum(f.shape[2] * f.shape[3] for f in feats) if feats is not None else pred.shape[2]
        if cand_cap is None:
            cand_cap = A * (nc if multi_label and nc > 1 else 1)                         # can never overflow
        i32 = torch.int32
        self.dets = dets if dets is not None else torch.empty(B, max_det, 6, dtype=torch.float32, device=dev)
        self.count = torch.empty(B, dtype=i32, device=dev)
        self.keep = torch.empty(B, max_det, dtype=i32, device=dev)
        self.status = torch.empty(1, dtype=i32, device=dev)
        self.args = (feats, pred, strides, nc, conf_thres, iou_thres, max_det, max_nms, _flags(multi_label, agnostic), cand_cap,
                     self.dets, self.count, self.keep, self.status)
        self.desc = _lib.NmsDesc()
        fill_nms(self.desc, *self.args)
        self.ws = torch.zeros(_lib.nms_ws_bytes(self.desc), dtype=torch.uint8, device=dev)   # zero-filled once: the lists' counters
        fill_nms(self.desc, *self.args, ws=self.ws)

    def run(self, dev):
        call("mgamaps_nms_run", dev, C.byref(self.desc), self.layout)


def _check_args(conf_thres, iou_thres, max_det, max_nms):
    if not 0 <= conf_thres <= 1 or not 0 <= iou_thres <= 1:
        raise ValueError(f"conf_thres={conf_thres} and iou_thres={iou_thres} must lie in [0, 1]")
    if max_det < 1 or max_nms < 1:
        raise ValueError(f"max_det={max_det} and max_nms={max_nms} must be at least 1")


def detect_postprocess(feats, *, nc: int, strides: Sequence[int] = (8, 16, 32), conf_thres: float = 0.25, iou_thres: float = 0.45,
                       max_det: int = 300, max_nms: int = 30000, multi_label: bool = False, agnostic: bool = False,
                       cand_cap: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Decode, candidates and greedy NMS.  `feats`: the Detect maps (level l: (B, 64 + nc, H_l, W_l)), or ONE tensor (B, 4 + nc, A): an
    already decoded prediction, xywh in pixels with probabilities (`strides` is then unused).  Returns dets (B, max_det, 6) fp32 -- the
    kept rows in visiting order as (x1, y1, x2, y2, conf, cls), zeros past the image's count --, count (B) int32 and keep (B, max_det)
    int32: the anchor index of each kept row, -1 past the count.  `cand_cap`: the candidates an image's list holds; None sizes it so that
    it cannot overflow; an image with more candidates gets count -1 and NaN rows (DetPostPlan.check_status)."""
    _check_args(conf_thres, iou_thres, max_det, max_nms)
    pred = None
    if isinstance(feats, torch.Tensor):
        pred, feats = feats, None
        if pred.dim() != 3 or pred.shape[1] != 4 + nc:
            raise ValueError(f"detect_postprocess: a decoded prediction must be (B, {4 + nc}, A)")
        tensors = [pred]
    else:
        feats = list(feats)
        check_maps("detect_postprocess", feats, nc, strides)
        tensors = feats
    if not tensors[0].is_cuda:
        if any(t.is_cuda for t in tensors):
            raise RuntimeError("detect_postprocess: the feature maps must all live on the GPU or all on the host")
        up = lambda t: t if t.dtype == torch.float64 else t.float()
        d, c, k = _host_postprocess(None if feats is None else [up(f) for f in feats], None if pred is None else up(pred), nc, strides,
                                    conf_thres, iou_thres, max_det, max_nms, multi_label, agnostic)
        return d.float(), c, k
    tensors, layout = device_maps(tensors) if feats is not None else (kernel_maps(tensors), 0)
    st = _PostState(tensors if feats is not None else None, tensors[0] if pred is not None else None, tuple(int(s) for s in strides),
                    int(nc), conf_thres, iou_thres, int(max_det), int(max_nms), multi_label, agnostic, cand_cap, layout=layout)
    st.run(tensors[0].device)
    return st.dets, st.count, st.keep


def non_max_suppression(prediction, conf_thres: float = 0.25, iou_thres: float = 0.45, classes=None, agnostic: bool = False,
                        multi_label: bool = False, labels=(), max_det: int = 300, nc: int = 0, max_time_img: float = 0.05,
                        max_nms: int = 30000, max_wh: int = 7680, in_place: bool = True, rotated: bool = False, end2end: bool = False,
                        return_idxs: bool = False):
    """The reference's call form and return type: `prediction` is the decoded (B, 4 + nc, A) tensor or the `(inference_out, loss_out)`
    tuple; returns a list of (n_i, 6) fp32 tensors (x1, y1, x2, y2, conf, cls), with return_idxs also the list of kept anchor indices.
    One read-back, of the counts, to slice.  `prediction` is never written (in_place), nothing is timed (max_time_img), and max_wh is unused:
    classes are compared.  Raises on what is not built: classes=, labels=, rotated, end2end (or an (B, n, 6) end-to-end prediction) and
    extra mask channels (nc other than C - 4)."""
    if isinstance(prediction, (list, tuple)):
        prediction = prediction[0]
    if classes is not None or (labels is not None and len(labels)):
        raise NotImplementedError("non_max_suppression: the classes= filter and labels= (autolabelling) are not built")
    if rotated or end2end or prediction.shape[-1] == 6:
        raise NotImplementedError("non_max_suppression: rotated boxes and end-to-end predictions are not built")
    C_ = prediction.shape[1]
    if nc and nc != C_ - 4:
        raise NotImplementedError(f"non_max_suppression: nc={nc} with {C_} channels: extra mask channels are not built")
    dets, count, keep = detect_postprocess(prediction, nc=C_ - 4, conf_thres=conf_thres, iou_thres=iou_thres, max_det=max_det,
                                           max_nms=max_nms, multi_label=multi_label, agnostic=agnostic)
    counts = count.tolist()                                      # the one read-back
    if any(n < 0 for n in counts):
        raise RuntimeError("non_max_suppression: an image's candidate list overflowed")
    output = [dets[b, :n] for b, n in enumerate(counts)]
    if not return_idxs:
        return output
    return output, [keep[b, :n].long() for b, n in enumerate(counts)]


class DetPostPlan:
    """The post-process on static buffers, for a captured graph: fill `feats` (or hand the plan the forward's own output tensors), call
    run() -- `dets` (B, max_det, 6), `count` (B) and `keep` (B, max_det) are written -- and read `status` outside the capture
    (check_status).  Nothing is allocated or read back by run(), and no buffer has to be cleared between replays."""

    def __init__(self, feats, nc, strides, conf_thres, iou_thres, max_det, max_nms, multi_label, agnostic, cand_cap, dets, channels_last=False):
        self.device, self.nc, self.strides, self.channels_last = feats[0].device, int(nc), tuple(int(s) for s in strides), bool(channels_last)
        self.feats = feats
        self._st = _PostState(feats, None, self.strides, self.nc, conf_thres, iou_thres, int(max_det), int(max_nms), multi_label, agnostic,
                              cand_cap, dets=dets, layout=plan_maps("DetPostPlan", feats, channels_last))
        self.dets, self.count, self.keep, self.status = self._st.dets, self._st.count, self._st.keep, self._st.status

    @classmethod
    def create(cls, shapes, nc: int, *, dtype=torch.float32, strides=(8, 16, 32), conf_thres: float = 0.25, iou_thres: float = 0.45,
               max_det: int = 300, max_nms: int = 30000, multi_label: bool = False, agnostic: bool = False, cand_cap: Optional[int] = None,
               dets=None, feats=None, device="cuda", channels_last: bool = False):
        """shapes: per level (B, H, W).  dets: an fp32 (B, max_det, 6) device tensor to write the rows to; feats: the tensors to read (the
        forward's static outputs) instead of buffers of the plan's own.  channels_last: the maps -- the plan's own or `feats` -- are
        torch.channels_last; `feats` of the other layout raise ValueError (they are read in place on every replay, never copied)."""
        _lib.load()
        _check_args(conf_thres, iou_thres, max_det, max_nms)
        dev = torch.device(device)
        if feats is None:
            feats = zero_maps(shapes, nc, dtype, dev, channels_last)
        return cls(list(feats), nc, strides, conf_thres, iou_thres, max_det, max_nms, multi_label, agnostic, cand_cap, dets, channels_last)

    def run(self):
        self._st.run(self.device)

    def check_status(self):
        """Raise if the last run met an image with more candidates than cand_cap (a host read: not inside a capture)."""
        raise_on_status(self.status, "DetPostPlan: an image has more candidates than cand_cap; its count is -1 and its rows are NaN")
