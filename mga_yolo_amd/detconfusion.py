"""The validator's confusion matrix (include/ext/mgaconfusion.h): what the reference's `ConfusionMatrix.process_batch`
(ultralytics/utils/metrics.py:378-456) does image by image on the host -- a `box_iou`, a `torch.where`, a read-back, two argsort / unique
passes and two Python loops -- restated as a parallel rule and run on the device for the whole batch, as the third stage behind
`detect_postprocess` and `match_detections`.

The rule, per image: a detection is counted iff conf > conf_thres; iou[l, d] is `box_iou` between every label and every counted detection,
whatever their classes; a pair qualifies iff iou > iou_thres.  l*(d) is the label with the largest qualifying IoU for d, w(l) the counted
detection with l*(d) = l and the largest iou[l, d]; a detection that loses its l* is not tried against another label.  A label with a
winner counts at [cls(w(l)), cls(l)], one without at [nc, cls(l)], a counted detection that is nobody's winner at [cls(d), nc].  Unlike
the matching's rule it ignores classes, its comparisons are strict, and the highest IoU owns a label, not the lowest detection index
(tests/confusion_oracle.py states the reference's procedure and this rule and compares them).  Equal IoUs of one detection with two labels
go to the lower label row, equal IoUs of two detections claiming one label to the lower detection index; the reference's order there is
that of an unstable sort.

Device tensors go through `mgacm_run`: two launches, fixed-size outputs, no host synchronisation and no allocation, so
`post.run(); match.run(); cm.run()` is one captured chain (`ConfusionPlan(labels=match)`).  Host tensors take `_host_confusion`, the same
rule stated in torch ops.

`ap_per_class` is the stage behind this one (detap.py, include/ext/mgaap.h).

Not built: `plot_matches` / `visualize`, rotated boxes (`batch_probiou`), the classification task's `process_cls_preds`,
more than 119 classes (`_lib.CM_MAX_NC`: the matrix is histogrammed in one workgroup's LDS).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._binding import call, fill_confusion
from .detlabels import LabelBuffers, as_labels, img_wh, label_boxes, pair_iou, plan_dets, rows_per_image, size_m_cap, sized_ws
from .detmaps import raise_on_status
from .detmatch import DetMatchPlan


def reference_conf(conf) -> float:
    """The confidence threshold the reference's process_batch uses for `conf`: 0.25 where the validator's default (None or 0.001) is
    passed (ultralytics/utils/metrics.py:403, axis-aligned boxes)."""
    return 0.25 if conf in {None, 0.001} else float(conf)


def _thresholds(conf, iou_thres) -> Tuple[float, float]:
    """The two thresholds as the fp32 values the comparisons use"""
    c, t = (float(torch.tensor(v, dtype=torch.float32)) for v in (reference_conf(conf), iou_thres))
    if not (c == c and abs(c) != float("inf")):
        raise ValueError(f"conf={conf} must be finite")
    if not 0 <= t < 1:
        raise ValueError(f"iou_thres={iou_thres} must lie in [0, 1)")
    return c, t


# ---------------------------------------------------------------------------------------------------------------------------
# torch ops (host tensors): the project's own statement of the rule, batched
# ---------------------------------------------------------------------------------------------------------------------------
def _host_confusion(dets, count, batch_idx, cls, bboxes, img_w: float, img_h: float, nc: int, conf_thres: float, iou_thres: float,
                    single_cls: bool):
    """The rule in torch ops on the whole batch, in the element type of `dets`.  Returns cm (nc + 1, nc + 1) int64, det_out (B, max_det)
    int32, lab_out (N) int32.  A class outside 0 .. nc - 1 among what is counted raises (the library's status 3)."""
    B, D = dets.shape[:2]
    dt, dev = dets.dtype, dets.device
    N = batch_idx.numel()
    rows, has, belongs = rows_per_image(batch_idx, B)
    live = torch.arange(D, device=dev)[None] < count.to(torch.int64).clamp(0, D)[:, None]
    counted = live & (dets[..., 4] > torch.tensor(conf_thres, dtype=torch.float32).to(dt))
    cm = torch.zeros(nc + 1, nc + 1, dtype=torch.int64, device=dev)
    det_out = torch.full((B, D), -1, dtype=torch.int64, device=dev)
    lab_out = torch.full((N,), -1, dtype=torch.int64, device=dev)
    if single_cls:
        dc, lc_flat = torch.zeros(B, D, dtype=torch.int64, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
    else:
        seen = torch.cat((dets[..., 5][counted].reshape(-1), cls.to(dt)[belongs]))
        if bool((~torch.isfinite(seen)).any()) or bool(((seen.trunc() < 0) | (seen.trunc() > nc - 1)).any()):
            raise ValueError(f"confusion_matrix: a counted detection or a label has a class outside 0 .. {nc - 1}")
        dc = torch.where(counted, dets[..., 5], torch.zeros((), dtype=dt, device=dev)).to(torch.int64)
        lc_flat = torch.where(belongs, cls.to(dt), torch.zeros((), dtype=dt, device=dev)).to(torch.int64)
    det_out[counted] = nc
    M = rows.shape[1]
    if M:
        safe = rows.clamp(min=0)
        iou = pair_iou(label_boxes(bboxes.to(dt), img_w, img_h)[safe], dets[..., :4])                       # (B, D, M)
        qual = has[:, None, :] & counted[:, :, None] & (iou > torch.tensor(iou_thres, dtype=torch.float32).to(dt))
        none = torch.full((), -1, dtype=dt, device=dev)
        iou = torch.where(qual, iou, none)
        best = iou.amax(2)                                                           # (B, D)
        found = best >= 0
        slot = (iou == best[..., None]).to(torch.int8).argmax(2)                     # the first, i.e. the lower label row, among equal IoUs
        claim = torch.where(found[..., None] & (slot[..., None] == torch.arange(M, device=dev)), best[..., None], none)   # (B, D, M)
        top = claim.amax(1)                                                          # (B, M)
        won = top >= 0
        w = (claim == top[:, None, :]).to(torch.int8).argmax(1)                      # the lowest detection among equal IoUs
        d_of = torch.arange(D, device=dev)[None].expand(B, D)
        wins = found & won.gather(1, slot) & (w.gather(1, slot) == d_of)
        lc = lc_flat[safe]                                                           # (B, M)
        det_out = torch.where(wins, lc.gather(1, slot), det_out)
        lab_out[rows[has]] = torch.where(won, dc.gather(1, w), torch.full_like(w, nc))[has]
    got = lab_out >= 0
    cm.index_put_((lab_out[got], lc_flat[got]), torch.ones((), dtype=torch.int64, device=dev), accumulate=True)
    fp = det_out == nc
    cm.index_put_((dc[fp], torch.full_like(dc[fp], nc)), torch.ones((), dtype=torch.int64, device=dev), accumulate=True)
    return cm, det_out.to(torch.int32), lab_out.to(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------------------------------
class _ConfusionState:
    """The buffers of one confusion-matrix call and its descriptor."""

    def __init__(self, dets, count, batch_idx, cls, bboxes, n, m_cap, nc, img_w, img_h, conf_thres, iou_thres, single_cls, acc=None):
        dev = dets.device
        B, D = dets.shape[:2]
        i32 = torch.int32
        self.det_out = torch.empty(B, D, dtype=i32, device=dev)
        self.lab_out = torch.empty(batch_idx.shape[0], dtype=i32, device=dev)
        self.cm = torch.empty(nc + 1, nc + 1, dtype=i32, device=dev)
        self.status = torch.empty(1, dtype=i32, device=dev)
        self.acc = acc
        self.args = (dets, count, batch_idx, cls, bboxes, n, m_cap, nc, _lib.CM_SINGLE_CLS if single_cls else 0, img_w, img_h, conf_thres,
                     iou_thres, self.det_out, self.lab_out, self.cm, acc, self.status)
        self.desc, self.ws = sized_ws(_lib.ConfusionDesc(), fill_confusion, _lib.confusion_ws_bytes, self.args, dev)

    def run(self, dev):
        call("mgacm_run", dev, C.byref(self.desc))


def confusion_matrix(dets: torch.Tensor, count: torch.Tensor, batch_idx: torch.Tensor, cls: torch.Tensor, bboxes: torch.Tensor, *, nc: int,
                     imgsz, conf=0.25, iou_thres: float = 0.45, single_cls: bool = False,
                     m_cap: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The confusion matrix of one batch.  `dets`, `count` and the labels as `match_detections` takes them; `nc`: the number of classes;
    `conf`: the validator's confidence argument, taken through `reference_conf` (None and 0.001 mean 0.25); `iou_thres`: a pair
    qualifies above it; `single_cls`: every class is taken as 0.  Returns cm (nc + 1, nc + 1) int64 indexed [predicted, true] with nc
    meaning background, det_out (B, max_det) int32 -- the class of the label a detection won, nc for a false positive, -1 for a row that is
    not counted -- and lab_out (N) int32 -- the class of a label's winner, nc for a false negative, -1 for a row of no image.  `m_cap`: the
    label rows an image may have (at most 256); None sizes it from the labels with one host read, a given value reads nothing back.  On the
    device an image over m_cap or a class outside 0 .. nc - 1 leaves cm all zeros (ConfusionPlan.check_status names the cause); nc above
    119 is refused there."""
    if dets.dim() != 3 or dets.shape[2] != 6 or count.shape != dets.shape[:1]:
        raise ValueError("confusion_matrix: dets must be (B, max_det, 6) and count (B)")
    if nc < 1:
        raise ValueError(f"confusion_matrix: nc={nc}")
    conf_thres, iou_thres = _thresholds(conf, iou_thres)
    img_w, img_h = img_wh(imgsz)
    dev = dets.device
    b_, c_, x_ = as_labels(batch_idx, cls, bboxes, dev)
    if not dets.is_cuda:
        if any(t.is_cuda for t in (count, batch_idx, cls, bboxes)):
            raise RuntimeError("confusion_matrix: the tensors must all live on the GPU or all on the host")
        d_ = dets if dets.dtype == torch.float64 else dets.float()
        return _host_confusion(d_, count, b_, c_, x_, img_w, img_h, int(nc), conf_thres, iou_thres, single_cls)
    st = _ConfusionState(dets.to(torch.float32).contiguous(), count.to(dev, torch.int32).contiguous(), b_, c_, x_, None,
                         size_m_cap(b_, dets.shape[0]) if m_cap is None else int(m_cap), int(nc), img_w, img_h, conf_thres, iou_thres, single_cls)
    st.run(dev)
    return st.cm.long(), st.det_out, st.lab_out


class ConfusionPlan:
    """The confusion matrix on static buffers, for a captured graph: hand it a DetPostPlan's `dets` and `count` and a DetMatchPlan's labels
    (or fill its own), call run() -- `cm`, `det_out`, `lab_out` are written and, with accumulate, `cm` is added to the run's int64 matrix on
    the device -- and read `status` outside the capture (check_status).  matrix() reads the accumulation back once.  Nothing is allocated
    or read back by run()."""

    def __init__(self, dets, count, labels, n_cap, m_cap, nc, img_w, img_h, conf_thres, iou_thres, single_cls, accumulate):
        dev = dets.device
        self.device, self.nc = dev, nc
        self.dets, self.count = dets, count
        self.labels = lab = labels.labels if labels is not None else LabelBuffers(n_cap, dev)      # the DetMatchPlan's own object, or this plan's
        self.batch_idx, self.cls, self.bboxes, self.n = lab.batch_idx, lab.cls, lab.bboxes, lab.n
        self._who = "ConfusionPlan" if labels is None else "DetMatchPlan"                           # whose buffers set_labels() fills
        self.acc = torch.zeros(nc + 1, nc + 1, dtype=torch.int64, device=dev) if accumulate else None
        self._st = _ConfusionState(dets, count, self.batch_idx, self.cls, self.bboxes, self.n, m_cap, nc, img_w, img_h, conf_thres, iou_thres,
                                   single_cls, acc=self.acc)
        self.cm, self.det_out, self.lab_out, self.status = self._st.cm, self._st.det_out, self._st.lab_out, self._st.status

    @classmethod
    def create(cls, B: int, max_det: int, *, nc: int, n_cap: Optional[int] = None, m_cap: int, imgsz, conf=0.25, iou_thres: float = 0.45,
               single_cls: bool = False, accumulate: bool = True, dets=None, count=None, labels: Optional[DetMatchPlan] = None, device="cuda"):
        """dets / count: a DetPostPlan's own fp32 (B, max_det, 6) and int32 (B) tensors; labels: a DetMatchPlan whose batch_idx, cls,
        bboxes and n tensors this plan shares, so that one set_labels() serves both and `post.run(); match.run(); cm.run()` is one
        captured chain (n_cap is then the DetMatchPlan's); buffers of the plan's own otherwise.  conf is taken through reference_conf."""
        _lib.load()
        dev = torch.device(device)
        if labels is not None:
            dev = labels.device
            if n_cap is not None and int(n_cap) != labels.batch_idx.numel():
                raise ValueError(f"ConfusionPlan: n_cap={n_cap}, the DetMatchPlan holds {labels.batch_idx.numel()} label rows")
            n_cap = labels.batch_idx.numel()
            dets, count = labels.dets if dets is None else dets, labels.count if count is None else count
        elif n_cap is None:
            raise ValueError("ConfusionPlan: n_cap or labels must be given")
        dets, count = plan_dets("ConfusionPlan", dets, count, B, max_det, dev)
        conf_thres, iou_thres = _thresholds(conf, iou_thres)
        img_w, img_h = img_wh(imgsz)
        return cls(dets, count, labels, int(n_cap), int(m_cap), int(nc), img_w, img_h, conf_thres, iou_thres, bool(single_cls), bool(accumulate))

    def set_labels(self, batch_idx, cls, bboxes):
        """Copy a batch's labels into the static buffers and write their count (outside a capture); with labels= it is the DetMatchPlan's."""
        self.labels.set(batch_idx, cls, bboxes, self._who)

    def run(self):
        self._st.run(self.device)

    def reset(self):
        """Start a validation run: zero the accumulated matrix (outside a capture)."""
        if self.acc is None:
            raise RuntimeError("ConfusionPlan: created with accumulate=False, there is no accumulation")
        self.acc.zero_()

    def check_status(self):
        """Raise if the last run counted nothing: an image with more label rows than m_cap, or a class outside 0 .. nc - 1 (a host
        read: not inside a capture)."""
        raise_on_status(self.status, {1: "ConfusionPlan: an image has more label rows than m_cap; cm is zeros and nothing was accumulated",
                                      3: f"ConfusionPlan: a counted detection or a label has a class outside 0 .. {self.nc - 1}; cm is zeros "
                                         "and nothing was accumulated"})

    def matrix(self) -> torch.Tensor:
        """The run's accumulated matrix, (nc + 1, nc + 1) int64 on the host.  One read-back."""
        if self.acc is None:
            raise RuntimeError("ConfusionPlan: created with accumulate=False, there is no accumulation")
        return self.acc.cpu()
