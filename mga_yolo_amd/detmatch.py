"""Detections matched to labels for the validation metrics (include/ext/mgamatch.h): what the reference's validator does with the
post-process's rows image by image on the host -- `_prepare_batch`, `box_iou`, `match_predictions` (ultralytics/models/yolo/detect/val.py:131-271,
ultralytics/engine/validator.py:249-290) -- restated as a parallel rule and run on the device for the whole batch.

The rule: wrong-class pairs have IoU 0; for a detection d let l*(d) be the label with the largest IoU; tp[d, t] is true iff
iou[l*(d), d] >= thr_t and d is the lowest detection index among the detections d' with l*(d') = l*(d) and iou[l*(d'), d'] >= thr_t.  That is
what the reference's sort / unique / unique sequence computes (tests/match_oracle.py states both and compares them).  Equal IoUs of one
detection with two labels of its class go to the lower label row; the reference's order there is that of an unstable sort.

Device tensors go through `mgamatch_run`: two launches, fixed-size outputs, no host synchronisation and no allocation, so the matching can
sit inside a captured graph behind the post-process (`DetMatchPlan` fed by a `DetPostPlan`).  Host tensors take `_host_match`, the same rule
stated in torch ops.

The confusion matrix is the third stage, in a module of its own (detconfusion.py, include/ext/mgaconfusion.h); `ap_per_class` on the
accumulation is the fourth (detap.py, include/ext/mgaap.h).

Not built: the scipy assignment branch of `match_predictions`, rotated boxes, and the
mask and pose matrices `tp_m` / `tp_p`.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._binding import call, fill_match
from .detlabels import LabelBuffers, as_labels, img_wh, label_boxes, pair_iou, plan_dets, rows_per_image, size_m_cap, sized_ws
from .detmaps import raise_on_status


def default_iouv() -> torch.Tensor:
    return torch.linspace(0.5, 0.95, 10)


def _iouv_list(iouv) -> list:
    """The thresholds as the fp32 values the comparison uses, checked as the library checks them."""
    v = default_iouv() if iouv is None else torch.as_tensor(iouv).detach().reshape(-1).cpu()
    v = v.to(torch.float32).tolist()
    if not 1 <= len(v) <= _lib.MATCH_MAX_IOU:
        raise ValueError(f"iouv holds {len(v)} thresholds (1 .. {_lib.MATCH_MAX_IOU})")
    if any(not (b > a) for a, b in zip([0.0] + v[:-1], v)) or not v[-1] <= 1:
        raise ValueError(f"iouv={v} must be strictly ascending in (0, 1]")
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# torch ops (host tensors): the project's own statement of the rule, batched
# ---------------------------------------------------------------------------------------------------------------------------
def _host_match(dets, count, batch_idx, cls, bboxes, img_w: float, img_h: float, iouv, single_cls: bool):
    """The rule in torch ops on the whole batch, in the element type of `dets`.  Returns tp (B, max_det, niou) bool, best_iou (B, max_det),
    best_gt (B, max_det) int32."""
    B, D = dets.shape[:2]
    dt, dev = dets.dtype, dets.device
    T = len(iouv)
    rows, has, _ = rows_per_image(batch_idx, B)
    M = rows.shape[1]
    tp = torch.zeros(B, D, T, dtype=torch.bool, device=dev)
    best_iou = torch.zeros(B, D, dtype=dt, device=dev)
    best_gt = torch.full((B, D), -1, dtype=torch.int32, device=dev)
    if M == 0:
        return tp, best_iou, best_gt
    safe = rows.clamp(min=0)
    lb = label_boxes(bboxes.to(dt), img_w, img_h)[safe]                              # (B, M, 4)
    lc = cls.to(dt)[safe]
    live = torch.arange(D, device=dev)[None] < count.to(torch.int64).clamp(0, D)[:, None]
    dc = dets[..., 5]
    iou = pair_iou(lb, dets[..., :4])                                                # (B, D, M)
    pair = has[:, None, :] & live[:, :, None]
    if not single_cls:
        pair = pair & (lc[:, None, :] == dc[:, :, None])
    iou = torch.where(pair, iou, torch.zeros((), dtype=dt, device=dev))
    best_iou = iou.amax(2)
    slot = (iou == best_iou[..., None]).to(torch.int8).argmax(2)                       # the first, i.e. the lower label row, among equal IoUs
    found = best_iou > 0
    best_gt = torch.where(found, rows.gather(1, slot), torch.full_like(slot, -1)).to(torch.int32)
    thr = torch.tensor(iouv, dtype=torch.float32, device=dev).to(dt)
    q = found[..., None] & (best_iou[..., None] >= thr)                               # (B, D, T)
    d_of = torch.arange(D, device=dev)[None, :, None].expand(B, D, T)
    at_ = slot[..., None].expand(B, D, T)
    owner = torch.full((B, M, T), D, dtype=torch.int64, device=dev)
    owner.scatter_reduce_(1, at_, torch.where(q, d_of, torch.full_like(d_of, D)), "amin")
    tp = q & (owner.gather(1, at_) == d_of)
    return tp, best_iou, best_gt


# ---------------------------------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------------------------------
class _MatchState:
    """The buffers of one matching call and its descriptor."""

    def __init__(self, dets, count, batch_idx, cls, bboxes, n, m_cap, img_w, img_h, iouv, single_cls, acc=None):
        dev = dets.device
        B, D = dets.shape[:2]
        self.tp = torch.empty(B, D, len(iouv), dtype=torch.uint8, device=dev)
        self.best_iou = torch.empty(B, D, dtype=torch.float32, device=dev)
        self.best_gt = torch.empty(B, D, dtype=torch.int32, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.args = (dets, count, batch_idx, cls, bboxes, n, m_cap, img_w, img_h, iouv, _lib.MATCH_SINGLE_CLS if single_cls else 0,
                     self.tp, self.best_iou, self.best_gt, self.status)
        self.desc, self.ws = sized_ws(_lib.MatchDesc(), fill_match, _lib.match_ws_bytes, self.args, dev, acc=acc)

    def run(self, dev):
        call("mgamatch_run", dev, C.byref(self.desc))


def match_detections(dets: torch.Tensor, count: torch.Tensor, batch_idx: torch.Tensor, cls: torch.Tensor, bboxes: torch.Tensor, *, imgsz,
                     iouv=None, single_cls: bool = False, m_cap: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Match a batch's detections to its labels.  `dets` (B, max_det, 6) = x1, y1, x2, y2, conf, cls in pixels and `count` (B), as
    `detect_postprocess` returns them (a negative count is taken as 0 rows; with device `dets`, `count` and the labels are moved to its device); `batch_idx` (N), `cls` (N) or (N, 1), `bboxes` (N, 4) xywh
    normalised: the batch's labels; `imgsz`: (h, w) or an int, what the label boxes are scaled by; `iouv`: the thresholds, None for
    torch.linspace(0.5, 0.95, 10); `single_cls`: every class compares equal.  Returns tp (B, max_det, niou) bool -- false past the count --,
    best_iou (B, max_det) fp32: each detection's largest class-matched IoU, and best_gt (B, max_det) int32: the label row it has it with, -1
    for none.  `m_cap`: the label rows an image may have (at most 256); None sizes it from the labels with one host read, a given value
    reads nothing back (an image with more rows then has tp false and best_iou NaN; DetMatchPlan.check_status)."""
    if dets.dim() != 3 or dets.shape[2] != 6 or count.shape != dets.shape[:1]:
        raise ValueError("match_detections: dets must be (B, max_det, 6) and count (B)")
    thr = _iouv_list(iouv)
    img_w, img_h = img_wh(imgsz)
    dev = dets.device
    b_, c_, x_ = as_labels(batch_idx, cls, bboxes, dev)
    if not dets.is_cuda:
        if any(t.is_cuda for t in (count, batch_idx, cls, bboxes)):
            raise RuntimeError("match_detections: the tensors must all live on the GPU or all on the host")
        d_ = dets if dets.dtype == torch.float64 else dets.float()
        tp, best_iou, best_gt = _host_match(d_, count, b_, c_, x_, img_w, img_h, thr, single_cls)
        return tp, best_iou.float(), best_gt
    st = _MatchState(dets.to(torch.float32).contiguous(), count.to(dev, torch.int32).contiguous(), b_, c_, x_, None,
                     size_m_cap(b_, dets.shape[0]) if m_cap is None else int(m_cap), img_w, img_h, thr, single_cls)
    st.run(dev)
    return st.tp.bool(), st.best_iou, st.best_gt


class DetMatchPlan:
    """The matching on static buffers, for a captured graph: hand it a DetPostPlan's `dets` and `count` (or fill its own), set_labels()
    outside the capture, call run() -- `tp`, `best_iou`, `best_gt` are written and, with rows_cap / tgt_cap given, the batch's rows are
    appended to the run's accumulation on the device -- and read `status` outside the capture (check_status).  stats() reads the accumulation
    back once, in the form DetMetrics.process concatenates.  Nothing is allocated or read back by run()."""

    def __init__(self, dets, count, n_cap, m_cap, img_w, img_h, iouv, single_cls, rows_cap, tgt_cap):
        dev = dets.device
        f32, i32 = torch.float32, torch.int32
        self.device, self.niou = dev, len(iouv)
        self.dets, self.count = dets, count
        self.labels = lab = LabelBuffers(n_cap, dev)                  # a ConfusionPlan(labels=this plan) holds the same object
        self.batch_idx, self.cls, self.bboxes, self.n = lab.batch_idx, lab.cls, lab.bboxes, lab.n
        acc = None
        self._arena = None
        if rows_cap is not None:
            # one buffer, so that stats() is one copy: state, then the 4-byte columns, then the tp bytes
            words = 4 + 3 * rows_cap + 2 * tgt_cap
            self._arena = torch.zeros(4 * words + rows_cap * self.niou, dtype=torch.uint8, device=dev)
            self._cuts = np.cumsum([0, 4, rows_cap, rows_cap, rows_cap, tgt_cap, tgt_cap]) * 4
            w = [self._arena[a:b] for a, b in zip(self._cuts[:-1], self._cuts[1:])]
            self.state = w[0].view(i32)
            acc = (self._arena[4 * words:].view(rows_cap, self.niou), w[1].view(f32), w[2].view(f32), w[3].view(i32), w[4].view(f32),
                   w[5].view(i32), self.state)
            self.rows_cap, self.tgt_cap = rows_cap, tgt_cap
        self._st = _MatchState(dets, count, self.batch_idx, self.cls, self.bboxes, self.n, m_cap, img_w, img_h, iouv, single_cls, acc=acc)
        self.tp, self.best_iou, self.best_gt, self.status = self._st.tp, self._st.best_iou, self._st.best_gt, self._st.status

    @classmethod
    def create(cls, B: int, max_det: int, *, n_cap: int, m_cap: int, imgsz, iouv=None, single_cls: bool = False,
               rows_cap: Optional[int] = None, tgt_cap: Optional[int] = None, dets=None, count=None, device="cuda"):
        """dets / count: a DetPostPlan's own fp32 (B, max_det, 6) and int32 (B) tensors, so that `post.run(); match.run()` is one captured
        chain; buffers of the plan's own otherwise.  rows_cap / tgt_cap: the detection and label rows a validation run may accumulate
        (both or neither; neither: no accumulation, stats() raises)."""
        _lib.load()
        if (rows_cap is None) != (tgt_cap is None):
            raise ValueError("DetMatchPlan: rows_cap and tgt_cap are given together or not at all")
        dev = torch.device(device)
        dets, count = plan_dets("DetMatchPlan", dets, count, B, max_det, dev)
        img_w, img_h = img_wh(imgsz)
        return cls(dets, count, int(n_cap), int(m_cap), img_w, img_h, _iouv_list(iouv), bool(single_cls),
                   None if rows_cap is None else int(rows_cap), None if tgt_cap is None else int(tgt_cap))

    def set_labels(self, batch_idx, cls, bboxes):
        """Copy a batch's labels into the static buffers and write their count (outside a capture)."""
        self.labels.set(batch_idx, cls, bboxes, "DetMatchPlan")

    def run(self):
        self._st.run(self.device)

    def reset(self):
        """Start a validation run: zero the accumulation's counters (outside a capture)."""
        if self._arena is None:
            raise RuntimeError("DetMatchPlan: created without rows_cap / tgt_cap, there is no accumulation")
        self.state.zero_()

    def check_status(self):
        """Raise if the last run met an image with more label rows than m_cap, or an append past rows_cap / tgt_cap (a host read: not
        inside a capture)."""
        raise_on_status(self.status, {1: "DetMatchPlan: an image has more label rows than m_cap; its tp rows are 0 and nothing was appended",
                                      2: "DetMatchPlan: the batch's rows do not fit behind rows_cap / tgt_cap; nothing was appended"})

    @property
    def seen(self) -> int:
        if self._arena is None:
            raise RuntimeError("DetMatchPlan: created without rows_cap / tgt_cap, there is no accumulation")
        return int(self.state[2].item())

    def stats(self) -> Dict[str, np.ndarray]:
        """The run's accumulation in the form DetMetrics.process concatenates -- tp bool (N, niou), conf, pred_cls, target_cls, target_img,
        image after image -- plus seen.  One read-back."""
        if self._arena is None:
            raise RuntimeError("DetMatchPlan: created without rows_cap / tgt_cap, there is no accumulation")
        host = self._arena.cpu().numpy()
        w = [host[a:b] for a, b in zip(self._cuts[:-1], self._cuts[1:])]
        n_rows, n_tgt, seen, _ = (int(v) for v in w[0].view(np.int32))
        rows_tp = host[self._cuts[-1]:].reshape(self.rows_cap, self.niou)
        return assemble_stats(rows_tp[:n_rows], w[1].view(np.float32)[:n_rows], w[2].view(np.float32)[:n_rows], w[3].view(np.int32)[:n_rows],
                              w[4].view(np.float32)[:n_tgt], w[5].view(np.int32)[:n_tgt], seen)


def assemble_stats(rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, seen: int) -> Dict[str, np.ndarray]:
    """Accumulated rows -> the reference's order: image after image by a stable sort on the serial; target_img is each image's unique classes."""
    r, t = np.argsort(rows_img, kind="stable"), np.argsort(tgt_img, kind="stable")
    tgt_cls, tgt_img = tgt_cls[t], tgt_img[t]
    pairs = np.unique(np.stack((tgt_img.astype(np.float64), tgt_cls.astype(np.float64)), 1), axis=0) if tgt_cls.size else np.zeros((0, 2))
    return dict(tp=rows_tp[r].astype(bool), conf=rows_conf[r].copy(), pred_cls=rows_cls[r].copy(), target_cls=tgt_cls.copy(),
                target_img=pairs[:, 1].astype(np.float32), seen=seen)


def host_stats(batches, *, imgsz, iouv=None, single_cls: bool = False) -> Dict[str, np.ndarray]:
    """What a DetMatchPlan accumulates over `batches` (each: dets, count, batch_idx, cls, bboxes), by the host path: the statement
    stats() is tested against."""
    cols = [[] for _ in range(6)]
    seen = 0
    for dets, count, batch_idx, cls, bboxes in batches:
        dets, count = dets.cpu().float(), count.cpu()
        b_, c_, _ = as_labels(batch_idx, cls, bboxes, "cpu")
        tp, _, _ = match_detections(dets, count, batch_idx.cpu(), cls.cpu(), bboxes.cpu(), imgsz=imgsz, iouv=iouv, single_cls=single_cls)
        B, D = dets.shape[:2]
        for b in range(B):
            k = min(max(int(count[b]), 0), D)
            cols[0].append(tp[b, :k].numpy()); cols[1].append(dets[b, :k, 4].numpy())
            cols[2].append(np.zeros(k, np.float32) if single_cls else dets[b, :k, 5].numpy()); cols[3].append(np.full(k, seen + b, np.int32))
        inside = (b_ >= 0) & (b_ < B) & (b_ == b_.floor())
        cols[4].append(c_[inside].numpy()); cols[5].append((b_[inside].to(torch.int32) + seen).numpy())
        seen += B
    return assemble_stats(*(np.concatenate(c, 0) if c else np.zeros(0) for c in cols), seen)


# ---------------------------------------------------------------------------------------------------------------------------
# the validator's update_metrics (install(match=True))
# ---------------------------------------------------------------------------------------------------------------------------
_ORIGINALS: dict = {}          # DetectionValidator class -> the update_metrics install(match=True) replaced on it (install._install_match)
_REPLACED = ("_process_batch", "_prepare_batch", "match_predictions")      # what the replacement stands in for and never calls
_CONFUSION_ON = False          # install(match=True, confusion=True): update_metrics also forms the batch's confusion matrix on the device


def _reference_s(self):
    """(the class install(match=True) rebound update_metrics on, its own update_metrics) for a validator, (None, None) for any other object"""
    for k in type(self).__mro__:
        if k.__dict__.get("update_metrics") is update_metrics:
            return k, _ORIGINALS.get(k)
    return None, None


def update_metrics(self, preds, batch) -> None:
    """DetectionValidator.update_metrics (ultralytics/models/yolo/detect/val.py:173-215) with the matching of the whole batch in one call
    and ONE read-back: the prediction list is padded on the device, the matching runs once with m_cap at its limit (nothing is read to size
    it), tp / conf / cls, the labels and the status word come back in one copy, and the images are walked on the host, feeding
    `self.metrics.update_stats` the per-image dicts the reference builds.  The confusion matrix, pred_to_json and save_one_txt still run per
    image under the reference's conditions -- but the confusion matrix where install(match=True, confusion=True) set the switch, args.plots
    is set, the detections are on the GPU and the validator's ConfusionMatrix is the detection task's, saves no matches (visualize) and has at
    most 119 classes: then one confusion call runs on the same padded batch, its matrix rides in the same read-back and is added to
    `self.confusion_matrix.matrix`, and no per-image process_batch runs (a non-zero status of that call -- a class outside 0 .. nc - 1 --
    leaves the batch to the per-image calls).  `_prepare_pred` runs first, so with args.single_cls the predictions' classes are zeroed and
    compared with the labels' as the reference compares them.
    What it does not cover goes to the reference's own method, the one install() replaced: a validator whose class overrides
    `_process_batch`, `_prepare_batch` or `match_predictions` (the segmentation, pose, OBB and YOLOE validators: masks, keypoints, rotated
    boxes), and a batch in which an image has more than 256 label rows (MGADET_MAX_GT).  Where that method is not known -- the function
    was bound by hand -- those raise NotImplementedError."""
    owner, original = _reference_s(self)
    theirs = [m for m in _REPLACED if owner is not None and getattr(type(self), m, None) is not getattr(owner, m, None)]
    if theirs:
        if original is None:
            raise NotImplementedError(f"update_metrics: {type(self).__name__} has its own {', '.join(theirs)}; only axis-aligned detection is built")
        return original(self, preds, batch)
    preds = [self._prepare_pred(p) for p in preds]
    B = len(preds)
    if B == 0:
        return
    dev = preds[0]["cls"].device
    counts = [int(p["cls"].shape[0]) for p in preds]
    D = max(max(counts), 1)
    dets = torch.zeros(B, D, 6, dtype=torch.float32, device=dev)
    for b, p in enumerate(preds):
        k = counts[b]
        if k:
            dets[b, :k, :4], dets[b, :k, 4], dets[b, :k, 5] = p["bboxes"][:, :4].float(), p["conf"].float(), p["cls"].float()
    count = torch.tensor(counts, dtype=torch.int32, device=dev)
    bi, lc, lx = as_labels(batch["batch_idx"], batch["cls"], batch["bboxes"], dev)
    niou = int(self.iouv.numel())
    imgsz = tuple(batch["img"].shape[2:])
    cmx = getattr(self, "confusion_matrix", None) if _CONFUSION_ON and self.args.plots and dets.is_cuda else None
    if cmx is not None and not (getattr(cmx, "task", None) == "detect" and cmx.matches is None and 1 <= cmx.nc <= _lib.CM_MAX_NC):
        cmx = None
    extra = []
    if dets.is_cuda:
        img_w, img_h = img_wh(imgsz)
        thr = getattr(self, "_mga_iouv", None)                     # the validator's thresholds are read from the device once, not per batch
        if thr is None:
            thr = self._mga_iouv = _iouv_list(self.iouv)
        st = _MatchState(dets, count, bi, lc, lx, None, _lib.DET_MAX_GT, img_w, img_h, thr, False)
        st.run(dev)
        tp, status = st.tp, st.status.float()
        if cmx is not None:
            from .detconfusion import _ConfusionState, reference_conf
            ct = _ConfusionState(dets, count, bi, lc, lx, None, _lib.DET_MAX_GT, cmx.nc, img_w, img_h, reference_conf(self.args.conf), 0.45, False)
            ct.run(dev)
            extra = [ct.status.float(), ct.cm.reshape(-1).float()]             # a batch's counts are far below 2^24: exact in fp32
    else:
        tp, _, _ = match_detections(dets, count, bi, lc, lx, imgsz=imgsz, iouv=self.iouv)
        status = torch.zeros(1)
    packed = torch.cat((status, tp.reshape(-1).float(), dets[..., 4:6].reshape(-1), bi, lc, *extra)).cpu().numpy()     # the one read-back
    if packed[0] != 0:                                             # an image over the limit: nothing was counted yet, and _prepare_pred is idempotent
        if original is None:
            raise NotImplementedError(f"update_metrics: an image has more than {_lib.DET_MAX_GT} label rows")
        return original(self, preds, batch)
    packed = packed[1:]
    cm_h = None
    if extra:
        cells = (cmx.nc + 1) ** 2
        if packed[-cells - 1] == 0:                                # its status; otherwise the per-image calls below take the batch
            cm_h = packed[-cells:].reshape(cmx.nc + 1, cmx.nc + 1)
        packed = packed[:-cells - 1]
    n_tp = B * D * niou
    tp_h = packed[:n_tp].reshape(B, D, niou) != 0
    cc_h = packed[n_tp:n_tp + 2 * B * D].reshape(B, D, 2)
    bi_h, lc_h = packed[n_tp + 2 * B * D:n_tp + 2 * B * D + bi.numel()], packed[n_tp + 2 * B * D + bi.numel():]
    cls_dtype = torch.empty(0, dtype=batch["cls"].dtype).numpy().dtype                                  # what .cpu().numpy() gives the reference
    need_batch = self.args.plots or self.args.save_json or self.args.save_txt
    for si, predn in enumerate(preds):
        self.seen += 1
        k = counts[si]
        cls = lc_h[bi_h == si].astype(cls_dtype)
        no_pred = k == 0
        self.metrics.update_stats({
            "tp": tp_h[si, :k].copy() if not no_pred else np.zeros((0, niou), dtype=bool),
            "target_cls": cls,
            "target_img": np.unique(cls),
            "conf": np.zeros(0) if no_pred else cc_h[si, :k, 0].copy(),
            "pred_cls": np.zeros(0) if no_pred else cc_h[si, :k, 1].copy(),
        })
        pbatch = self._prepare_batch(si, batch) if need_batch else None
        if self.args.plots and cm_h is None:
            self.confusion_matrix.process_batch(predn, pbatch, conf=self.args.conf)
            if self.args.visualize:
                self.confusion_matrix.plot_matches(batch["img"][si], pbatch["im_file"], self.save_dir)
        if no_pred:
            continue
        if self.args.save_json:
            self.pred_to_json(predn, pbatch)
        if self.args.save_txt:
            self.save_one_txt(predn, self.args.save_conf, pbatch["ori_shape"], self.save_dir / "labels" / f"{Path(pbatch['im_file']).stem}.txt")
    if cm_h is not None:
        self.confusion_matrix.matrix += cm_h
