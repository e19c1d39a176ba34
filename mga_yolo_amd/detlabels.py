"""A batch's labels as the criterion (detloss.py), the matching (detmatch.py) and the confusion matrix (detconfusion.py) take them:
`batch_idx` (n), `cls` (n), `bboxes` (n, 4) xywh normalised, the int32 device word `n` of live rows and the capacity `n_cap`, said once
(csrc/labels.cuh: the kernels' side; csrc/detmaps_host.cuh: what a descriptor's labels are refused for).  NOT unified, on purpose:
  * Membership.  The validator's stages take a row for image b iff 0 <= batch_idx < B and batch_idx is integral (`rows_per_image`, `size_m_cap`;
    labels.cuh: labels_has_image).  The criterion truncates (`batch_idx.to(int64) == b`: `rows_per_image(integral=False)`) and `detection_loss`
    sizes m_cap with out-of-range rows clamped into [0, B - 1]: a different m_cap changes k_det_resolve's entry count E = m_cap * 16 and with it
    the order of its float sum, so that sizing line stays the criterion's own.
  * The box.  `label_boxes` (the validator's) and `loss_boxes` (the criterion's) round differently; each is pinned by its stored results.
  * Ties.  Which of two equal IoUs wins is the matching's and the confusion matrix's own rule, stated where each applies it.
"""
import torch


def img_wh(imgsz):
    """(h, w) or an int -> (img_w, img_h): what the label boxes are scaled by"""
    if isinstance(imgsz, (int, float)):
        return float(imgsz), float(imgsz)
    h, w = imgsz
    return float(w), float(h)


def as_labels(batch_idx, cls, bboxes, device):
    """The labels as every path reads them: flat fp32 batch_idx (n), cls (n) and bboxes (n, 4), contiguous on `device`."""
    f32 = torch.float32
    return (batch_idx.reshape(-1).to(device, f32).contiguous(), cls.reshape(-1).to(device, f32).contiguous(),
            bboxes.reshape(-1, 4).to(device, f32).contiguous())


class LabelBuffers:
    """A static plan's labels: zeroed fp32 batch_idx (n_cap), cls (n_cap), bboxes (n_cap, 4) and the int32 word n the kernels read."""

    def __init__(self, n_cap: int, device):
        self.batch_idx, self.cls = (torch.zeros(n_cap, dtype=torch.float32, device=device) for _ in range(2))
        self.bboxes = torch.zeros(n_cap, 4, dtype=torch.float32, device=device)
        self.n = torch.zeros(1, dtype=torch.int32, device=device)

    def set(self, batch_idx, cls, bboxes, who: str) -> None:
        """Copy a batch's labels into the buffers and write their count (outside a capture)."""
        n = batch_idx.numel()
        if n > self.batch_idx.numel():
            raise ValueError(f"{who}: {n} label rows, the plan holds {self.batch_idx.numel()}")
        self.batch_idx[:n].copy_(batch_idx.reshape(-1)); self.cls[:n].copy_(cls.reshape(-1)); self.bboxes[:n].copy_(bboxes.reshape(-1, 4))
        self.n.fill_(n)


def size_m_cap(batch_idx, B: int) -> int:
    """m_cap for the matching and the confusion matrix where the caller gives none: the most rows an image has (one host read), at least 1."""
    inside = batch_idx[(batch_idx >= 0) & (batch_idx < B)].long()
    return max(int(torch.bincount(inside).max()) if inside.numel() else 1, 1)


def plan_dets(who: str, dets, count, B: int, max_det: int, device):
    """A plan's detection rows, its own where none are handed in: read in place on every replay, so they must be what the kernels take."""
    dets = torch.zeros(B, max_det, 6, dtype=torch.float32, device=device) if dets is None else dets
    count = torch.zeros(B, dtype=torch.int32, device=device) if count is None else count
    if tuple(dets.shape) != (B, max_det, 6) or dets.dtype != torch.float32 or not dets.is_contiguous() or tuple(count.shape) != (B,) \
            or count.dtype != torch.int32:
        raise ValueError(f"{who}: dets must be a contiguous fp32 ({B}, {max_det}, 6) tensor and count int32 ({B})")
    return dets, count


def sized_ws(desc, fill, ws_bytes, args, device, **kw):
    """A descriptor's two passes: filled without ws to ask the library for its size, then again with the ws allocated here.  (desc, ws)"""
    fill(desc, *args, **kw)
    ws = torch.empty(ws_bytes(desc), dtype=torch.uint8, device=device)
    fill(desc, *args, ws=ws, **kw)
    return desc, ws


def label_boxes(bboxes, img_w: float, img_h: float):
    """xywh normalised -> xyxy in pixels as the reference's validator forms it: (c -+ s / 2) * size (ops.xywh2xyxy, then the scale)."""
    half = bboxes[:, 2:] / 2
    size = torch.tensor([img_w, img_h, img_w, img_h], dtype=bboxes.dtype, device=bboxes.device)
    return torch.cat((bboxes[:, :2] - half, bboxes[:, :2] + half), 1) * size


def loss_boxes(bboxes, img_w: float, img_h: float):
    """The same as the reference's criterion forms it: the row scaled by (W, H, W, H), then centre -+ half the size (utils/loss.py:231)."""
    xywh = bboxes * torch.tensor([img_w, img_h, img_w, img_h], dtype=bboxes.dtype, device=bboxes.device)
    half = xywh[..., 2:] / 2
    return torch.cat((xywh[..., :2] - half, xywh[..., :2] + half), -1)


def rows_per_image(batch_idx, B: int, integral: bool = True):
    """Per image its label rows in flat order: rows (B, M) int64, -1 past an image's own (M: the most rows an image has, 0 for none at all),
    has = rows >= 0, and belongs (n): the rows that are some image's -- 0 <= batch_idx < B and integral (a NaN is nobody's); with
    integral=False the criterion's rule: batch_idx truncated toward zero lies in 0 .. B - 1."""
    idx = batch_idx.to(torch.int64)
    belongs = (batch_idx >= 0) & (batch_idx < B) & (batch_idx == idx) if integral else (idx >= 0) & (idx < B)
    per = torch.bincount(idx[belongs], minlength=B) if bool(belongs.any()) else torch.zeros(B, dtype=torch.int64, device=batch_idx.device)
    rows = torch.full((B, int(per.max())), -1, dtype=torch.int64, device=batch_idx.device)
    for b in range(B):
        r = torch.nonzero(belongs & (idx == b)).flatten()
        rows[b, :r.numel()] = r
    return rows, rows >= 0, belongs


def pair_iou(lb, db):
    """The reference's box_iou (ultralytics/utils/metrics.py:53-74), an image's labels lb (B, M, 4) x its detections db (B, D, 4): (B, D, M)"""
    iw = (torch.minimum(lb[:, None, :, 2], db[:, :, None, 2]) - torch.maximum(lb[:, None, :, 0], db[:, :, None, 0])).clamp(min=0)
    ih = (torch.minimum(lb[:, None, :, 3], db[:, :, None, 3]) - torch.maximum(lb[:, None, :, 1], db[:, :, None, 1])).clamp(min=0)
    inter = iw * ih
    area_l = (lb[..., 2] - lb[..., 0]) * (lb[..., 3] - lb[..., 1])
    area_d = (db[..., 2] - db[..., 0]) * (db[..., 3] - db[..., 1])
    return inter / (area_l[:, None, :] + area_d[:, :, None] - inter + 1e-7)
