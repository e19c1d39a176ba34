"""The detection post-process of include/mganms.h stated in numpy fp64: Detect decode, candidates, max_nms, greedy suppression.

    oracle(feats=..., strides=..., nc=..., ...)   from the Detect maps        oracle(pred=..., nc=..., ...)   from a decoded prediction

Returns dets (B, max_det, 6), count (B), keep (B, max_det) and `terms` (B, max_det, 6): per coordinate the sum of the magnitudes of every
rounded intermediate on the way to it -- anchor x stride, distance x stride, the coordinate, and the centre and half size of the xywh form the
reference passes through -- and per score the probability; the class column's term is 0 (exact).  An fp32 evaluation, in whatever order, lies
within a few eps_fp32 * terms of this one: bar().  `lowest_first` switches the tie order: equal scores are visited lowest candidate index
first (the kernels' rule) or highest first.  `gaps` holds what the fixture generator's guards look at."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REG = 16
MAX_WH = 7680.0                                # the reference's class offset (ops.py:204)
EPS32 = float(np.finfo(np.float32).eps)


def decode(feats, strides, nc):
    """boxes (B, A, 4) xyxy in pixels, prob (B, A, nc), terms (B, A, 4)."""
    B = feats[0].shape[0]
    x = np.concatenate([np.asarray(f, dtype=np.float64).reshape(B, 4 * REG + nc, -1) for f in feats], 2)
    A = x.shape[2]
    z = x[:, :4 * REG].reshape(B, 4, REG, A)
    e = np.exp(z - z.max(2, keepdims=True))
    d = (e / e.sum(2, keepdims=True) * np.arange(REG, dtype=np.float64).reshape(1, 1, REG, 1)).sum(2)          # (B, 4, A)
    ax, ay, st = [], [], []
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        yy, xx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        ax.append(xx.reshape(-1)); ay.append(yy.reshape(-1)); st.append(np.full(h * w, float(s)))
    ax, ay, st = np.concatenate(ax), np.concatenate(ay), np.concatenate(st)
    boxes = np.stack(((ax - d[:, 0]) * st, (ay - d[:, 1]) * st, (ax + d[:, 2]) * st, (ay + d[:, 3]) * st), -1)
    cx, cy = (boxes[..., 0] + boxes[..., 2]) / 2, (boxes[..., 1] + boxes[..., 3]) / 2
    hw_, hh = (boxes[..., 2] - boxes[..., 0]) / 2, (boxes[..., 3] - boxes[..., 1]) / 2
    anc = np.stack((ax * st, ay * st, ax * st, ay * st), -1)[None]
    dist = np.moveaxis(d, 1, 2) * st[None, :, None]
    xy = np.stack((np.abs(cx) + hw_, np.abs(cy) + hh, np.abs(cx) + hw_, np.abs(cy) + hh), -1)
    terms = anc + dist + np.abs(boxes) + xy
    prob = 1.0 / (1.0 + np.exp(-np.moveaxis(x[:, 4 * REG:], 1, 2)))
    return boxes, prob, terms


def from_pred(pred):
    p = np.asarray(pred, dtype=np.float64)
    cx, cy, w2, h2 = p[:, 0], p[:, 1], p[:, 2] / 2, p[:, 3] / 2
    boxes = np.stack((cx - w2, cy - h2, cx + w2, cy + h2), -1)
    xy = np.stack((np.abs(cx) + np.abs(w2), np.abs(cy) + np.abs(h2)) * 2, -1)
    return boxes, np.moveaxis(p[:, 4:], 1, 2), xy + np.abs(boxes)


def _iou_row(a, r):
    iw = np.clip(np.minimum(a[2], r[:, 2]) - np.maximum(a[0], r[:, 0]), 0, None)
    ih = np.clip(np.minimum(a[3], r[:, 3]) - np.maximum(a[1], r[:, 1]), 0, None)
    inter = iw * ih
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]) - inter)


def greedy(boxes, cls, iou_thres, max_det, by_class, kept_only=True, gaps=None):
    """Candidates in visiting order -> the positions kept.  kept_only=False is the WRONG rule (suppressed by any earlier box over the
    threshold, kept or not): what the `chain` case tells apart.  gaps: a list that receives |IoU - iou_thres| of every compared pair,
    computed on the plain boxes for the pairs that can suppress, and with the reference's class offset for every pair."""
    n = boxes.shape[0]
    alive = np.ones(n, dtype=bool)
    off = boxes + (cls[:, None] * MAX_WH if by_class else 0.0)
    kept = []
    for i in range(n):
        if not alive[i] and kept_only:
            continue
        if alive[i]:
            kept.append(i)
            if len(kept) == max_det:
                break
        iou = _iou_row(boxes[i], boxes[i + 1:])
        can = cls[i + 1:] == cls[i] if by_class else np.ones(n - i - 1, dtype=bool)
        live = alive[i + 1:].copy()
        if gaps is not None and live.any():
            g = np.abs(iou[live & can] - iou_thres)
            g2 = np.abs(_iou_row(off[i], off[i + 1:])[live] - iou_thres)
            gaps.extend([float(np.nanmin(g)) if g.size and not np.all(np.isnan(g)) else 1.0,
                         float(np.nanmin(g2)) if g2.size and not np.all(np.isnan(g2)) else 1.0])
        alive[i + 1:] &= ~((iou > iou_thres) & can)
    return kept


def oracle(feats=None, pred=None, *, nc, strides=(8, 16, 32), conf_thres=0.25, iou_thres=0.45, max_det=300, max_nms=30000,
           multi_label=False, agnostic=False, lowest_first=True, kept_only=True, compare_classes=True):
    """kept_only / compare_classes = False are deliberately wrong variants, for the tests that show which case catches which mistake."""
    boxes, prob, bterms = decode(feats, strides, nc) if pred is None else from_pred(pred)
    B, A = prob.shape[:2]
    multi = bool(multi_label) and nc > 1
    dets, terms = np.zeros((B, max_det, 6)), np.zeros((B, max_det, 6))
    count, keep = np.zeros(B, dtype=np.int64), -np.ones((B, max_det), dtype=np.int64)
    gaps, n_cand = [], []
    for b in range(B):
        if multi:
            a_i, c_i = np.nonzero(prob[b] > conf_thres)
        else:
            c_all = prob[b].argmax(1)                                                    # numpy: the first of equal maxima
            a_i = np.nonzero(prob[b][np.arange(A), c_all] > conf_thres)[0]
            c_i = c_all[a_i]
        sc = prob[b][a_i, c_i]
        n_cand.append(int(a_i.size))
        if not lowest_first:
            a_i, c_i, sc = a_i[::-1], c_i[::-1], sc[::-1]
        order = np.argsort(-sc, kind="stable")[:max_nms]
        a_i, c_i, sc = a_i[order], c_i[order], sc[order]
        k = greedy(boxes[b][a_i], c_i, iou_thres, max_det, (not agnostic) and nc > 1 and compare_classes, kept_only, gaps)
        n = len(k)
        dets[b, :n, :4], dets[b, :n, 4], dets[b, :n, 5] = boxes[b][a_i[k]], sc[k], c_i[k]
        terms[b, :n, :4], terms[b, :n, 4] = bterms[b][a_i[k]], sc[k]
        keep[b, :n], count[b] = a_i[k], n
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(prob - conf_thres) / conf_thres if conf_thres > 0 else np.ones_like(prob)
    return dict(dets=dets, count=count, keep=keep, terms=terms, n_cand=n_cand,
                gaps=dict(conf=float(rel.min()), iou=min(gaps) if gaps else 1.0))


def guards(o):
    """The reasons a case is too close to a decision to define parity on (empty: none): tools/gen_golden_nms.py re-seeds on them."""
    why = []
    if o["gaps"]["conf"] <= 1e-5:
        why.append(f"a probability within {o['gaps']['conf']:.1e} relative of conf_thres")
    if o["gaps"]["iou"] <= 1e-4:
        why.append(f"a compared pair's IoU within {o['gaps']['iou']:.1e} of iou_thres")
    return why


# the bar: |err| <= K eps_fp32 terms, K = twice the largest ratio of the reference's own fp32 run against its fp64 run over the cases
# (tests/golden/nms_ratios.json, written by the generator), and not below 1: two valid orders of the same fp32 roundings differ by up to
# one eps of the terms
K = None
_RATIOS = os.path.join(GOLDEN, "nms_ratios.json")
if os.path.exists(_RATIOS):                                    # absent only while the generator writes it
    with open(_RATIOS) as _f:
        K = max(1.0, 2.0 * json.load(_f)["worst"])


def ratio(got, want, terms):
    """The largest |got - want| / (eps_fp32 terms) over the elements with a term; an element without one must be equal."""
    got, want, terms = (np.asarray(a, dtype=np.float64) for a in (got, want, terms))
    on = terms > 0
    assert np.array_equal(got[~on], want[~on]), "an element without a rounded intermediate differs"
    return float((np.abs(got - want)[on] / (EPS32 * terms[on])).max()) if on.any() else 0.0
