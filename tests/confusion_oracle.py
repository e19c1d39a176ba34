"""The fp64 oracle of the confusion matrix (include/ext/mgaconfusion.h, mga_yolo_amd/detconfusion.py), in numpy, on one batch.

Two statements on a label x counted-detection IoU matrix of one image (classes ignored, `iou > thr` strictly):
  procedure   the reference's host procedure, stated literally: take the pairs with iou > thr; order them by descending IoU; keep each
              detection's first pair; order again; keep each label's first pair.  A label kept counts at [cls(d), cls(l)], every other label
              at [nc, cls(l)], every detection not kept at [cls(d), nc].
  rule        l*(d): the label with the largest qualifying IoU; w(l): among the detections with l*(d) = l the one with the largest IoU.
They agree wherever a detection's qualifying IoUs are distinct and a label's claimants' IoUs are distinct; on equal IoUs `rule` takes the
lower label row / the lower detection index and `procedure` whatever an unstable sort leaves first.  Five deliberately wrong variants of
`rule` exist so that the tests can show each by-construction case fails the rule it was built against.

oracle() also gives the guards a fixture must pass: no IoU within GUARD of iou_thres, no detection's two largest qualifying IoUs and no
label's two largest claimants' IoUs within GUARD of each other.  Under them every comparison with the device is exact equality of integers.
"""
import numpy as np

import match_oracle as O

GUARD = O.GUARD
WRONG = ("lowest_index_owns", "second_best_allowed", "class_matched", "ge", "filter_after_matching")


def procedure(iou, thr, lcls, dcls, nc):
    """The host procedure on one image.  iou (L, D) over the counted detections; lcls (L), dcls (D) ints.  Returns (matrix, lab (L): the
    class counted for the label's row or nc, det (D): the class of the label the detection is kept with, or nc)."""
    L, D = iou.shape
    mat = np.zeros((nc + 1, nc + 1), np.int64)
    lab, det = np.full(L, nc, np.int64), np.full(D, nc, np.int64)
    li, di = np.nonzero(iou > thr)
    if li.size:
        m = np.stack((li.astype(np.float64), di.astype(np.float64), iou[li, di]), 1)
        if li.size > 1:
            m = m[m[:, 2].argsort()[::-1]]
            m = m[np.unique(m[:, 1], return_index=True)[1]]
            m = m[m[:, 2].argsort()[::-1]]
            m = m[np.unique(m[:, 0], return_index=True)[1]]
    else:
        m = np.zeros((0, 3))
    m0, m1 = m[:, 0].astype(int), m[:, 1].astype(int)
    for i, gc in enumerate(lcls):
        j = m0 == i
        if j.sum() == 1:
            d = int(m1[j][0])
            mat[dcls[d], gc] += 1
            lab[i], det[d] = dcls[d], gc
        else:
            mat[nc, gc] += 1
    for i, dc in enumerate(dcls):
        if not np.any(m1 == i):
            mat[dc, nc] += 1
    return mat, lab, det


def rule(iou, thr, lcls, dcls, nc, wrong=None, counted=None):
    """The parallel rule on one image, same arguments and results as procedure().  wrong: None or one of WRONG; counted (D) bool is read
    by filter_after_matching only, under which `iou` holds every live detection."""
    L, D = iou.shape
    q = iou >= thr if wrong == "ge" else iou > thr
    if wrong == "class_matched":
        q = q & (np.asarray(lcls)[:, None] == np.asarray(dcls)[None, :])
    v = np.where(q, iou, -1.0)
    lstar = np.where(v.max(0) >= 0, v.argmax(0), -1) if L else np.full(D, -1)        # argmax: the first, i.e. lowest, row among equals
    win = np.full(L, -1)
    if wrong == "second_best_allowed":                                                # greedy over the pairs by descending IoU
        taken = set()
        for k in np.argsort(-v, axis=None, kind="stable"):
            l, d = divmod(int(k), D)
            if v[l, d] >= 0 and win[l] < 0 and d not in taken:
                win[l] = d
                taken.add(d)
    else:
        for l in range(L):
            cand = [d for d in range(D) if lstar[d] == l]
            if cand:
                win[l] = min(cand) if wrong == "lowest_index_owns" else max(cand, key=lambda d: (iou[l, d], -d))
    keep = np.ones(D, bool) if counted is None else np.asarray(counted, bool)
    mat = np.zeros((nc + 1, nc + 1), np.int64)
    lab, det = np.full(L, nc, np.int64), np.full(D, nc, np.int64)
    for l in range(L):
        if win[l] >= 0 and keep[win[l]]:
            lab[l], det[win[l]] = dcls[win[l]], lcls[l]
        mat[lab[l], lcls[l]] += 1
    for d in range(D):
        if keep[d] and det[d] == nc:
            mat[dcls[d], nc] += 1
    det[~keep] = -1
    return mat, lab, det


def oracle(dets, count, batch_idx, cls, bboxes, imgsz, nc, conf_thres, iou_thres, single_cls=False, n=None, wrong=None, use_procedure=False,
           round32=False):
    """One batch.  dets (B, D, 6), count (B), labels as the descriptor takes them, imgsz (h, w); conf_thres and iou_thres are taken as
    the fp32 values the comparisons use.  round32: the IoUs rounded to fp32 (the cases by construction, whose fp32 evaluation is exact).
    Returns dict(cm, per_image (B, nc + 1, nc + 1), det_out (B, D), lab_out (N), guards [str], claims: the most detections claiming one
    label, offdiag: the counts in class cells off the diagonal)."""
    dets64 = np.asarray(dets, np.float64)
    B, D = dets64.shape[:2]
    ct, it = float(np.float32(conf_thres)), float(np.float32(iou_thres))
    bi = np.asarray(batch_idx, np.float64).reshape(-1)
    N = bi.size
    n = N if n is None else min(max(int(n), 0), N)
    lb_all = O.label_boxes(np.asarray(bboxes).reshape(-1, 4), imgsz[1], imgsz[0])
    lc_all = np.zeros(N, np.int64) if single_cls else np.trunc(np.nan_to_num(np.asarray(cls, np.float64).reshape(-1))).astype(np.int64)
    out = dict(cm=np.zeros((nc + 1, nc + 1), np.int64), per_image=np.zeros((B, nc + 1, nc + 1), np.int64), det_out=np.full((B, D), -1, np.int64),
               lab_out=np.full(N, -1, np.int64), guards=[], claims=0, offdiag=0)
    for b in range(B):
        rows = np.nonzero(bi[:n] == b)[0]
        k = min(max(int(count[b]), 0), D)
        conf = dets64[b, :k, 4]
        counted = conf >= ct if wrong == "ge" else conf > ct                          # a NaN is not counted
        use = np.ones(k, bool) if wrong == "filter_after_matching" else counted
        di = np.nonzero(use)[0]
        dcls = np.zeros(di.size, np.int64) if single_cls else np.trunc(dets64[b, di, 5]).astype(np.int64)
        lcls = lc_all[rows]
        iou = O.iou_matrix(lb_all[rows], dets64[b, di, :4])[0] if rows.size and di.size else np.zeros((rows.size, di.size))
        if round32:
            iou = iou.astype(np.float32).astype(np.float64)
        if use_procedure:
            mat, lab, det = procedure(iou, it, lcls, dcls, nc)
        else:
            mat, lab, det = rule(iou, it, lcls, dcls, nc, wrong, counted[di] if wrong == "filter_after_matching" else None)
        out["per_image"][b] = mat
        out["lab_out"][rows] = lab
        out["det_out"][b, di] = det
        if iou.size:
            if not round32 and np.abs(iou[iou > 0] - it).min(initial=1.0) <= GUARD:
                out["guards"].append(f"image {b}: a pair's IoU lies within {GUARD} of iou_thres")
            v = np.where(iou > it, iou, -1.0)
            if iou.shape[0] > 1:
                top = np.sort(v, 0)[-2:]
                if np.where(top[0] >= 0, top[1] - top[0], 1.0).min() <= GUARD:
                    out["guards"].append(f"image {b}: a detection's two largest qualifying IoUs lie within {GUARD}")
            lstar = np.where(v.max(0) >= 0, v.argmax(0), -1)
            for l in range(iou.shape[0]):
                c = np.sort(iou[l, lstar == l])
                out["claims"] = max(out["claims"], c.size)
                if c.size > 1 and c[-1] - c[-2] <= GUARD:
                    out["guards"].append(f"image {b}: a label's two largest claimants' IoUs lie within {GUARD}")
    out["cm"] = out["per_image"].sum(0)
    cells = out["cm"][:nc, :nc]
    out["offdiag"] = int(cells.sum() - np.trace(cells))
    return out
