"""Cases of the detection matching (include/ext/mgamatch.h, csrc/match.cuh): the smallest shapes at which each piece can go wrong.

Two kinds, both numpy.random.RandomState (a frozen stream) and arithmetic only, rounded once to fp32:
  random           labels are placed in the image (freely, or one per cell of a grid where an image has many, so that the pairs with an IoU
                   stay few); a detection is a jittered copy of one of its image's labels, mostly of the label's class, or a box of its own;
                   confidences descend.  A detection is drawn again until every IoU it has with a label of its class is farther than 2 GUARD
                   from every threshold and its two largest are that far apart, so nearly every seed passes the generator's guards.
  by construction  coordinates on a 1/64 grid of a 64 x 64 image: the boxes, their IoUs and the answer are exact in fp32 and known: ANSWERS.

tests/golden/match_<name>.npz (tools/gen_golden_match.py) holds the inputs, the seed the generator accepted, and what the reference's own
validator gave on exactly these values; load() rebuilds the case from the seed and refuses inputs that differ from the stored ones.

Which path of csrc/match.cuh runs where:
  k_match's staging loop, a second chunk of 1024 rows   chunks (1082 rows, every image's on both sides of row 1024, best labels behind it: the carry
                                                        of the rows met so far), dup_far (a label's twin at row 1030: the lower row wins across chunks)
  k_match's detection loop, a second trip of 512        dets600 (counts 600, 513, 512, 257: a second trip of 88 rows with none in its upper half, of one
                                                        row, none, and a first trip with one row in its upper half; owners decided between a
                                                        detection below 512 and one at or above it)
  k_match_append with five label workgroups             chunks through a plan (the GPU tests: the n word at 1024, 1025 and 1030)
  status 1 from rows counted in the second chunk        chunks with m_cap one below an image's rows (the GPU tests)"""
import os

import numpy as np
import torch

import match_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IOUV10 = np.linspace(0.5, 0.95, 10).astype(np.float32)            # what torch.linspace(0.5, 0.95, 10) holds
IOUV16 = np.linspace(0.2, 0.95, 16).astype(np.float32)

# random: counts per image, labels per image, then options.  garbage: rows behind the n word.  extra: label rows of images that do not exist
CASES = {
    "basic": dict(D=16, nc=3, counts=(16, 9, 12), labels=(3, 2, 2), hw=(96, 128), extra=[5], shuffle=True),
    "steal": dict(construct=True),
    "owned": dict(construct=True),
    "wide": dict(D=300, nc=4, counts=(300, 257, 65, 1), labels=(40, 30, 12, 3), hw=(640, 640), grid=8, shuffle=True),
    "labels256": dict(D=300, nc=5, counts=(300, 100, 20), labels=(256, 65, 0), hw=(640, 640), grid=16, shuffle=True),
    "empty": dict(D=8, nc=2, counts=(0, 6, -1), labels=(3, 0, 2), hw=(64, 64)),
    "single_cls": dict(D=12, nc=4, counts=(12, 7), labels=(4, 3), hw=(64, 96), single_cls=True, shuffle=True),
    "dup": dict(construct=True, parity=False),
    "nword": dict(D=10, nc=2, counts=(10, 6), labels=(3, 3), hw=(64, 64), garbage=5),
    "iou1": dict(D=12, nc=2, counts=(12, 8), labels=(3, 4), hw=(64, 64), iouv=IOUV10[:1]),
    "iou16": dict(D=12, nc=2, counts=(12, 8), labels=(3, 4), hw=(64, 64), iouv=IOUV16),
    "wrongcls": dict(construct=True),
    # 1082 label rows in two staging chunks; the images that do not exist hold 32 of them
    "chunks": dict(D=48, nc=4, counts=(48, 33, 20, 7, 0, 48), labels=(200, 190, 180, 170, 160, 150), hw=(640, 640), grid=16,
                   extra=[6, 9, 6, 7] * 8, shuffle=True),
    # `wide` with up to 600 detections an image: two trips of the detection loop
    "dets600": dict(D=600, nc=4, counts=(600, 513, 512, 257), labels=(40, 30, 12, 3), hw=(640, 640), grid=8, shuffle=True),
    # `dup` with its twin labels in two staging chunks (parity=False as for `dup`: the reference's order of equal IoUs is an unstable sort's)
    "dup_far": dict(construct=True, parity=False),
}
NAMES = list(CASES)
PARITY = [n for n in NAMES if CASES[n].get("parity", True)]        # held to the reference's own answer
TWINS = ("dup", "dup_far")                                         # a detection's two largest IoUs are equal by construction
STAGE = 1024                                                       # label rows per staging chunk: kMatchStage * kBlock of csrc/match.cuh
N_WORDS = (STAGE, STAGE + 1, STAGE + 6)                            # `chunks` under an n word on and inside its second chunk
TRIP = 512                                                         # detections per trip of k_match's detection loop: 2 * kBlock


def _px(boxes, size=64.0):
    """xyxy in pixels of a 64 x 64 image -> xywh normalised, exact for coordinates on the 1/64 grid... of halves"""
    b = np.asarray(boxes, np.float64)
    return np.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1) / size


# by construction: labels (class, x1, y1, x2, y2), detections (x1, y1, x2, y2, conf, class), one image of 64 x 64
_CONSTRUCT = {
    # IoUs with the one label: 704 / 1024 = 0.6875 and 992 / 1024 = 0.96875
    "steal": dict(labels=[(0, 8, 8, 40, 40)], dets=[(8, 8, 40, 30, 0.9, 0), (8, 8, 40, 39, 0.8, 0)]),
    # detection 0: 0.9375 with label 0.  detection 1: 832 / 1216 = 0.684 with label 0, 704 / 1344 = 0.524 with label 1
    "owned": dict(labels=[(0, 8, 8, 40, 40), (0, 24, 8, 56, 40)], dets=[(8, 8, 40, 38, 0.9, 0), (14, 8, 46, 40, 0.8, 0)]),
    # rows 1 and 3 are the same label; rows 0 and 2 belong to an image that does not exist
    "dup": dict(labels=[(0, 1, 1, 9, 9), (0, 8, 8, 40, 40), (0, 1, 1, 9, 9), (0, 8, 8, 40, 40)], batch_idx=[7, 0, 7, 0],
                dets=[(8, 8, 40, 30, 0.9, 0)]),
    # 928 / 1024 = 0.90625 with the label of class 0, 736 / 1280 = 0.575 with the label of its own class
    "wrongcls": dict(labels=[(0, 8, 8, 40, 40), (1, 8, 14, 40, 48)], dets=[(8, 8, 40, 37, 0.9, 1)]),
}
# dup's detection; the matched label at flat rows 3 and 1030, every other row a small box of an image that does not exist
_FAR = (3, STAGE + 6)
_CONSTRUCT["dup_far"] = dict(labels=[(0, 8, 8, 40, 40) if r in _FAR else (0, 1, 1, 9, 9) for r in range(_FAR[1] + 1)],
                             batch_idx=[0 if r in _FAR else 7 for r in range(_FAR[1] + 1)], dets=_CONSTRUCT["dup"]["dets"])
_T = lambda n: [i < n for i in range(10)]
# tp rows and best_gt by construction (thresholds 0.5, 0.55, ..., 0.95)
ANSWERS = {
    "steal": dict(tp=[_T(4), [not v for v in _T(4)]], best_gt=[0, 0]),
    "owned": dict(tp=[_T(9), _T(0)], best_gt=[0, 0]),
    "dup": dict(tp=[_T(4)], best_gt=[1]),
    "wrongcls": dict(tp=[_T(2)], best_gt=[1]),
    "dup_far": dict(tp=[_T(4)], best_gt=[_FAR[0]]),
}
# the wrong rule each by-construction case fails (match_oracle.WRONG)
BUILT_AGAINST = {"steal": "highest_iou_owns", "owned": "second_best_allowed", "wrongcls": "class_ignored"}


def _iou_ok(box, cls, lb, lc, thrs, single_cls):
    same = np.ones(len(lc), bool) if single_cls else lc == cls
    if not same.any():
        return True
    iou, _ = O.iou_matrix(lb[same], box[None])
    v = np.sort(iou[:, 0][iou[:, 0] > 0])
    if v.size == 0:
        return True
    return np.abs(v[:, None] - thrs[None, :]).min() > 2 * O.GUARD and (v.size < 2 or v[-1] - v[-2] > 2 * O.GUARD)


def build(name, seed):
    """-> dict of numpy arrays and settings: dets (B, D, 6) fp32, count (B) int32, batch_idx (N) fp32, cls (N, 1) fp32, bboxes (N, 4) fp32, n
    (None or the live rows), hw, iouv fp32, single_cls, m_cap"""
    spec = CASES[name]
    iouv = np.asarray(spec.get("iouv", IOUV10), np.float32)
    if spec.get("construct"):
        c = _CONSTRUCT[name]
        lab = np.array(c["labels"], np.float64)
        dets = np.array(c["dets"], np.float32)[None]
        return dict(dets=dets, count=np.array([dets.shape[1]], np.int32), batch_idx=np.array(c.get("batch_idx", [0] * len(lab)), np.float32),
                    cls=lab[:, :1].astype(np.float32), bboxes=_px(lab[:, 1:]).astype(np.float32), n=None, hw=(64, 64), iouv=iouv, single_cls=False,
                    m_cap=4)
    rs = np.random.RandomState(seed)
    H, W = spec["hw"]
    D, nc, single = spec["D"], spec["nc"], spec.get("single_cls", False)
    B = len(spec["counts"])
    thrs = iouv.astype(np.float64)
    rows = []                                                      # (image, class, xywh normalised)
    dets = np.zeros((B, D, 6), np.float32)
    for b in range(B):
        L = spec["labels"][b]
        if "grid" in spec:                                         # one label per cell
            g = spec["grid"]
            cells = rs.permutation(g * g)[:L]
            cw, ch = W / g, H / g
            w, h = cw * rs.uniform(0.5, 0.8, L), ch * rs.uniform(0.5, 0.8, L)
            cx, cy = (cells % g + 0.5) * cw + rs.uniform(-0.08, 0.08, L) * cw, (cells // g + 0.5) * ch + rs.uniform(-0.08, 0.08, L) * ch
        else:
            w, h = W * rs.uniform(0.15, 0.45, L), H * rs.uniform(0.15, 0.45, L)
            cx, cy = w / 2 + (W - w) * rs.uniform(0, 1, L), h / 2 + (H - h) * rs.uniform(0, 1, L)
        lcls = rs.randint(0, nc, L).astype(np.float64)
        xywh = np.stack((cx / W, cy / H, w / W, h / H), 1).astype(np.float32)
        rows += [(b, lcls[i], xywh[i]) for i in range(L)]
        lb = O.label_boxes(xywh, W, H) if L else np.zeros((0, 4))
        k = spec["counts"][b]
        if k < 0:
            dets[b] = np.nan                                       # as mganms_run leaves an image whose list overflowed
            continue
        conf = np.sort(rs.uniform(0.05, 0.95, k))[::-1]
        for d in range(k):
            while True:
                if L and rs.uniform() < 0.85:
                    l = rs.randint(L)
                    s = rs.choice([0.04, 0.12, 0.3])
                    sz = np.array([lb[l, 2] - lb[l, 0], lb[l, 3] - lb[l, 1]] * 2)
                    box = lb[l] + rs.uniform(-s, s, 4) * sz
                    c = lcls[l] if rs.uniform() < 0.85 else float(rs.randint(nc))
                else:
                    bw, bh = W * rs.uniform(0.1, 0.4), H * rs.uniform(0.1, 0.4)
                    x, y = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
                    box, c = np.array([x, y, x + bw, y + bh]), float(rs.randint(nc))
                box = box.astype(np.float32).astype(np.float64)
                if box[2] > box[0] and box[3] > box[1] and _iou_ok(box, c, lb, lcls, thrs, single):
                    break
            dets[b, d] = (*box, conf[d], c)
    for b in spec.get("extra", []):
        rows.append((b, 0.0, np.array([0.5, 0.5, 0.4, 0.4], np.float32)))
    if spec.get("shuffle"):
        rows = [rows[i] for i in rs.permutation(len(rows))]
    n = None
    if spec.get("garbage"):                                        # rows behind the n word: large boxes of real images and classes
        n = len(rows)
        rows += [(g % B, float(g % nc), np.array([0.5, 0.5, 0.9, 0.9], np.float32)) for g in range(spec["garbage"])]
    return dict(dets=dets, count=np.array(spec["counts"], np.int32), batch_idx=np.array([r[0] for r in rows], np.float32),
                cls=np.array([[r[1]] for r in rows], np.float32).reshape(-1, 1), bboxes=np.array([r[2] for r in rows], np.float32).reshape(-1, 4),
                n=n, hw=(H, W), iouv=iouv, single_cls=single, m_cap=max(max(spec["labels"]), 1))


def built_for(name, c, o):
    """Why the case built from a seed does not hold what it was built for ([]: it does).  o: its oracle."""
    why = []
    tp = o["tp"]
    if name == "basic" and not (np.any(np.diff(c["batch_idx"]) < 0) and np.any(c["batch_idx"] >= len(c["count"]))):
        why.append("the label rows are in order, or none belongs to no image")
    if name in ("basic", "wide", "labels256"):
        # both properties of the rule must show: a detection above a threshold that stays false because a lower one owns its label
        best = o["best_iou"][..., None] >= c["iouv"][None, None, :].astype(np.float64)
        if not np.any(best & ~tp):
            why.append("no detection is refused because its label is owned")
    if name in ("chunks", "dets600"):
        best = o["best_iou"][..., None] >= c["iouv"][None, None, :].astype(np.float64)
    if name == "chunks":
        bi = c["batch_idx"]
        if len(bi) <= STAGE or not all(np.any(bi[:STAGE] == b) and np.any(bi[STAGE:] == b) for b in range(len(c["count"]))):
            why.append(f"an image without label rows on both sides of row {STAGE}")
        if not np.any(o["best_gt"] >= STAGE):
            why.append(f"no detection's best label lies at or behind row {STAGE}")
        if not np.any(best & ~tp):
            why.append("no detection is refused because its label is owned")
    if name == "dets600":
        if not tp[:, TRIP:].any():
            why.append(f"no detection at or above {TRIP} is true")
        if not np.any((best & ~tp)[:, TRIP:]):
            why.append(f"no detection at or above {TRIP} is refused because a lower one owns its label")
    if name == "nword" and c["n"] is None:
        why.append("no n word")
    if name in ("iou1", "iou16") and not (tp.any() and not tp.all()):
        why.append("tp is all of one value")
    return why


def path(name):
    return os.path.join(GOLDEN, f"match_{name}.npz")


_INPUTS = ("dets", "count", "batch_idx", "cls", "bboxes", "iouv")


def load(name):
    """The golden record and the case rebuilt from its seed, checked against the stored inputs: (case, record)"""
    z = np.load(path(name), allow_pickle=False)
    c = build(name, int(z["seed"]))
    for k in _INPUTS:
        assert np.array_equal(c[k], z[k], equal_nan=True), f"{name}: {k} rebuilt from seed {int(z['seed'])} differs from the stored input"
    return c, z


def oracle(name, c=None, **kw):
    c = c if c is not None else load(name)[0]
    return O.oracle(c["dets"], c["count"], c["batch_idx"], c["cls"], c["bboxes"], c["hw"], c["iouv"], single_cls=c["single_cls"], n=c["n"], **kw)


def tensors(c, device="cpu"):
    """dets, count, batch_idx, cls, bboxes of a case as torch tensors (all the label rows, the ones behind the n word included)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t(c["dets"]), t(c["count"]), t(c["batch_idx"]), t(c["cls"]), t(c["bboxes"])


def live(c):
    """the case with the rows behind its n word cut off"""
    if c["n"] is None:
        return c
    return dict(c, batch_idx=c["batch_idx"][:c["n"]], cls=c["cls"][:c["n"]], bboxes=c["bboxes"][:c["n"]], n=None)
