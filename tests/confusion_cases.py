"""Cases of the confusion matrix (include/ext/mgaconfusion.h, csrc/confusion.cuh): the smallest shapes at which each piece can go wrong.

Two kinds, both numpy.random.RandomState (a frozen stream) and arithmetic only, rounded once to fp32:
  random           labels are placed in the image (freely, or one per cell of a grid where an image has many); a detection is a jittered
                   copy of one of its image's labels, of the label's class or -- one time in three -- of another, or a box of its own;
                   confidences are NOT sorted and straddle conf_thres.  A detection is drawn again until every IoU it has with a label is
                   farther than 2 GUARD from iou_thres and its two largest are that far apart.
  by construction  coordinates on a 1/64 grid of a 64 x 64 image: the boxes, their IoUs and the answer are exact in fp32 and known: ANSWERS.

tests/golden/confusion_<name>.npz (tools/gen_golden_confusion.py) holds the inputs, the seed the generator accepted, and the matrices the
reference's own ConfusionMatrix.process_batch gave on exactly these values, one fresh matrix per image; load() rebuilds the case from the
seed and refuses inputs that differ from the stored ones.

Which path of csrc/confusion.cuh runs where:
  k_cm_match's staging loop, a second chunk of 1024 rows    chunks (1082 rows, every image's on both sides of row 1024), twins_far (a label's twin at row 1030)
  k_cm_match's detection loop, a second trip of 512         dets600 (counts 600, 513, 512, 257; a label's winner decided between a detection below 512 and one
                                                            at or above it)
  k_cm_count's last rows and columns of LDS cells           nc119 (classes 118 and 117 among labels and detections)
  status 1 from rows counted in the second chunk            chunks with m_cap one below an image's rows (the GPU tests)"""
import os

import numpy as np
import torch

import confusion_oracle as CO
import match_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAGE = 1024                                                       # label rows per staging chunk: kMatchStage * kBlock of csrc/match_common.cuh
N_WORDS = (STAGE, STAGE + 1, STAGE + 6)                            # `chunks` under an n word on and inside its second chunk
TRIP = 512                                                         # detections per trip of k_cm_match's detection loop: 2 * kBlock

# random: counts per image, labels per image, then options.  conf: the validator's argument (0.001 stands for 0.25, as None does)
CASES = {
    "basic": dict(D=16, nc=3, counts=(16, 9, 12), labels=(3, 2, 2), hw=(96, 128), extra=[5], shuffle=True, conf=0.001),
    "best_iou_wins": dict(construct=True),
    "loser_not_rematched": dict(construct=True),
    "wrongcls": dict(construct=True),
    "on_threshold": dict(construct=True),
    "lowconf_blocks_nothing": dict(construct=True),
    "twins": dict(construct=True, parity=False),
    "twins_far": dict(construct=True, parity=False),
    # labels and no rows; an overflowed image (count -1, NaN rows); detections and no labels; every detection below conf_thres
    "empty": dict(D=8, nc=2, counts=(0, -1, 6, 5), labels=(3, 2, 0, 2), hw=(64, 64), lowconf=(3,), conf=0.25),
    "nword": dict(D=10, nc=2, counts=(10, 6), labels=(3, 3), hw=(64, 64), garbage=5, conf=0.3),
    "single_cls": dict(D=12, nc=4, counts=(12, 7), labels=(4, 3), hw=(64, 96), single_cls=True, shuffle=True, conf=0.001),
    "nc1": dict(D=12, nc=1, counts=(12, 8), labels=(4, 3), hw=(64, 64), conf=0.25),
    "nc80": dict(D=24, nc=80, counts=(24, 17), labels=(8, 6), hw=(128, 128), shuffle=True, conf=0.001),
    "nc119": dict(D=24, nc=119, counts=(24, 17), labels=(8, 6), hw=(128, 128), shuffle=True, conf=0.25, pool=(118, 117, 0, 60)),
    "labels256": dict(D=300, nc=5, counts=(300, 100, 20), labels=(256, 65, 0), hw=(640, 640), grid=16, shuffle=True, conf=0.25),
    # 1082 label rows in two staging chunks; the images that do not exist hold 32 of them
    "chunks": dict(D=48, nc=4, counts=(48, 33, 20, 7, 0, 48), labels=(200, 190, 180, 170, 160, 150), hw=(640, 640), grid=16,
                   extra=[6, 9, 6, 7] * 8, shuffle=True, conf=0.001),
    "dets600": dict(D=600, nc=4, counts=(600, 513, 512, 257), labels=(40, 30, 12, 3), hw=(640, 640), grid=8, shuffle=True, conf=0.25),
}
NAMES = list(CASES)
PARITY = [n for n in NAMES if CASES[n].get("parity", True)]        # held to the reference's own answer
TWINS = ("twins", "twins_far")                                     # equal IoUs by construction
IOU_THRES = 0.45


def _px(boxes, size=64.0):
    """xyxy in pixels of a 64 x 64 image -> xywh normalised, exact for coordinates on the 1/64 grid"""
    b = np.asarray(boxes, np.float64)
    return np.stack(((b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]), 1) / size


# by construction: labels (class, x1, y1, x2, y2), detections (x1, y1, x2, y2, conf, class), one image of 64 x 64, nc = 2, conf_thres 0.25
_CONSTRUCT = {
    # IoUs with the one label: 704 / 1024 = 0.6875 and 992 / 1024 = 0.96875: the later detection, of class 1, owns it
    "best_iou_wins": dict(labels=[(0, 8, 8, 40, 40)], dets=[(8, 8, 40, 30, 0.9, 0), (8, 8, 40, 39, 0.8, 1)]),
    # detection 0: 0.9375 with label 0, 480 / 1504 with label 1.  detection 1: 832 / 1216 = 0.684 with label 0, 704 / 1344 = 0.524 with label 1
    "loser_not_rematched": dict(labels=[(0, 8, 8, 40, 40), (0, 24, 8, 56, 40)], dets=[(8, 8, 40, 38, 0.9, 0), (14, 8, 46, 40, 0.8, 0)]),
    # 928 / 1024 = 0.90625 between a class-1 detection and a class-0 label
    "wrongcls": dict(labels=[(0, 8, 8, 40, 40)], dets=[(8, 8, 40, 37, 0.9, 1)]),
    # 50 / (100 + 50 - 50 + 1e-7) is 0.5 exactly in fp32, iou_thres is 0.5; the second detection is its label's box with conf = conf_thres
    "on_threshold": dict(labels=[(0, 0, 0, 10, 10), (1, 32, 32, 48, 48)], dets=[(0, 0, 10, 5, 0.9, 0), (32, 32, 48, 48, 0.25, 1)], iou_thres=0.5),
    # the label's best claimant (0.96875) is not counted: the other (0.6875) wins
    "lowconf_blocks_nothing": dict(labels=[(0, 8, 8, 40, 40)], dets=[(8, 8, 40, 30, 0.9, 0), (8, 8, 40, 39, 0.1, 0)]),
    # rows 1 and 3 are the same label, the two detections the same box; rows 0 and 2 belong to an image that does not exist
    "twins": dict(labels=[(0, 1, 1, 9, 9), (0, 8, 8, 40, 40), (0, 1, 1, 9, 9), (0, 8, 8, 40, 40)], batch_idx=[7, 0, 7, 0],
                  dets=[(8, 8, 40, 30, 0.9, 0), (8, 8, 40, 30, 0.8, 0)]),
}
_FAR = (3, STAGE + 6)
_CONSTRUCT["twins_far"] = dict(labels=[(0, 8, 8, 40, 40) if r in _FAR else (0, 1, 1, 9, 9) for r in range(_FAR[1] + 1)],
                               batch_idx=[0 if r in _FAR else 7 for r in range(_FAR[1] + 1)], dets=_CONSTRUCT["twins"]["dets"])
# by construction: the non-zero cells [predicted, true] of the 3 x 3 matrix, det_out, and lab_out of the image's rows in flat order
ANSWERS = {
    "best_iou_wins": dict(cells={(1, 0): 1, (0, 2): 1}, det_out=[2, 0], lab_out=[1]),
    "loser_not_rematched": dict(cells={(0, 0): 1, (2, 0): 1, (0, 2): 1}, det_out=[0, 2], lab_out=[0, 2]),
    "wrongcls": dict(cells={(1, 0): 1}, det_out=[0], lab_out=[1]),
    "on_threshold": dict(cells={(2, 0): 1, (0, 2): 1, (2, 1): 1}, det_out=[2, -1], lab_out=[2, 2]),
    "lowconf_blocks_nothing": dict(cells={(0, 0): 1}, det_out=[0, -1], lab_out=[0]),
    "twins": dict(cells={(0, 0): 1, (2, 0): 1, (0, 2): 1}, det_out=[0, 2], lab_out=[0, 2]),
    "twins_far": dict(cells={(0, 0): 1, (2, 0): 1, (0, 2): 1}, det_out=[0, 2], lab_out=[0, 2]),
}
# the wrong rule each by-construction case fails (confusion_oracle.WRONG)
BUILT_AGAINST = {"best_iou_wins": "lowest_index_owns", "loser_not_rematched": "second_best_allowed", "wrongcls": "class_matched",
                 "on_threshold": "ge", "lowconf_blocks_nothing": "filter_after_matching"}


def answer_matrix(name, nc=2):
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for (p, t), v in ANSWERS[name]["cells"].items():
        m[p, t] = v
    return m


def _iou_ok(box, lb, thr):
    if not len(lb):
        return True
    v = np.sort(O.iou_matrix(lb, box[None])[0][:, 0])
    v = v[v > 0]
    if v.size == 0:
        return True
    return np.abs(v - thr).min() > 2 * O.GUARD and (v.size < 2 or v[-1] - v[-2] > 2 * O.GUARD)


def build(name, seed):
    """-> dict of numpy arrays and settings: dets (B, D, 6) fp32, count (B) int32, batch_idx (N) fp32, cls (N, 1) fp32, bboxes (N, 4) fp32, n
    (None or the live rows), hw, nc, conf (the validator's argument), iou_thres, single_cls, m_cap, construct"""
    spec = CASES[name]
    if spec.get("construct"):
        c = _CONSTRUCT[name]
        lab = np.array(c["labels"], np.float64)
        dets = np.array(c["dets"], np.float32)[None]
        return dict(dets=dets, count=np.array([dets.shape[1]], np.int32), batch_idx=np.array(c.get("batch_idx", [0] * len(lab)), np.float32),
                    cls=lab[:, :1].astype(np.float32), bboxes=_px(lab[:, 1:]).astype(np.float32), n=None, hw=(64, 64), nc=2, conf=0.25,
                    iou_thres=c.get("iou_thres", IOU_THRES), single_cls=False, m_cap=4, construct=True)
    rs = np.random.RandomState(seed)
    H, W = spec["hw"]
    D, nc, single = spec["D"], spec["nc"], spec.get("single_cls", False)
    B = len(spec["counts"])
    thr = float(np.float32(IOU_THRES))
    pool = spec.get("pool")
    draw = (lambda: float(pool[rs.randint(len(pool))])) if pool else (lambda: float(rs.randint(nc)))
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
        lcls = np.array([draw() for _ in range(L)])
        xywh = np.stack((cx / W, cy / H, w / W, h / H), 1).astype(np.float32)
        rows += [(b, lcls[i], xywh[i]) for i in range(L)]
        lb = O.label_boxes(xywh, W, H) if L else np.zeros((0, 4))
        k = spec["counts"][b]
        if k < 0:
            dets[b] = np.nan                                       # as mganms_run leaves an image whose list overflowed
            continue
        conf = rs.uniform(0.02, 0.2, k) if b in spec.get("lowconf", ()) else rs.uniform(0.05, 0.95, k)
        for d in range(k):
            while True:
                if L and rs.uniform() < 0.85:
                    l = rs.randint(L)
                    s = rs.choice([0.04, 0.12, 0.3])
                    sz = np.array([lb[l, 2] - lb[l, 0], lb[l, 3] - lb[l, 1]] * 2)
                    box = lb[l] + rs.uniform(-s, s, 4) * sz
                    c = lcls[l] if rs.uniform() < 0.67 else draw()
                else:
                    bw, bh = W * rs.uniform(0.1, 0.4), H * rs.uniform(0.1, 0.4)
                    x, y = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
                    box, c = np.array([x, y, x + bw, y + bh]), draw()
                box = box.astype(np.float32).astype(np.float64)
                if box[2] > box[0] and box[3] > box[1] and _iou_ok(box, lb, thr):
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
                n=n, hw=(H, W), nc=nc, conf=spec["conf"], iou_thres=IOU_THRES, single_cls=single, m_cap=max(max(spec["labels"]), 1),
                construct=False)


def conf_thres(c):
    """what the reference substitutes for the validator's default (detconfusion.reference_conf, restated)"""
    return 0.25 if c["conf"] in (None, 0.001) else c["conf"]


def built_for(name, c, o):
    """Why the case built from a seed does not hold what it was built for ([]: it does).  o: its oracle."""
    why = []
    nc, cm = c["nc"], o["cm"]
    B = len(c["count"])
    if name in ("basic", "nc80", "nc119", "labels256", "chunks", "dets600") and not o["offdiag"]:
        why.append("no count in a class cell off the diagonal")
    if name in ("basic", "labels256", "chunks") and not (cm[nc, :nc].sum() and cm[:nc, nc].sum() and np.trace(cm[:nc, :nc])):
        why.append("no false negative, no false positive or no true positive")
    if name == "dets600" and not (cm[:nc, nc].sum() and np.trace(cm[:nc, :nc])):           # 600 rows leave no label of 40 unclaimed
        why.append("no false positive or no true positive")
    if name in ("basic", "labels256", "chunks", "dets600") and o["claims"] < 2:
        why.append("no label is claimed by two detections")
    if name == "basic":
        if not (np.any(np.diff(c["batch_idx"]) < 0) and np.any(c["batch_idx"] >= B)):
            why.append("the label rows are in order, or none belongs to no image")
        k = int(c["count"][0])
        if not np.any(np.diff(c["dets"][0, :k, 4]) > 0) or not np.any(c["dets"][0, :k, 4] <= conf_thres(c)):
            why.append("the detections are sorted by confidence, or none lies below conf_thres")
    if name == "empty":
        if not (cm[nc, :nc].sum() and cm[:nc, nc].sum()) or np.trace(cm[:nc, :nc]) or (o["det_out"][3] >= 0).any():
            why.append("the empty images do not give false negatives and false positives only")
    if name == "nword" and c["n"] is None:
        why.append("no n word")
    if name == "nc119" and not all(cm[k].sum() and cm[:, k].sum() for k in (117, 118)):
        why.append("classes 117 and 118 are not both predicted and true")
    if name == "labels256" and max(np.bincount(c["batch_idx"].astype(int))) != 256:
        why.append("no image with 256 label rows")
    if name == "chunks":
        bi = c["batch_idx"]
        if len(bi) <= STAGE or not all(np.any(bi[:STAGE] == b) and np.any(bi[STAGE:] == b) for b in range(B)):
            why.append(f"an image without label rows on both sides of row {STAGE}")
        if not np.any((o["lab_out"][STAGE:] >= 0) & (o["lab_out"][STAGE:] < nc)):
            why.append(f"no label at or behind row {STAGE} has a winner")
    if name == "dets600":
        if not _winner_across_trips(c, o):
            why.append(f"no label's winner is decided between a detection below {TRIP} and one at or above it")
    return why


def _winner_across_trips(c, o):
    """a label of image 0 claimed by a detection below TRIP and by one at or above it (image 0 holds 600 rows)"""
    thr, ct = float(np.float32(c["iou_thres"])), float(np.float32(conf_thres(c)))
    rows = np.nonzero(c["batch_idx"] == 0)[0]
    k = int(c["count"][0])
    iou = O.iou_matrix(O.label_boxes(c["bboxes"][rows], c["hw"][1], c["hw"][0]), c["dets"][0, :k, :4].astype(np.float64))[0]
    v = np.where((iou > thr) & (c["dets"][0, :k, 4] > ct)[None, :], iou, -1.0)
    lstar = np.where(v.max(0) >= 0, v.argmax(0), -1)
    return any(np.any(lstar[:TRIP] == l) and np.any(lstar[TRIP:] == l) for l in range(len(rows)))


def path(name):
    return os.path.join(GOLDEN, f"confusion_{name}.npz")


_INPUTS = ("dets", "count", "batch_idx", "cls", "bboxes")


def load(name):
    """The golden record and the case rebuilt from its seed, checked against the stored inputs: (case, record)"""
    z = np.load(path(name), allow_pickle=False)
    c = build(name, int(z["seed"]))
    for k in _INPUTS:
        assert np.array_equal(c[k], z[k], equal_nan=True), f"{name}: {k} rebuilt from seed {int(z['seed'])} differs from the stored input"
    assert int(z["nc"]) == c["nc"] and float(z["conf"]) == c["conf"] and float(z["iou_thres"]) == c["iou_thres"]
    return c, z


def oracle(name, c=None, **kw):
    c = c if c is not None else load(name)[0]
    return CO.oracle(c["dets"], c["count"], c["batch_idx"], c["cls"], c["bboxes"], c["hw"], c["nc"], conf_thres(c), c["iou_thres"],
                     single_cls=c["single_cls"], n=c["n"], round32=c["construct"], **kw)


def tensors(c, device="cpu"):
    """dets, count, batch_idx, cls, bboxes of a case as torch tensors (all the label rows, the ones behind the n word included)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t(c["dets"]), t(c["count"]), t(c["batch_idx"]), t(c["cls"]), t(c["bboxes"])


def live(c):
    """the case with the rows behind its n word cut off"""
    if c["n"] is None:
        return c
    return dict(c, batch_idx=c["batch_idx"][:c["n"]], cls=c["cls"][:c["n"]], bboxes=c["bboxes"][:c["n"]], n=None)
