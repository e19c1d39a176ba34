"""The cases of the average-precision tests: seeded cases, rebuilt from the seed recorded here, and cases by construction whose answers are
known by hand.  A case is dict(tp (n, niou) bool, conf (n) fp32, pred_cls (n) fp32, target_cls (m) fp32, nc).

Reference parity (PARITY, the goldens tests/golden/ap_<name>.npz written by tools/gen_golden_ap.py): only cases in which no two rows of one
class share a confidence -- distinct_within_class() checks it here, on the CPU -- so that the reference's unstable argsort cannot matter
and the reference alone decides the answer.  The seeded cases draw their confidences as a permutation of distinct fp32 values.  The cases
outside PARITY are answered by construction (ANSWERS) and by the oracle's rule."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SEED = 20251

# name -> (n detections, m targets, nc, niou)
SEEDED = {
    "seed_nc1_t1": (300, 90, 1, 1),
    "seed_nc3_t10": (700, 160, 3, 10),
    "seed_nc80_t10": (5000, 1500, 80, 10),
    "seed_nc300_t16": (4000, 1200, 300, 16),           # the second class digit
    "seed_nc80_junk": (3000, 900, 80, 10),             # detections of class 2.5, nc, -1 and of classes without labels among the rest
}
CONSTRUCT = ("all_true", "all_false", "perfect_rank", "recall_one_early", "labels_no_dets", "dets_no_labels", "odd_classes", "ties",
             "signed_zeros", "one_and_denormal", "no_targets", "no_detections")
CASES = tuple(SEEDED) + CONSTRUCT
TIES = ("ties", "signed_zeros")                          # equal confidences inside a class: the tie rule, by construction only
PARITY = tuple(n for n in CASES if n not in TIES)
# ap by hand (class 0, every threshold).  all_true / perfect_rank / recall_one_early: the envelope is 1 up to recall 1, and x = 1.0 takes the
# sentinel's 0, so the last of the 100 trapezoids is half: 0.995.  ties: rows (conf .5, false), (conf .5, true) in accumulation order, two
# labels: mrec = [0, 0, .5, 1], envelope = [1, .5, .5, 0]: .5 on [0, .5], then 1 - x: 0.25 + 0.125.  The other order would give 0.6225.
ANSWERS = {"all_true": 0.995, "all_false": 0.0, "perfect_rank": 0.995, "recall_one_early": 0.995, "ties": 0.375}
TIES_OTHER_ORDER = 0.6225


def path(name):
    return os.path.join(GOLDEN, f"ap_{name}.npz")


def distinct_fp32(rng, n, lo=0.001, hi=0.999):
    """n distinct fp32 values in [lo, hi], in a random order"""
    v = np.unique(np.linspace(lo, hi, 4 * n + 7).astype(np.float32))
    assert v.size >= n
    return rng.permutation(v)[:n].copy()


def random_case(rng, n, m, nc, niou, labelled=15, junk=False):
    """n detections with distinct confidences and m labels over nc classes.  At most `labelled` + 1 classes have labels (a golden holds four
    1000-point curves per such class), the last class always among them; four detections in five fall into those classes.  About a third
    of the rows are true at the first threshold, fewer at every later one (a row true at t is true at every t' < t), and a class has at
    most as many true rows as labels, as the matching guarantees (a label is owned once per threshold): recall stays within [0, 1], so
    mrec is sorted -- np.interp is undefined on abscissae that are not."""
    conf = distinct_fp32(rng, n)
    present = np.unique(np.concatenate((rng.permutation(nc)[: min(max(1, (3 * nc) // 4), labelled)], [nc - 1])))
    target_cls = rng.choice(present, size=m).astype(np.float32)
    pred_cls = np.where(rng.random(n) < 0.8, rng.choice(present, size=n), rng.integers(0, nc, size=n)).astype(np.float32)
    if junk:
        pred_cls[rng.permutation(n)[:60]] = np.repeat(np.float32([2.5, nc, -1.0, nc + 7.25]), 15)
    tp = (rng.random(n) * 3.0)[:, None] < np.linspace(1.0, 0.2, niou)[None, :]
    nt = np.bincount(target_cls.astype(np.int64), minlength=nc)
    order = rng.permutation(n)
    true = order[tp[order, 0] & (pred_cls[order] >= 0) & (pred_cls[order] < nc) & (pred_cls[order] == np.floor(pred_cls[order]))]
    k = pred_cls[true].astype(np.int64)
    by_class = true[np.argsort(k, kind="stable")]
    k = np.sort(k, kind="stable")
    rank = np.arange(k.size) - np.searchsorted(k, k, side="left")              # a true row's number within its class, in a random order
    tp[by_class[rank >= nt[k]]] = False
    return dict(tp=np.ascontiguousarray(tp), conf=conf, pred_cls=pred_cls, target_cls=target_cls, nc=nc)


def _seeded(name):
    n, m, nc, niou = SEEDED[name]
    return random_case(np.random.default_rng([SEED, sorted(SEEDED).index(name)]), n, m, nc, niou, junk=name.endswith("junk"))


def _case(tp, conf, pred_cls, target_cls, nc, niou=3):
    tp = np.asarray(tp, bool)
    if tp.ndim == 1:
        tp = np.repeat(tp[:, None], niou, 1)
    return dict(tp=np.ascontiguousarray(tp), conf=np.ascontiguousarray(conf, np.float32), pred_cls=np.ascontiguousarray(pred_cls, np.float32),
                target_cls=np.ascontiguousarray(target_cls, np.float32), nc=nc)


def _capped(c):
    """at most nt true rows per class and threshold (see random_case): the later ones in row order are made false"""
    for k in np.unique(c["target_cls"]):
        rows = np.nonzero(c["pred_cls"] == k)[0]
        over = np.cumsum(c["tp"][rows], 0) > (c["target_cls"] == k).sum()
        c["tp"][rows] &= ~over
    return c


def _constructed(name):
    rng = np.random.default_rng([SEED, 100 + CONSTRUCT.index(name)])
    if name in ("labels_no_dets", "dets_no_labels", "odd_classes"):
        return _capped(_random_constructed(name, rng))
    if name in ("ties", "signed_zeros", "one_and_denormal", "no_targets", "no_detections"):
        return _fixed_constructed(name, rng)
    if name == "all_true":
        return _case(np.ones(40, bool), distinct_fp32(rng, 40), np.zeros(40), np.zeros(40), 1)
    if name == "all_false":
        return _case(np.zeros(40, bool), distinct_fp32(rng, 40), np.zeros(40), np.zeros(25), 1)
    if name == "perfect_rank":                                                 # class 0: five labels, the five true rows rank first
        conf = np.sort(distinct_fp32(rng, 12))[::-1]
        c = _case(np.arange(12) < 5, conf, np.zeros(12), [0] * 5 + [1] * 3, 2)
        c["pred_cls"][9:] = 1
        c["tp"][9:] = False
        return c
    if name == "recall_one_early":                                             # recall is exactly 1.0 from rank 7 of 30 on: repeated abscissae
        conf = np.sort(distinct_fp32(rng, 30))[::-1]
        return _case(np.arange(30) < 7, conf, np.zeros(30), np.zeros(7), 1, niou=10)
    raise KeyError(name)


def _random_constructed(name, rng):
    if name == "labels_no_dets":                                               # class 1 has labels and no detections: a row of zeros
        return _case(rng.random(30) < 0.5, distinct_fp32(rng, 30), np.zeros(30), [0] * 9 + [1] * 4, 3)
    if name == "dets_no_labels":                                               # class 2 has detections and no labels: no row
        return _case(rng.random(30) < 0.5, distinct_fp32(rng, 30), np.repeat([0.0, 2.0], 15), [0] * 9 + [1] * 4, 3)
    if name == "odd_classes":                                                  # a detection class of 2.5, and one of nc
        cls = np.float32([0, 1, 2.5, 3, 0, 1, 2, 2.5, 3, 0, 1, 2])
        return _case(rng.random(12) < 0.6, distinct_fp32(rng, 12), cls, [0, 0, 1, 1, 2, 2], 3)
    raise KeyError(name)


def _fixed_constructed(name, rng):
    if name == "ties":
        return _case([False, True], [0.5, 0.5], [0, 0], [0, 0], 1)
    if name == "signed_zeros":                                                 # -0.0 beside +0.0 in one class, with different tp: they tie
        return _case([True, False, True, False, True], [0.25, -0.0, 0.0, -0.0, 0.0], np.zeros(5), np.zeros(4), 1)
    if name == "one_and_denormal":
        return _case([True, False, True, True], [1.0, 1e-40, 0.5, 1e-44], np.zeros(4), np.zeros(3), 1)
    if name == "no_targets":
        return _case(rng.random(10) < 0.5, distinct_fp32(rng, 10), rng.integers(0, 3, 10), np.zeros(0), 3)
    if name == "no_detections":
        return _case(np.zeros((0, 3), bool), np.zeros(0), np.zeros(0), [0, 0, 2], 3)
    raise KeyError(name)


def build(name):
    return _seeded(name) if name in SEEDED else _constructed(name)


def distinct_within_class(c):
    """no two rows of one class share a confidence (-0.0 and +0.0 are the same confidence)"""
    pairs = np.stack((c["pred_cls"].astype(np.float64), c["conf"].astype(np.float64) + 0.0), 1)
    return np.unique(pairs, axis=0).shape[0] == pairs.shape[0]


def load_golden(name):
    """-> (the case's inputs as recorded, the reference's twelve outputs)"""
    z = np.load(path(name), allow_pickle=False)
    return {k: z[k] for k in ("tp", "conf", "pred_cls", "target_cls")}, tuple(z[f"ref{i}"] for i in range(12))
