"""Cases of the detection post-process (include/mganms.h, csrc/nms.cuh): the smallest shapes at which each piece can go wrong.

Two kinds of features, both numpy.random.RandomState (a frozen stream) and arithmetic only, rounded once to fp32:
  trained-like   the recipe of tests/det_cases.py: background 0.5 n in the bins, the classes uniform in [-5.5, -2.7] (probabilities 0.004 to 0.063:
                 a candidate at conf 0.001, none at 0.25; four octaves, so that bit-equal scores among 1344 anchors stay rare); inside a box the bin logits of a side -(j - t)^2 / 1.5 + 0.3 n around the true distance t moved by
                 up to a cell, and the row's class logit lg + lsd n (default 1.5 + n).  Clusters of anchors predict nearly the same box.
  by construction   every class logit -20 (probability 2e-9) except at the placed anchors, whose four sides are one-hot (+-40) on one bin, or on
                 two neighbouring bins for a distance of k + 0.5: the softmax expectation is exact in fp32 and fp64, so the boxes, their IoUs
                 and the answer are known by construction: ANSWERS.

tests/golden/nms_<name>.npz (tools/gen_golden_nms.py) holds the features of a small case whole; a larger one records the seed the generator
accepted and the SHA-256 of the features, and load() refuses rebuilt features whose digest differs.  Either way it holds what the reference's
own Detect._inference and non_max_suppression gave on exactly these values, from an fp32 and an fp64 run -- for the cases of PARITY.  A case
with parity=False (cut_ties, cut_ties_wide) is held to its construction and the oracle alone, and its record holds no reference lists.

Which path of csrc/nms.cuh runs where:
  nms_select in LDS            maxnms (distinct scores: the score word decides), cut_ties (the cut inside 86 equal scores: the four low passes)
  nms_select in the workspace  cut_ties_wide (1280 candidates, their indices over two bytes of the low word), and the stored `wide` features at
                               max_nms 1, 1023, 1024, 1025, 1100, 1343 (SELECT_CUTS; 1344 = n: no select)
  nms_rounds in the workspace  wide (nc 1: by_class false), ml_wide (nc 80: by_class true, some 4500 candidates an image)
  multi-label append           classes_ml (4 anchors, nc 3), ml_wide (a full wave and one of 20 lanes, 44 to 64 classes an anchor, unequal counts;
                               cand_cap crossed inside an anchor's classes: the GPU tests' overflow run)
  `pred` in fp16 / bf16        basic, classes, wide (PRED_HALF_CASES): in `wide` scores tie by the hundreds and the tie order decides the answer;
                               wide cut at max_nms 700: in some images the 700th and 701st scores are equal, the select's low passes decide
A plan replayed across the paths (long list, empty list, long list) is the GPU tests' own."""
import hashlib
import os

import numpy as np
import torch

import nms_oracle as O

DEFAULTS = dict(conf_thres=0.25, iou_thres=0.45, max_det=300, max_nms=30000, multi_label=False, agnostic=False)
S3 = (8, 16, 32)
LDS = 1024                                     # kNmsLds of csrc/nms.cuh
STORE_WHOLE = 1 << 16                          # feature elements up to which a case is stored whole

_OBJ = [(0, 0, 6.3, 9.1, 41.7, 50.2), (0, 0, 30.5, 20.2, 60.9, 45.1), (0, 0, 4.2, 44.3, 24.6, 62.1), (1, 0, 10.4, 5.7, 52.6, 58.3),
        (1, 0, 40.3, 2.2, 62.1, 20.7)]
_OBJ2 = [(0, 1, 6.3, 9.1, 41.7, 50.2), (0, 0, 50.5, 20.2, 90.9, 45.1), (1, 0, 10.4, 5.7, 52.6, 58.3), (1, 1, 60.3, 12.2, 92.1, 40.7)]
_CLS = [(0, 0, 2, 2, (2, 2, 2, 2), {0: 3.0}), (0, 0, 2, 3, (3, 2, 1, 2), {1: 2.0}), (0, 0, 3, 2, (2, 3, 2, 1), {2: 1.0}),
        (0, 0, 5, 5, (1.5, 1.5, 1.5, 1.5), {0: 2.5, 2: 0.5})]
_CHAIN = [(0, 0, 3, 2, (2.5,) * 4, {0: 3.0}), (0, 0, 3, 3, (2.5,) * 4, {0: 2.0}), (0, 0, 3, 4, (2.5,) * 4, {0: 1.0})]
_TIE3 = (2.0, 1.0, 0.0)
_CELL = (0.5,) * 4                             # a box that is exactly its anchor's cell
_CUT = [(0, 0, y, x, _CELL, {0: _TIE3[(y + x) % 3]}) for y in range(16) for x in range(16)]
_CUT_WIDE = [(0, 0, y, x, _CELL, {0: _TIE3[(y + x) % 3]}) for y in range(32) for x in range(32)] + \
            [(1, 0, y, x, _CELL, {0: _TIE3[(y + 2 * x) % 3]}) for y in range(16) for x in range(16)]
# trained-like: rows = (image, class, x1, y1, x2, y2[, dict(lg=, lsd=)]); by construction: puts = (level, image, y, x, (l, t, r, b) in cells, {class: logit})
CASES = {
    "basic": dict(B=2, hw=(64, 64), nc=1, strides=S3, rows=_OBJ),
    # a suppresses b, b would have suppressed c (IoU 2/3 at a shift of one cell, 3/7 at two): c is kept
    "chain": dict(B=1, hw=(64, 64), nc=1, strides=S3, puts=_CHAIN),
    # the same box in three classes; an anchor over conf in two classes
    "classes": dict(B=1, hw=(64, 64), nc=3, strides=S3, puts=_CLS),
    "classes_ml": dict(B=1, hw=(64, 64), nc=3, strides=S3, puts=_CLS, kw=dict(multi_label=True)),
    "classes_agn": dict(B=1, hw=(64, 64), nc=3, strides=S3, puts=_CLS, kw=dict(agnostic=True)),
    "classes_ml_agn": dict(B=1, hw=(64, 64), nc=3, strides=S3, puts=_CLS, kw=dict(multi_label=True, agnostic=True)),
    "empty": dict(B=2, hw=(64, 64), nc=1, strides=S3, puts=[(0, 1) + p[2:] for p in _CHAIN]),
    "empty_all": dict(B=2, hw=(64, 64), nc=1, strides=S3, puts=[]),
    # eight disjoint boxes (each its own cell), scores descending in the order listed
    "maxdet": dict(B=1, hw=(64, 64), nc=1, strides=S3, kw=dict(max_det=5),
                   puts=[(0, 0, y, x, (0.5,) * 4, {0: 3.0 - 0.25 * i}) for i, (y, x) in enumerate(((5, 3), (1, 1), (3, 5), (1, 5), (5, 1), (3, 1), (1, 3), (3, 3)))]),
    # 84 anchors of a high-scoring object, 42 of a low-scoring one beside it: the best of the second survives, at a rank past max_nms
    "maxnms": dict(B=1, hw=(96, 96), nc=1, strides=S3, kw=dict(max_nms=40),
                   rows=[(0, 0, 2.3, 2.2, 60.4, 60.1, dict(lg=3.0, lsd=0.3)), (0, 0, 64.2, 2.4, 94.3, 60.2, dict(lg=0.3, lsd=0.1))]),
    # bit-equal scores: an overlapping pair (IoU 0.6), a disjoint pair, one box of its own score between them
    "ties": dict(B=1, hw=(64, 64), nc=1, strides=S3,
                 puts=[(0, 0, 1, 1, (2,) * 4, {0: 2.0}), (0, 0, 1, 2, (2,) * 4, {0: 2.0}), (0, 0, 5, 1, (0.5,) * 4, {0: 1.0}),
                       (0, 0, 5, 5, (0.5,) * 4, {0: 1.0}), (0, 0, 6, 3, (0.5,) * 4, {0: 1.5})]),
    # 1344 anchors, every one a candidate: more than one trip of every strided loop, a list past kNmsLds, 17 workgroups, max_det reached.
    # tight: a background anchor predicts a box inside its own cell (sides peaked at 0.3 cells), so the hundreds of thousands of background
    # pairs the visit compares have an IoU of 0, or of some 0.2 across levels, and the guard on near-threshold pairs can hold at all
    "wide": dict(B=17, hw=(256, 256), nc=1, strides=S3, kw=dict(conf_thres=0.001), tight=True,
                 rows=[(0, 0, 12.3, 20.4, 44.6, 50.7), (5, 0, 170.2, 8.3, 220.7, 40.9), (16, 0, 140.6, 130.3, 170.2, 160.8), (16, 0, 8.9, 180.4, 40.3, 220.6)]),
    # every level-0 anchor placed with its own cell as its box (every IoU 0), three scores in a diagonal pattern: the max_nms cut falls inside
    # the second group of equal scores, so the select's four low passes, over the inverted candidate index, decide it -- in LDS.
    # parity=False: the reference cuts behind an unstable argsort, so which of the equal scores it keeps is not defined; the case is held to
    # its construction (ANSWERS) and the oracle, and its record holds no reference lists
    "cut_ties": dict(B=1, hw=(128, 128), nc=1, strides=S3, puts=_CUT, kw=dict(max_nms=120, max_det=2000), parity=False),
    # the same in the workspace: 1024 level-0 anchors and the 256 of level 1 (a level-1 cell holds four level-0 cells: IoU 0.25, nothing is
    # suppressed), 1280 candidates whose indices spread over two bytes of the key's low word.  parity=False for the same reason
    "cut_ties_wide": dict(B=1, hw=(256, 256), nc=1, strides=S3, puts=_CUT_WIDE, kw=dict(max_nms=700, max_det=2000), parity=False),
    # multi-label at a trained-like class count: 84 anchors (a full wave and one of 20 lanes), 44 to 64 candidate classes each, some 4500
    # candidates an image: the wave scan over unequal counts, the per-class append, by_class in the workspace, max_det reached
    "ml_wide": dict(B=2, hw=(64, 64), nc=80, strides=S3, kw=dict(conf_thres=0.01, multi_label=True), tight=True,
                    rows=[(0, 3, 6.3, 9.1, 41.7, 50.2), (0, 17, 30.5, 20.2, 60.9, 45.1), (1, 79, 10.4, 5.7, 52.6, 58.3), (1, 0, 40.3, 2.2, 62.1, 20.7)]),
    "lv1": dict(B=2, hw=(64, 96), nc=2, strides=(8,), rows=_OBJ2),
    "lv2": dict(B=2, hw=(64, 96), nc=2, strides=(8, 16), rows=_OBJ2),
    "lv4": dict(B=2, hw=(64, 96), nc=2, strides=(4, 8, 16, 32), rows=_OBJ2),
}
NAMES = list(CASES)
PARITY = [n for n in NAMES if CASES[n].get("parity", True)]        # held to the reference's own lists
HALF_CASES = ("basic", "classes", "wide", "ml_wide")
# the `pred` front end on an fp16 / bf16 prediction: (case, arguments that replace the case's).  The last: `wide` cut at max_nms 700 with
# max_det out of reach, so that the select in the workspace cuts inside equal scores of trained-like values and every survivor is a kept row
PRED_HALF_CASES = (("basic", {}), ("classes", {}), ("wide", {}), ("wide", dict(max_nms=700, max_det=1400)))
PRED_HALF_IDS = ["basic", "classes", "wide", "wide_cut"]
# the select on the stored `wide` features: its images 0 and 1 (1344 candidates each) at these max_nms, max_det above every count
SELECT_CUTS = (1, 1023, 1024, 1025, 1100, 1343, 1344)
SELECT_KW = dict(max_det=1400)
# the kept anchors and their classes, by construction (anchor = y * 8 + x on level 0 of a 64^2 image)
ANSWERS = {
    "chain": ([[26, 28]], [[0, 0]]),
    "classes": ([[18, 45, 19, 26]], [[0, 0, 1, 2]]),
    "classes_ml": ([[18, 45, 19, 26, 45]], [[0, 0, 1, 2, 2]]),
    "classes_agn": ([[18, 45]], [[0, 0]]),
    "classes_ml_agn": ([[18, 45]], [[0, 0]]),
    "empty": ([[], [26, 28]], [[], [0, 0]]),
    "empty_all": ([[], []], [[], []]),
    "maxdet": ([[43, 9, 29, 13, 41]], [[0] * 5]),
    "ties": ([[9, 51, 41, 45]], [[0] * 4]),
}
# what each deliberately wrong rule must get wrong (tests/test_nms_oracle.py; the same four mistakes were put into local builds of the kernels)
MUTATIONS = {"chain": dict(kept_only=False), "classes": dict(compare_classes=False), "maxnms": dict(max_nms=1 << 30), "ties": dict(lowest_first=False),
             "cut_ties": dict(lowest_first=False), "cut_ties_wide": dict(lowest_first=False)}
TIE_ORDER = tuple(n for n, m in MUTATIONS.items() if m == dict(lowest_first=False))      # the cases whose answer the tie order decides


def kw(name):
    c = CASES[name]
    return dict(DEFAULTS, nc=c["nc"], strides=tuple(c["strides"]), **c.get("kw", {}))


def shapes(name):
    c = CASES[name]
    return [(c["hw"][0] // s, c["hw"][1] // s) for s in c["strides"]]


def anchors(name):
    return sum(h * w for h, w in shapes(name))


def elements(name):
    c = CASES[name]
    return c["B"] * (64 + c["nc"]) * anchors(name)


def _cut_answer(name):
    """cut_ties, cut_ties_wide: nothing is suppressed and max_det is out of reach, so the kept rows are the first max_nms of the placed
    anchors by (logit descending, anchor ascending), from the puts."""
    a0 = np.cumsum([0] + [h * w for h, w in shapes(name)])
    width = [w for _, w in shapes(name)]
    rows = sorted((-lg[0], int(a0[l]) + y * width[l] + x) for l, _, y, x, _, lg in CASES[name]["puts"])
    n = kw(name)["max_nms"]
    assert n < len(rows) and rows[n - 1][0] == rows[n][0], "the cut does not fall inside a group of equal scores"
    return [[a for _, a in rows[:n]]], [[0] * n]


ANSWERS.update({n: _cut_answer(n) for n in ("cut_ties", "cut_ties_wide")})


def build_feats(name, seed):
    """The case's feature maps (B, 64 + nc, H_l, W_l), fp32."""
    c = CASES[name]
    B, nc = c["B"], c["nc"]
    j = np.arange(16, dtype=np.float64)
    feats = []
    if "puts" in c:
        for h, w in shapes(name):
            f = np.zeros((B, 64 + nc, h, w))
            f[:, 64:] = -20.0
            feats.append(f)
        for l, b, y, x, dist, logits in c["puts"]:
            for s, d in enumerate(dist):
                hot = (j == np.floor(d)) | (j == np.ceil(d))
                feats[l][b, 16 * s:16 * s + 16, y, x] = np.where(hot, 40.0, -40.0)
            for k, v in logits.items():
                feats[l][b, 64 + k, y, x] = v
        return [torch.from_numpy(f.astype(np.float32)) for f in feats]
    rs = np.random.RandomState(seed)
    for s, (h, w) in zip(c["strides"], shapes(name)):
        f = 0.5 * rs.standard_normal((B, 64 + nc, h, w))
        if c.get("tight"):
            f[:, :64] = (-(j - 0.3) * (j - 0.3) / 0.2).reshape(1, 1, 16, 1, 1).repeat(4, 1).reshape(1, 64, 1, 1) + 0.1 * rs.standard_normal((B, 64, h, w))
        f[:, 64:] = rs.uniform(-5.5, -2.7, (B, nc, h, w))
        py, px = np.meshgrid((np.arange(h) + 0.5) * s, (np.arange(w) + 0.5) * s, indexing="ij")
        for row in c["rows"]:
            b, k, x1, y1, x2, y2 = row[:6]
            opt = row[6] if len(row) > 6 else {}
            ys, xs = np.nonzero((x1 < px) & (px < x2) & (y1 < py) & (py < y2))
            m = ys.size
            t = np.stack((px[ys, xs] - x1, py[ys, xs] - y1, x2 - px[ys, xs], y2 - py[ys, xs]), 1) / s
            far = (t > 15.0).any(1)                                  # a side no bin reaches: the level leaves this anchor to the coarser ones
            t = np.clip(t + (rs.random_sample((m, 4)) * 2 - 1), 0.0, 15.0)
            bins = -(j[None, None] - t[:, :, None]) * (j[None, None] - t[:, :, None]) / 1.5 + 0.3 * rs.standard_normal((m, 4, 16))
            logit = opt.get("lg", 1.5) + opt.get("lsd", 1.0) * rs.standard_normal(m)
            ys, xs, bins, logit = ys[~far], xs[~far], bins[~far], logit[~far]
            f[b, :64, ys, xs] = bins.reshape(-1, 64)
            f[b, 64 + k, ys, xs] = logit
        feats.append(torch.from_numpy(f.astype(np.float32)))
    return feats


def digest(feats):
    d = hashlib.sha256()
    for f in feats:
        d.update(np.ascontiguousarray(f.numpy(), dtype="<f4").tobytes())
    return d.hexdigest()


def path(name):
    return os.path.join(O.GOLDEN, f"nms_{name}.npz")


def ref_decode(feats, strides, nc):
    """The decoded prediction (B, 4 + nc, A) as Detect._inference forms it -- anchor -+ distance, then centre and size, times the stride --
    in torch ops of the features' element type: the input of the `pred` front end."""
    B = feats[0].shape[0]
    dt = feats[0].dtype
    x = torch.cat([f.reshape(B, 64 + nc, -1) for f in feats], 2)
    A = x.shape[2]
    d = (x[:, :64].reshape(B, 4, 16, A).transpose(2, 1).softmax(1) * torch.arange(16, dtype=dt).view(1, 16, 1, 1)).sum(1)      # (B, 4, A)
    ax, ay, st = [], [], []
    for f, s in zip(feats, strides):
        h, w = f.shape[2:]
        yy, xx = torch.meshgrid(torch.arange(h, dtype=dt) + 0.5, torch.arange(w, dtype=dt) + 0.5, indexing="ij")
        ax.append(xx.reshape(-1)); ay.append(yy.reshape(-1)); st.append(torch.full((h * w,), float(s), dtype=dt))
    anc, st = torch.stack((torch.cat(ax), torch.cat(ay)))[None], torch.cat(st)[None, None]
    lt, rb = anc - d[:, :2], anc + d[:, 2:]
    return torch.cat((torch.cat(((lt + rb) / 2, rb - lt), 1) * st, x[:, 64:].sigmoid()), 1)


def load(name):
    """The record of tests/golden/nms_<name>.npz with its features (stored, or rebuilt from its seed and checked against its digest)."""
    z = np.load(path(name))
    c = {k: z[k] for k in z.files}
    nl = len(CASES[name]["strides"])
    if "feat0" in c:
        feats = [torch.from_numpy(c[f"feat{l}"]) for l in range(nl)]
    else:
        feats = build_feats(name, int(c["seed"]))
        assert digest(feats) == str(c["sha256"]), f"{name}: the rebuilt features are not the ones the record was made from"
    k = kw(name)
    for key in DEFAULTS:
        assert float(c[key]) == float(k[key]), f"{name}: {key} differs from the record"
    B = CASES[name]["B"]
    c.update(name=name, B=B, feats=feats, kw=k)
    if name not in PARITY:
        assert "ref_count" not in c, f"{name}: a case without parity holds no reference lists"
        return c
    cnt = c["ref_count"]
    off = np.concatenate(([0], np.cumsum(cnt)))
    c.update(ref32=[c["ref_dets_f32"][off[b]:off[b + 1]] for b in range(B)], ref64=[c["ref_dets_f64"][off[b]:off[b + 1]] for b in range(B)],
             ref_keep=[c["ref_keep_all"][off[b]:off[b + 1]] for b in range(B)])
    return c


_CACHE = {}


def oracle(name, dtype=None, front="maps"):
    """The oracle's answer on the case's features (dtype: rounded to fp16 / bf16 first), computed once and shared; front="pred": on the
    reference-style decoded prediction of the fp32 features instead."""
    key = (name, dtype, front)
    if key not in _CACHE:
        feats = load(name)["feats"]
        if dtype is not None:
            feats = [f.to(dtype).float() for f in feats]
        k = kw(name)
        if front == "pred":
            o = O.oracle(pred=ref_decode(feats, k["strides"], k["nc"]).numpy(), **k)
        else:
            o = O.oracle(feats=[f.numpy() for f in feats], **k)
        _CACHE[key] = o
    return _CACHE[key]


def select_case(max_nms):
    """The select on stored features: images 0 and 1 of `wide`, max_det above every count, the given max_nms -> (feats, arguments, the
    oracle's answer under them), computed once and shared."""
    key = ("select", max_nms)
    if key not in _CACHE:
        feats = [f[:2].contiguous() for f in load("wide")["feats"]]
        k = dict(kw("wide"), max_nms=max_nms, **SELECT_KW)
        _CACHE[key] = (feats, k, O.oracle(feats=[f.numpy() for f in feats], **k))
    return _CACHE[key]


def pred_half(name, dtype, lowest_first=True, **over):
    """The reference-style decoded prediction of the case's fp32 features rounded to fp16 / bf16 -> (the rounded prediction, the arguments
    without strides, the oracle's answer on its upcast values), computed once and shared.  over: arguments that replace the case's."""
    key = ("pred_half", name, dtype, lowest_first, tuple(sorted(over.items())))
    if key not in _CACHE:
        k = dict(kw(name), **over)
        strides = k.pop("strides")
        pred = ref_decode(load(name)["feats"], strides, k["nc"]).to(dtype)
        _CACHE[key] = (pred, k, O.oracle(pred=pred.float().numpy(), lowest_first=lowest_first, **k))
    return _CACHE[key]


def built_for(name, feats):
    """What the case was built to hold, beyond its ANSWERS; returns the reasons it does not (empty: it does)."""
    why = []
    k = kw(name)
    np_feats = [f.numpy() for f in feats]
    o = O.oracle(feats=np_feats, **k)
    if name == "basic" and not (o["count"] >= 2).all():
        why.append(f"counts {o['count'].tolist()}")
    if name == "maxnms":
        free = O.oracle(feats=np_feats, **dict(k, max_nms=1 << 30))
        if not (80 <= o["n_cand"][0] <= 160):
            why.append(f"{o['n_cand'][0]} candidates")
        if not free["count"][0] > o["count"][0]:
            why.append("no survivor past max_nms")
    if name == "wide":
        if not all(n == anchors(name) for n in o["n_cand"]) or anchors(name) <= LDS:
            why.append("not every anchor is a candidate")
        if not (o["count"] >= 2).all():
            why.append(f"counts {o['count'].tolist()}")
    if name in ("cut_ties", "cut_ties_wide"):
        free = O.oracle(feats=np_feats, **dict(k, max_nms=1 << 30))
        placed = len(CASES[name]["puts"])
        if o["n_cand"] != [placed] or (placed > LDS) != (name == "cut_ties_wide"):
            why.append(f"{o['n_cand']} candidates of {placed} placed anchors")
        if o["count"].tolist() != [k["max_nms"]] or free["count"].tolist() != [placed]:
            why.append(f"counts {o['count'].tolist()} with max_nms, {free['count'].tolist()} without")
    if name == "ml_wide":
        _, prob, _ = O.decode(np_feats, k["strides"], k["nc"])
        per = (prob > k["conf_thres"]).sum(2)                       # (B, A): an anchor's candidates, a lane's count in k_nms_cand's scan
        if not all(n > LDS for n in o["n_cand"]):
            why.append(f"{o['n_cand']} candidates: not past {LDS} in every image")
        if anchors(name) % 64 == 0 or not all(len(set(per[b, w:w + 64].tolist())) >= 2 for b in range(per.shape[0]) for w in range(0, per.shape[1], 64)):
            why.append("a wave whose lanes all have the same count, or no partly live wave")
        if not (o["count"] == k["max_det"]).all():
            why.append(f"counts {o['count'].tolist()}: max_det is not reached")
        if not all(len(set(o["dets"][b, :o["count"][b], 5].tolist())) >= 2 for b in range(per.shape[0])):
            why.append("kept rows of one class only")
    if name in ("lv1", "lv2", "lv4"):
        a0 = np.cumsum([0] + [h * w for h, w in shapes(name)])
        kept = o["keep"][o["keep"] >= 0]
        if not all(((kept >= a0[l]) & (kept < a0[l + 1])).any() for l in range(len(a0) - 1)):
            why.append("a level without a kept anchor")
        if len(set(o["dets"][..., 5][o["keep"] >= 0].tolist())) < 2:
            why.append("one class only")
    if name in MUTATIONS:
        m = O.oracle(feats=np_feats, **dict(k, **MUTATIONS[name]))
        if np.array_equal(m["keep"], o["keep"]):
            why.append("the wrong rule gives the same answer")
    return why


def check(what, dets, count, keep, o, bar=None):
    """dets (B, max_det, 6), count (B), keep (B, max_det) of an evaluation against the oracle's result `o`: the kept set, its order, cls,
    keep and count exact, the rows past the count zero / -1, coordinates and scores within bar (default O.K) eps_fp32 terms.  Returns the
    largest ratio met (printed before it is asserted)."""
    dets, count, keep = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t) for t in (dets, count, keep))
    assert np.array_equal(count, o["count"]), f"{what}: count {count.tolist()}, the oracle's {o['count'].tolist()}"
    assert np.array_equal(keep, o["keep"]), f"{what}: keep differs from the oracle's"
    assert np.array_equal(dets[..., 5], o["dets"][..., 5]), f"{what}: cls differs from the oracle's"
    r = O.ratio(dets[..., :5], o["dets"][..., :5], o["terms"][..., :5])
    bar = O.K if bar is None else bar
    print(f"{what}: |err| / (eps terms) = {r:.3f} (bar {bar:.3f})")
    assert r <= bar, f"{what}: |err| = {r:.3f} eps terms, the bar is {bar:.3f}"
    return r
