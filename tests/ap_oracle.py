"""Average precision per class, stated twice in fp64 numpy and compared:

  procedure()  the literal procedure of the reference's ap_per_class as the issue describes it: one argsort over every detection, a loop
               over the unique target classes, per class and threshold a cumulative sum, a reversed running maximum, np.interp on 101 and
               1000 points, np.trapezoid, then the box-filtered F1 maximum.  (The sort is stable here; the reference's is not, so cases
               with equal confidences inside a class are kept out of reference parity: ap_cases.PARITY.)
  rule()       the parallel rule of include/ext/mgaap.h, shaped as the kernels compute it: ONE order over all rows (class, then descending
               confidence, then row index), ONE inclusive scan of each tp column over that order (a class's running count is the scan minus
               its value before the class's first row), a running maximum from the right that resets at class boundaries, and np.interp's
               index rule spelled out: the last j with xp[j] <= x.

Both return with every ap the sum S of the absolute trapezoid terms it is the sum of: the bar for a sum taken in another order is
128 * 2^-53 * S (100 additions).  Everything else -- recall, precision, the envelope, the interpolated curves -- is the same sequence of
correctly rounded fp64 operations in both and must be EQUAL."""
import warnings

import numpy as np

X101, X1000 = np.linspace(0, 1, 101), np.linspace(0, 1, 1000)
AP_ULPS = 128 * 2.0 ** -53


def _trapezoid(y, x):
    terms = (x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0
    return terms, float(np.abs(terms).sum())


def procedure(tp, conf, pred_cls, target_cls, eps=1e-16):
    """-> the 12-tuple, in the reference's (compact) form, and ap_abs of ap's shape"""
    tp, conf, pred_cls = np.asarray(tp), np.asarray(conf), np.asarray(pred_cls)
    order = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, nt = np.unique(target_cls, return_counts=True)
    k = classes.shape[0]
    ap, ap_abs = np.zeros((k, tp.shape[1])), np.zeros((k, tp.shape[1]))
    p_curve, r_curve, prec_values = np.zeros((k, 1000)), np.zeros((k, 1000)), []
    trapz = np.trapezoid if hasattr(np, "trapezoid") else np.trapz
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if sel.sum() == 0 or nt[ci] == 0:
            continue
        tpc = tp[sel].cumsum(0)
        fpc = (1 - tp[sel]).cumsum(0)
        recall = tpc / (nt[ci] + eps)
        precision = tpc / (tpc + fpc)
        r_curve[ci] = np.interp(-X1000, -conf[sel], recall[:, 0], left=0)
        p_curve[ci] = np.interp(-X1000, -conf[sel], precision[:, 0], left=1)
        for t in range(tp.shape[1]):
            mrec = np.concatenate(([0.0], recall[:, t], [1.0]))
            mpre = np.flip(np.maximum.accumulate(np.flip(np.concatenate(([1.0], precision[:, t], [0.0])))))
            y = np.interp(X101, mrec, mpre)
            ap[ci, t] = trapz(y, X101)
            ap_abs[ci, t] = _trapezoid(y, X101)[1]
            if t == 0:
                prec_values.append(np.interp(X1000, mrec, mpre))
    prec_values = np.array(prec_values) if prec_values else np.zeros((1, 1000))
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mean = f1_curve.mean(0)
        nf = round(len(mean) * 0.1 * 2) // 2 + 1
        ends = np.ones(nf // 2)
        i = np.convolve(np.concatenate((ends * mean[0], mean, ends * mean[-1])), np.ones(nf) / nf, mode="valid").argmax()
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    tpn = (r * nt).round()
    fpn = (tpn / (p + eps) - tpn).round()
    return (tpn, fpn, p, r, f1, ap, classes.astype(int), p_curve, r_curve, f1_curve, X1000, prec_values), ap_abs


def interp_rule(x, xp, fp, left=None):
    """np.interp by its index rule, every point at once (fp64, each operation rounded once)"""
    x, xp, fp = np.asarray(x, np.float64), np.asarray(xp, np.float64), np.asarray(fp, np.float64)
    last = len(xp) - 1
    j = np.searchsorted(xp, x, side="right") - 1                     # the last j with xp[j] <= x; -1 below xp[0]
    at = np.clip(j, 0, last)
    nxt = np.minimum(at + 1, last)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = (fp[nxt] - fp[at]) / (xp[nxt] - xp[at])
        between = slope * (x - xp[at]) + fp[at]
    out = np.where((at == last) | (xp[at] == x), fp[at], between)
    return np.where(j < 0, fp[0] if left is None else left, out)


def rule(tp, conf, pred_cls, target_cls, nc):
    """-> dense dict(ap, ap_abs (nc, niou), p_curve, r_curve, prec_values (nc, 1000), nt, n_det (nc) int32), as mgaap_run's result block"""
    tp = np.asarray(tp) != 0
    conf = np.asarray(conf, np.float32)
    pred_cls, target_cls = np.asarray(pred_cls, np.float64), np.asarray(target_cls, np.float64)
    n, niou = tp.shape
    assert not np.isnan(conf).any() and ((target_cls == np.floor(target_cls)) & (target_cls >= 0) & (target_cls < nc)).all()
    nt = np.bincount(target_cls.astype(np.int64), minlength=nc)
    with np.errstate(invalid="ignore"):
        counted = np.isfinite(pred_cls) & (pred_cls == np.floor(pred_cls)) & (pred_cls >= 0) & (pred_cls < nc)
    klass = np.where(counted, pred_cls, nc).astype(np.int64)                  # rows of no class: a bin behind class nc - 1
    c64 = np.where(conf == 0, np.float32(0), conf).astype(np.float64)         # -0.0 taken as +0.0
    order = np.lexsort((np.arange(n), -c64, klass))                           # class, descending confidence, row index
    n_det = np.bincount(klass, minlength=nc + 1)[:nc]
    first = np.concatenate(([0], np.cumsum(n_det)))
    S = np.cumsum(tp[order].astype(np.int64), 0)                              # one scan over everything
    out = dict(ap=np.zeros((nc, niou)), ap_abs=np.zeros((nc, niou)), p_curve=np.zeros((nc, 1000)), r_curve=np.zeros((nc, 1000)),
               prec_values=np.zeros((nc, 1000)), nt=nt.astype(np.int32), n_det=n_det.astype(np.int32))
    for c in range(nc):
        a, b = first[c], first[c + 1]
        if nt[c] == 0 or a == b:
            continue
        before = S[a - 1] if a > 0 else np.zeros(niou, np.int64)
        tpc = (S[a:b] - before).astype(np.float64)
        recall = tpc / (np.float64(nt[c]) + 1e-16)
        precision = tpc / np.arange(1, b - a + 1, dtype=np.float64)[:, None]
        xp = -c64[order[a:b]]
        out["r_curve"][c] = interp_rule(-X1000, xp, recall[:, 0], left=0.0)
        out["p_curve"][c] = interp_rule(-X1000, xp, precision[:, 0], left=1.0)
        for t in range(niou):
            env = np.maximum.accumulate(precision[::-1, t])[::-1]             # from the right; the carry starts anew in every class
            mrec = np.concatenate(([0.0], recall[:, t], [1.0]))
            mpre = np.concatenate(([1.0], env, [0.0]))                        # precision <= 1: the left sentinel stays 1
            y = interp_rule(X101, mrec, mpre)
            terms, out["ap_abs"][c, t] = _trapezoid(y, X101)
            out["ap"][c, t] = np.cumsum(terms)[-1]                            # a fixed order: ascending (cumsum adds one by one)
            if t == 0:
                out["prec_values"][c] = interp_rule(X1000, mrec, mpre)
    return out


def compact(dense):
    """the dense arrays -> the rows the reference has: ap, p_curve, r_curve of the classes with labels; prec_values of those with
    detections as well (one row of zeros if there is none); the classes"""
    keep = np.nonzero(dense["nt"] > 0)[0]
    both = np.nonzero((dense["nt"] > 0) & (dense["n_det"] > 0))[0]
    return dict(classes=keep, ap=dense["ap"][keep], p_curve=dense["p_curve"][keep], r_curve=dense["r_curve"][keep],
                prec_values=dense["prec_values"][both] if both.size else np.zeros((1, 1000)),
                ap_abs=dense["ap_abs"][keep] if "ap_abs" in dense else None)


def compare(tp, conf, pred_cls, target_cls, nc):
    """the two statements against each other on one case: the classes, the curves and the sums of absolute terms EQUAL, ap within its
    bound (np.trapezoid adds pairwise, the rule in ascending order); -> (the procedure's tuple, the rule's dense arrays)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lit, lit_abs = procedure(tp, conf, pred_cls, target_cls)
    dense = rule(tp, conf, pred_cls, target_cls, nc)
    c = compact(dense)
    assert np.array_equal(c["classes"], lit[6]) and np.array_equal(c["ap_abs"], lit_abs)
    for k, i in (("p_curve", 7), ("r_curve", 8), ("prec_values", 11)):
        assert np.array_equal(c[k], lit[i]), k
    assert (np.abs(c["ap"] - lit[5]) <= AP_ULPS * lit_abs).all()
    return lit, dense


def assert_dense(got, want, what=""):
    """a result block (device or _host_curves) against rule(): integers and curves equal, ap within 128 * 2^-53 * S"""
    for k in ("nt", "n_det"):
        assert np.array_equal(got[k], want[k]), (what, k)
    for k in ("p_curve", "r_curve", "prec_values"):
        bad = np.nonzero(got[k] != want[k])
        assert bad[0].size == 0, (what, k, bad[0][:4], bad[1][:4], got[k][bad][:4], want[k][bad][:4])
    err, bound = np.abs(got["ap"] - want["ap"]), AP_ULPS * want["ap_abs"]
    print(f"{what}: ap max |diff| {err.max() if err.size else 0:.3e}, smallest bound with a difference "
          f"{bound[err > 0].min() if (err > 0).any() else 0:.3e}")
    assert (err <= bound).all(), (what, "ap", err.max(), np.nonzero(err > bound))


def assert_tuple(got, want, ap_abs, what=""):
    """two 12-tuples: everything equal but ap, which is within its bound"""
    assert len(got) == len(want) == 12
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, i, g.shape, w.shape)
        if i == 5:
            assert (np.abs(g - w) <= AP_ULPS * ap_abs).all(), (what, "ap", np.abs(g - w).max())
        else:
            assert np.array_equal(g, w, equal_nan=True), (what, i)
