"""Average precision per class (include/ext/mgaap.h): what the reference's `ap_per_class` (ultralytics/utils/metrics.py:727-854, called from
`DetMetrics.process`, :1087-1117) does on the host after every row of the run was read back -- an argsort over the run's detections, a
Python loop over the classes, per class and threshold a cumulative sum, a reversed running maximum and four interpolations -- restated as
a parallel rule and run on the device, as the fourth stage behind `detect_postprocess`, `match_detections` and `confusion_matrix`.

The rule, in fp64: within a class the rows are ordered by descending confidence, equal confidences staying in accumulation order (-0.0
equal to +0.0; the reference's order there is that of an unstable sort, so ties are defined here and excluded from reference parity).  A
detection whose class is not an integer in 0 .. nc - 1 is ignored.  With nt the class's label count and tpc[i, t] the running count of true
positives at rank i: recall = tpc / (nt + 1e-16), precision = tpc / i; mrec = [0, recall, 1], mpre = [1, precision, 0] made non-increasing
from the right; ap[c, t] = the trapezoid sum over linspace(0, 1, 101) of interp(x, mrec, mpre); at threshold 0 over x = linspace(0, 1, 1000):
prec_values = interp(x, mrec, mpre), r_curve = interp(-x, -conf, recall, left=0), p_curve = interp(-x, -conf, precision, left=1).  interp is
`np.interp`: with repeated abscissae the LAST index j with xp[j] <= x, fp[j] where x == xp[j] (tests/ap_oracle.py states the reference's
procedure and this rule and compares them).  Confidences are taken as fp32, what the validator accumulates.

Device arrays go through `mgaap_run`: a radix sort, two scans per threshold and one workgroup per class, no host synchronisation and no
allocation, so `post.run(); match.run(); ap.run()` is one captured chain, and `results()` reads back 8 * nc * (niou + 3001) bytes instead of
the run's rows.  Host arrays take `_host_ap`, the same rule in numpy with a stable sort.  What is O(nc * 1000) -- f1_curve, the smoothed
maximum, p, r, f1, tp, fp at it, unique_classes -- is done on the host in numpy for both.

Not built: `nt_per_image` (the unique image / class pairs stay `DetMatchPlan.stats()`'s), the `continuous` AP method, the segment / pose /
OBB metric classes, more than 1024 classes (`_lib.AP_MAX_NC`), an eps other than 1e-16 on the device.
"""
from __future__ import annotations

import ctypes as C
import warnings
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._binding import call, fill_ap
from .detlabels import sized_ws
from .detmaps import raise_on_status
from .detmatch import DetMatchPlan

EPS = 1e-16


def grids() -> Tuple[np.ndarray, np.ndarray]:
    """The two abscissa grids, as the doubles np.linspace gives: the kernels get these very arrays."""
    return np.linspace(0, 1, _lib.AP_POINTS), np.linspace(0, 1, _lib.AP_CURVE_POINTS)


def _numpy(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _tp2d(tp) -> np.ndarray:
    tp = _numpy(tp)
    if tp.ndim != 2:
        raise ValueError(f"ap_per_class: tp must be (n, niou), got {tp.shape}")
    return tp


def _size_nc(target_cls: np.ndarray) -> int:
    """nc from the targets: the largest class + 1 (at least 1)"""
    t = target_cls[np.isfinite(target_cls)] if target_cls.size else target_cls
    return max(int(t.max()) + 1, 1) if t.size else 1


# ---------------------------------------------------------------------------------------------------------------------------
# numpy (host arrays): the project's own statement of the rule
# ---------------------------------------------------------------------------------------------------------------------------
def _interp(x, xp, fp, left=None):
    """np.interp's index rule, stated: j = the last index with xp[j] <= x; fp[j] at the last index or where x == xp[j]; the left value
    below xp[0]; else slope * (x - xp[j]) + fp[j], each operation rounded once."""
    last = len(xp) - 1
    j = np.searchsorted(xp, x, side="right") - 1
    jc = np.clip(j, 0, last)
    j1 = np.minimum(jc + 1, last)
    with np.errstate(divide="ignore", invalid="ignore"):
        val = (fp[j1] - fp[jc]) / (xp[j1] - xp[jc]) * (x - xp[jc]) + fp[jc]
    out = np.where((jc == last) | (xp[jc] == x), fp[jc], val)
    out[j < 0] = fp[0] if left is None else left
    return out


def _host_curves(tp, conf, pred_cls, target_cls, nc: int, eps: float = EPS) -> Dict[str, np.ndarray]:
    """The rule in numpy, dense over the nc classes as mgaap_run's result block: ap (nc, niou), p_curve, r_curve, prec_values (nc, 1000),
    nt, n_det (nc).  A target class that is not an integer in 0 .. nc - 1 or a NaN confidence raises (the library's status 3 and 4)."""
    tp, conf = _tp2d(tp) != 0, _numpy(conf).astype(np.float32).reshape(-1)
    pred_cls, target_cls = _numpy(pred_cls).astype(np.float64).reshape(-1), _numpy(target_cls).astype(np.float64).reshape(-1)
    niou = tp.shape[1]
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(target_cls) & (target_cls == np.floor(target_cls)) & (target_cls >= 0) & (target_cls < nc))
    if bad.any():
        raise ValueError(f"ap_per_class: a target class is not an integer in 0 .. {nc - 1}")
    if np.isnan(conf).any():
        raise ValueError("ap_per_class: a confidence is NaN")
    nt = np.bincount(target_cls.astype(np.int64), minlength=nc).astype(np.int32)
    with np.errstate(invalid="ignore"):
        counted = np.isfinite(pred_cls) & (pred_cls == np.floor(pred_cls)) & (pred_cls >= 0) & (pred_cls < nc)
    rows = np.nonzero(counted)[0]
    neg = -(conf[rows].astype(np.float64) + 0.0)                             # -0.0 + 0.0 = +0.0: the two zeros compare equal either way
    rows = rows[np.argsort(neg, kind="stable")]
    rows = rows[np.argsort(pred_cls[rows], kind="stable")]                    # class, then descending confidence, then accumulation order
    n_det = np.bincount(pred_cls[rows].astype(np.int64), minlength=nc).astype(np.int32)
    first = np.concatenate(([0], np.cumsum(n_det)))
    x101, x1000 = grids()
    out = dict(ap=np.zeros((nc, niou)), p_curve=np.zeros((nc, x1000.size)), r_curve=np.zeros((nc, x1000.size)),
               prec_values=np.zeros((nc, x1000.size)), nt=nt, n_det=n_det)
    for c in np.nonzero((nt > 0) & (n_det > 0))[0]:
        r = rows[first[c]:first[c + 1]]
        tpc = np.cumsum(tp[r].astype(np.int64), 0).astype(np.float64)
        recall = tpc / (float(nt[c]) + eps)
        precision = tpc / np.arange(1, r.size + 1, dtype=np.float64)[:, None]
        xp = -(conf[r].astype(np.float64) + 0.0)
        out["r_curve"][c] = _interp(-x1000, xp, recall[:, 0], left=0.0)
        out["p_curve"][c] = _interp(-x1000, xp, precision[:, 0], left=1.0)
        for t in range(niou):
            mrec = np.concatenate(([0.0], recall[:, t], [1.0]))
            mpre = np.concatenate(([1.0], precision[:, t], [0.0]))
            mpre = np.maximum.accumulate(mpre[::-1])[::-1]
            y = _interp(x101, mrec, mpre)
            out["ap"][c, t] = np.cumsum((x101[1:] - x101[:-1]) * (y[1:] + y[:-1]) / 2.0)[-1]       # the terms added in ascending order
            if t == 0:
                out["prec_values"][c] = _interp(x1000, mrec, mpre)
    return out


def _box_mean(y: np.ndarray, f: float = 0.1) -> np.ndarray:
    """The box-filtered mean the reference picks the operating point from: a box of nf = round(2 f n) // 2 + 1 samples, the curve's ends
    continued by their own value for nf // 2 samples."""
    nf = round(len(y) * f * 2) // 2 + 1
    half = nf // 2
    padded = np.concatenate((np.full(half, y[0]), y, np.full(half, y[-1])))
    return np.convolve(padded, np.ones(nf) / nf, mode="valid")


def _finish(dense: Dict[str, np.ndarray], eps: float = EPS) -> tuple:
    """The dense per-class arrays -> the reference's 12-tuple: tp, fp, p, r, f1, ap, unique_classes, p_curve, r_curve, f1_curve, x,
    prec_values.  The rows are those of the classes with labels, ascending (np.unique(target_cls)); prec_values has a row per class with
    labels AND detections (one row of zeros if there is none), as the reference's list has."""
    nt_all, n_det = dense["nt"], dense["n_det"]
    keep = np.nonzero(nt_all > 0)[0]
    nt = nt_all[keep].astype(np.int64)
    ap, p_curve, r_curve = dense["ap"][keep], dense["p_curve"][keep], dense["r_curve"][keep]
    both = np.nonzero((nt_all > 0) & (n_det > 0))[0]
    prec_values = dense["prec_values"][both] if both.size else np.zeros((1, _lib.AP_CURVE_POINTS))
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    with warnings.catch_warnings(), np.errstate(invalid="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)                      # no class at all: the mean of an empty slice, as in the reference
        i = int(_box_mean(f1_curve.mean(0), 0.1).argmax())
    p, r, f1 = p_curve[:, i], r_curve[:, i], f1_curve[:, i]
    tp = (r * nt).round()
    fp = (tp / (p + eps) - tp).round()
    return tp, fp, p, r, f1, ap, keep.astype(int), p_curve, r_curve, f1_curve, grids()[1], prec_values


def _host_ap(tp, conf, pred_cls, target_cls, nc: Optional[int] = None, eps: float = EPS) -> tuple:
    """The whole of ap_per_class on the host: the rule in numpy, then the finish."""
    target = _numpy(target_cls).astype(np.float64).reshape(-1)
    return _finish(_host_curves(tp, conf, pred_cls, target, _size_nc(target) if nc is None else int(nc), eps), eps)


# ---------------------------------------------------------------------------------------------------------------------------
# HIP path
# ---------------------------------------------------------------------------------------------------------------------------
class _ApState:
    """The buffers of one average-precision call and its descriptor.  acc: rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state
    as DetMatchPlan holds them."""

    def __init__(self, acc, nc: int):
        rows_tp = acc[0]
        dev = rows_tp.device
        self.nc, self.niou = int(nc), int(rows_tp.shape[1])
        self.layout = _lib.ap_result_layout(self.nc, self.niou)
        g101, g1000 = grids()
        self.grid_ap, self.grid_curve = torch.from_numpy(g101).to(dev), torch.from_numpy(g1000).to(dev)
        self.result = torch.empty(self.layout["total"], dtype=torch.uint8, device=dev)
        self.status = torch.empty(1, dtype=torch.int32, device=dev)
        self.args = (*acc, self.nc, self.grid_ap, self.grid_curve, self.result, self.status)
        self.desc, self.ws = sized_ws(_lib.ApDesc(), fill_ap, _lib.ap_ws_bytes, self.args, dev)

    def run(self, dev):
        call("mgaap_run", dev, C.byref(self.desc))

    def dense(self) -> Dict[str, np.ndarray]:
        """One read-back of the result block, cut into its arrays."""
        host = self.result.cpu().numpy()
        out = {}
        for name, where in self.layout.items():
            if name != "total":
                o, shape, dt = where
                out[name] = host[o:o + int(np.prod(shape)) * int(dt[1])].view(dt).reshape(shape)
        return out


_STATUS = {3: "ap_per_class: a target class is not a finite integer in 0 .. nc - 1; the result is NaN",
           4: "ap_per_class: a confidence is NaN; the result is NaN"}


def ap_per_class(tp, conf, pred_cls, target_cls, *, nc: Optional[int] = None, eps: float = EPS) -> tuple:
    """The reference's ap_per_class.  `tp` (n, niou) bool or 0 / 1, `conf` (n), `pred_cls` (n), `target_cls` (m): tensors or numpy arrays,
    all on the GPU or all on the host.  `nc`: the number of classes (at most 1024 on the device); None sizes it from the targets with one
    host read.  Returns the reference's 12-tuple as numpy arrays: tp, fp, p, r, f1, ap, unique_classes, p_curve, r_curve, f1_curve, x,
    prec_values.  A detection of a class without labels, or whose class is not an integer in 0 .. nc - 1, is ignored, as the reference
    never visits it; a target class outside 0 .. nc - 1 or a NaN confidence raises."""
    arrays = (tp, conf, pred_cls, target_cls)
    on_gpu = [isinstance(a, torch.Tensor) and a.is_cuda for a in arrays]
    if not any(on_gpu):
        return _host_ap(tp, conf, pred_cls, target_cls, nc, eps)
    if not all(on_gpu):
        raise RuntimeError("ap_per_class: the arrays must all live on the GPU or all on the host")
    if eps != EPS:
        raise ValueError(f"ap_per_class: eps={eps}; the device rule fixes it at {EPS}")
    if tp.dim() != 2:
        raise ValueError(f"ap_per_class: tp must be (n, niou), got {tuple(tp.shape)}")
    dev = tp.device
    target = target_cls.reshape(-1).to(torch.float32)
    if nc is None:
        nc = _size_nc(target.cpu().numpy())
    n, m, niou = tp.shape[0], target.numel(), tp.shape[1]
    f32, i32 = torch.float32, torch.int32
    rows_tp = torch.zeros(max(n, 1), niou, dtype=torch.uint8, device=dev)
    rows_conf, rows_cls = torch.zeros(max(n, 1), dtype=f32, device=dev), torch.zeros(max(n, 1), dtype=f32, device=dev)
    tgt = torch.zeros(max(m, 1), dtype=f32, device=dev)
    rows_tp[:n], rows_conf[:n], rows_cls[:n], tgt[:m] = tp != 0, conf.reshape(-1).to(f32), pred_cls.reshape(-1).to(f32), target
    state = torch.tensor([n, m, 0, 0], dtype=i32, device=dev)
    st = _ApState((rows_tp, rows_conf, rows_cls, None, tgt, None, state), int(nc))
    st.run(dev)
    raise_on_status(st.status, _STATUS)
    return _finish(st.dense(), eps)


class DetApPlan:
    """Average precision on static buffers, behind a DetMatchPlan's accumulation, which it reads in place: run() may follow match.run() in
    a captured graph or be called once at the end of a validation run; it allocates nothing and reads nothing back.  Read `status` outside
    the capture (check_status); results() makes one read-back of the result block and does the numpy finish."""

    def __init__(self, match: DetMatchPlan, nc: int):
        if match._arena is None:
            raise RuntimeError("DetApPlan: the DetMatchPlan was created without rows_cap / tgt_cap, there is no accumulation")
        self.device, self.nc, self.match = match.device, int(nc), match
        a, cuts, f32, i32 = match._arena, match._cuts, torch.float32, torch.int32
        w = [a[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]
        rows_tp = a[cuts[-1]:].view(match.rows_cap, match.niou)
        self._st = _ApState((rows_tp, w[1].view(f32), w[2].view(f32), w[3].view(i32), w[4].view(f32), w[5].view(i32), w[0].view(i32)), self.nc)
        self.status, self.result = self._st.status, self._st.result

    @classmethod
    def create(cls, match: DetMatchPlan, *, nc: int):
        _lib.load()
        if not 1 <= int(nc) <= _lib.AP_MAX_NC:
            raise ValueError(f"DetApPlan: nc={nc} (1 .. {_lib.AP_MAX_NC})")
        return cls(match, int(nc))

    def run(self):
        self._st.run(self.device)

    def check_status(self):
        """Raise if the last run met a target class outside 0 .. nc - 1 or a NaN confidence (a host read: not inside a capture)."""
        raise_on_status(self.status, _STATUS)

    def _dense(self) -> Dict[str, np.ndarray]:
        d = self._st.dense()
        if d["nt"].size and d["nt"][0] < 0:
            raise RuntimeError("DetApPlan: the last run ended with a non-zero status and its result is NaN (check_status names the cause)")
        return d

    def results(self) -> tuple:
        """The reference's 12-tuple from the last run().  One read-back."""
        return _finish(self._dense())

    def box_results(self) -> tuple:
        """results()[2:]: what the reference's Metric.update takes."""
        return self.results()[2:]

    @property
    def nt_per_class(self) -> np.ndarray:
        """The label rows of each of the nc classes, as the last run() counted them (one read-back)."""
        return self._dense()["nt"].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's ap_per_class (install(ap=True))
# ---------------------------------------------------------------------------------------------------------------------------
def reference_replacement(module):
    """A function with the reference's signature for `module` (one of its ultralytics.utils.metrics module objects): the arrays go to the GPU
    when there is one, and with plot=True the module's OWN plot_pr_curve / plot_mc_curve, looked up when called, draw the results.  What
    the device does not take -- more than 1024 classes, another eps -- runs the same rule on the host."""

    def ap_per_class_(tp, conf, pred_cls, target_cls, plot=False, on_plot=None, save_dir=Path(), names={}, eps=EPS, prefix=""):
        arrays = [_tp2d(tp), _numpy(conf), _numpy(pred_cls), _numpy(target_cls)]
        nc = _size_nc(arrays[3].astype(np.float64).reshape(-1))
        if torch.cuda.is_available() and eps == EPS and nc <= _lib.AP_MAX_NC:
            arrays = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
        out = ap_per_class(*arrays, nc=nc, eps=eps)
        if plot:
            ap, classes, p_curve, r_curve, f1_curve, x, prec_values = out[5:]
            shown = {i: names[k] for i, k in enumerate(classes) if k in names}
            module.plot_pr_curve(x, prec_values, ap, save_dir / f"{prefix}PR_curve.png", shown, on_plot=on_plot)
            for curve, stem, label in ((f1_curve, "F1", "F1"), (p_curve, "P", "Precision"), (r_curve, "R", "Recall")):
                module.plot_mc_curve(x, curve, save_dir / f"{prefix}{stem}_curve.png", shown, ylabel=label, on_plot=on_plot)
        return out

    ap_per_class_.__name__ = ap_per_class_.__qualname__ = "ap_per_class"
    ap_per_class_._mga_replacement = True
    return ap_per_class_
