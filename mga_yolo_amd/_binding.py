"""The torch side of the binding: the one place where tensors become C-ABI level structs (include/mgacbam.h, include/mgaspade.h) and
where a library entry point is called on torch's current stream.  One fill function per struct sets EVERY field of it; the autograd
Functions (functional.py, segloss.py) and the static plans (plan.py, slice.py) all build their level tables here and differ only in the
arguments they pass.  Sizes are asked in _lib.py (`_lib.size`).  The four feature blocks are described once more, as a `Family` each
(CBAM, ECA, HEAD, SPADE at the end of this file): structs, layout flag, byte counts, fills, entry points and parameter names, which the eager
frame and the plans read instead of restating them."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib

DTYPES = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}    # element type -> ABI code


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# ---- library calls
def raw_stream(dev: torch.device) -> int:
    """hipStream_t of torch's current stream on `dev` (the private accessor is ~10x cheaper than building a Stream object: this
    sits on the eager path's per-call critical path)."""
    try:
        return torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device())
    except AttributeError:
        return torch.cuda.current_stream(dev).cuda_stream


class on_device:
    """`with torch.cuda.device(dev)` only when dev is not already current (the common case costs one integer compare)."""
    __slots__ = ("dev", "guard")

    def __init__(self, dev):
        self.dev, self.guard = dev, None

    def __enter__(self):
        idx = self.dev.index
        if idx is not None and idx != torch.cuda.current_device():
            self.guard = torch.cuda.device(self.dev)
            self.guard.__enter__()

    def __exit__(self, *a):
        if self.guard is not None:
            self.guard.__exit__(*a)


def call(name: str, dev: torch.device, *args) -> None:
    """Entry point `name`(*args, stream) on the stream that is current on `dev` NOW (looked up on every call: the caller may be inside
    torch.cuda.stream(...)); a non-zero return code raises with the entry point's name."""
    with on_device(dev):
        rc = getattr(_lib.load(), name)(*args, raw_stream(dev))
    if rc:
        _lib.check(rc, name)


# ---- MaskCBAM
def cbam_params(params: Sequence[torch.Tensor], cfg) -> _lib.Params:
    w1, b1, w2, b2, wsa, beta = params
    return _lib.Params(w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), wsa.data_ptr(), beta.data_ptr(),
                       cfg.hidden, cfg.k, int(cfg.use_sigmoid_mask), cfg.tiny_thr, cfg.eps)


def fill_cbam_fwd(L: _lib.FwdLevel, x, mask, y, ctx, params, cfg, flags: int = 0, ws=None) -> None:
    """flags: LAYOUT_NHWC (x, y channels_last; needs ws, the per-chunk pooling partials) | FWD_SAVE_PROJ."""
    B, Cc, H, W = x.shape
    L.x, L.mask, L.y, L.ctx, L.ctx_bytes = x.data_ptr(), _ptr(mask), y.data_ptr(), ctx.data_ptr(), ctx.numel()
    L.p = cbam_params(params, cfg)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags
    L.ws, L.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


def fill_cbam_bwd(L: _lib.BwdLevel, x, mask, gy, ctx, scratch, gx, gmask, pgrads, params, cfg, flags: int = 0) -> None:
    """pgrads: (gw1, gb1, gw2, gb2, gwsa, gbeta); flags: LAYOUT_NHWC | BWD_HAVE_PROJ."""
    B, Cc, H, W = x.shape
    L.x, L.mask, L.gy, L.ctx, L.scratch = x.data_ptr(), _ptr(mask), gy.data_ptr(), ctx.data_ptr(), scratch.data_ptr()
    L.ctx_bytes, L.scratch_bytes = ctx.numel(), scratch.numel()
    L.gx, L.gmask = gx.data_ptr(), _ptr(gmask)
    L.gw1, L.gb1, L.gw2, L.gb2, L.gwsa, L.gbeta = (t.data_ptr() for t in pgrads)
    L.p = cbam_params(params, cfg)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags


# ---- MaskECA
def eca_params(w, beta, cfg) -> _lib.EcaParams:
    return _lib.EcaParams(w.data_ptr(), beta.data_ptr(), cfg.k, int(cfg.use_sigmoid_mask), cfg.tiny_thr, cfg.eps)


def fill_eca_fwd(L: _lib.EcaFwdLevel, x, mask, y, ctx, w, beta, cfg, flags: int = 0) -> None:
    B, Cc, H, W = x.shape
    L.x, L.mask, L.y, L.ctx, L.ctx_bytes = x.data_ptr(), _ptr(mask), y.data_ptr(), ctx.data_ptr(), ctx.numel()
    L.p = eca_params(w, beta, cfg)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags


def fill_eca_bwd(L: _lib.EcaBwdLevel, x, mask, gy, ctx, scratch, gx, gmask, gw, gbeta, w, beta, cfg, flags: int = 0) -> None:
    B, Cc, H, W = x.shape
    L.x, L.mask, L.gy, L.ctx, L.scratch = x.data_ptr(), _ptr(mask), gy.data_ptr(), ctx.data_ptr(), scratch.data_ptr()
    L.ctx_bytes, L.scratch_bytes = ctx.numel(), scratch.numel()
    L.gx, L.gmask, L.gw, L.gbeta = gx.data_ptr(), _ptr(gmask), gw.data_ptr(), gbeta.data_ptr()
    L.p = eca_params(w, beta, cfg)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags


# ---- MGAMaskHead
def head_params(w1, gamma, beta, rmean, rvar, nbt, wh, bh, hidden, eps, momentum, training) -> _lib.HeadParams:
    return _lib.HeadParams(w1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), _ptr(nbt),
                           wh.data_ptr(), bh.data_ptr(), hidden, eps, momentum, int(training))


def fill_head_fwd(L: _lib.HeadFwdLevel, x, logits, ctx, params, running, hidden, eps, momentum, training, flags: int = 0) -> None:
    """params: (proj.0.weight, proj.1.weight, proj.1.bias, head.weight, head.bias); running: (running_mean, running_var,
    num_batches_tracked | None); flags: HEAD_LAYOUT_NHWC | HEAD_LOGITS_F32."""
    B, Cc, H, W = x.shape
    L.x, L.logits, L.ctx, L.ctx_bytes = x.data_ptr(), logits.data_ptr(), ctx.data_ptr(), ctx.numel()
    L.p = head_params(*params[:3], *running, *params[3:], hidden, eps, momentum, training)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags


def fill_head_bwd(L: _lib.HeadBwdLevel, x, g_logits, g_logits2, ctx, scratch, gx, pgrads, params, running, hidden, eps, momentum,
                  training, flags: int = 0) -> None:
    """g_logits2: a second dL/dlogits summed while the backward loads them (slice.SlicePlan: MaskCBAM's dL/dmask), or None;
    pgrads: gradients in the order of params; flags: HEAD_LAYOUT_NHWC | HEAD_BWD_ACCUM_GX | HEAD_LOGITS_F32.  The backward never
    counts a batch: its parameter struct carries no num_batches_tracked, whatever `running` holds."""
    B, Cc, H, W = x.shape
    L.x, L.g_logits, L.g_logits2 = x.data_ptr(), g_logits.data_ptr(), _ptr(g_logits2)
    L.ctx, L.scratch, L.gx = ctx.data_ptr(), scratch.data_ptr(), gx.data_ptr()
    L.ctx_bytes, L.scratch_bytes = ctx.numel(), scratch.numel()
    L.gw1, L.gbn_weight, L.gbn_bias, L.gwh, L.gbh = (t.data_ptr() for t in pgrads)
    L.p = head_params(*params[:3], running[0], running[1], None, *params[3:], hidden, eps, momentum, training)
    L.B, L.C, L.H, L.W, L.dtype, L.flags = B, Cc, H, W, DTYPES[x.dtype], flags


# ---- segmentation loss
def fill_seg(L: _lib.SegLevel, logits, target, glogits, scale_weight: float, resize: int) -> None:
    """logits (B,1,H,W), target (B,1,Ht,Wt) fp32; glogits: where the backward writes dL/dlogits, None in a forward-only table."""
    B, _, H, W = logits.shape
    L.logits, L.target, L.glogits = logits.data_ptr(), target.data_ptr(), _ptr(glogits)
    L.B, L.H, L.W, L.Ht, L.Wt = B, H, W, target.shape[-2], target.shape[-1]
    L.dtype, L.scale_weight, L.resize = DTYPES[logits.dtype], scale_weight, resize


# ---- MaskSPADE: one struct for both directions
_SPADE_P = ("w0", "b0", "wg", "bg", "wb", "bb")


def fill_spade(L: _lib.SpadeLevel, x, mask, params, cfg, running, ctx, y=None, save_gamma: bool = False,
               gy=None, gx=None, gmask=None, pgrads=None, scratch=None, flags: int = 0) -> None:
    """params / pgrads: six tensors, or six None for a level without a mask; running: (running_mean, running_var, num_batches_tracked),
    read for norm_type 'bn' only.  Forward passes y and save_gamma, backward gy, gx, gmask, pgrads and scratch.  flags: 0, or
    _lib.SPADE_LAYOUT_NHWC when x / y / gy / gx are channels_last (x.shape stays (B,C,H,W)); a backward carries its forward's flag."""
    B, Cc, H, W = x.shape
    L.x, L.mask, L.y, L.gy, L.gx, L.gmask = x.data_ptr(), _ptr(mask), _ptr(y), _ptr(gy), _ptr(gx), _ptr(gmask)
    if mask is None:                                     # a level without a mask reads no parameter and writes no parameter gradient
        params = pgrads = (None,) * 6
    for name, p, g in zip(_SPADE_P, params, pgrads or (None,) * 6):
        setattr(L, name, _ptr(p))
        setattr(L, "g" + name, _ptr(g))
    rm, rv, nbt = running if cfg.bn else (None, None, None)
    L.running_mean, L.running_var, L.num_batches_tracked = _ptr(rm), _ptr(rv), _ptr(nbt)
    L.ctx, L.ctx_bytes = ctx.data_ptr(), ctx.numel()
    L.scratch, L.scratch_bytes = (None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel())
    L.B, L.C, L.H, L.W, L.hidden, L.dtype = B, Cc, H, W, cfg.hidden, DTYPES[x.dtype]
    L.norm_type, L.training = (_lib.NORM_BN if cfg.bn else _lib.NORM_IN), int(cfg.training)
    L.use_sigmoid_mask, L.save_gamma, L.eps, L.momentum, L.flags = int(cfg.use_sigmoid_mask), int(save_gamma), cfg.eps, cfg.momentum, int(flags)


# ---- the mask resample of the static plans (include/mgaresample.h): one struct for both directions
def fill_resample(L: _lib.ResampleLevel, src, dst, in_hw, out_hw) -> None:
    """in_hw / out_hw: the sizes of the FORWARD's source and destination in both directions.  Forward: src (B,1,*in_hw) -> dst (B,1,*out_hw);
    backward: src = dL/d(forward dst) (B,1,*out_hw), dst = dL/d(forward src) (B,1,*in_hw)."""
    L.src, L.dst, L.B = src.data_ptr(), dst.data_ptr(), src.shape[0]
    (L.in_h, L.in_w), (L.out_h, L.out_w) = in_hw, out_hw


# ---- ProbMaskGater on a pyramid (include/mgagate.h): one struct for both directions
def fill_gate(L: _lib.GateLevel, p, out, msoft, gout, gp, mode: int, stream_id: int, tau: float, p_min: float, threshold: float) -> None:
    """p: the gate's fp32 input; forward passes out (and msoft for the two soft modes), backward gout, gp (and that msoft); mode: _lib.GATE_*."""
    L.p, L.out, L.msoft, L.gout, L.gp = p.data_ptr(), _ptr(out), _ptr(msoft), _ptr(gout), _ptr(gp)
    L.n, L.mode, L.stream_id = p.numel(), int(mode), int(stream_id)
    L.tau, L.p_min, L.threshold = float(tau), float(p_min), float(threshold)


# ---- the fused optimizer step (include/mgaopt.h)
def fill_opt_segment(S: _lib.OptSegment, param, grad, state0, state1, ema, group: int) -> None:
    """param: the fp32 tensor updated in place; grad: its gradient (a view into the bucket or the accumulator), None for an EMA-only segment;
    state0 / state1: SGD's momentum buffer / AdamW's exp_avg, exp_avg_sq; ema: the average or None; group: 0 biases, 1 decayed, 2 norm weights."""
    S.param, S.grad, S.state0, S.state1, S.ema = param.data_ptr(), _ptr(grad), _ptr(state0), _ptr(state1), _ptr(ema)
    S.n, S.group, S.reserved = param.numel(), int(group), 0


# ---- the multi-scale segmentation targets (include/mgatargets.h)
TGT_SRC = {torch.uint8: _lib.TGT_SRC_U8, torch.float32: _lib.TGT_SRC_F32}


def fill_targets(D: _lib.TargetsDesc, src, dsts, strides, method: int, flags: int = 0, scratch=None) -> None:
    """src: (B,H,W) contiguous uint8 or fp32; dsts: per stride the (B,1,ceil(H/s),ceil(W/s)) fp32 tensor that is written; method:
    _lib.TGT_AVGPOOL | TGT_MAXPOOL; flags: 0 | _lib.TGT_CLOSE3, which needs scratch (uint8, _lib.targets_scratch_bytes of the filled struct:
    fill once without it to ask, then again with it)."""
    B, H, W = src.shape
    D.src = src.data_ptr()
    for l in range(_lib.TGT_MAX_LEVELS):
        on = l < len(dsts)
        D.dst[l], D.stride[l] = (dsts[l].data_ptr(), int(strides[l])) if on else (None, 0)
    D.n_levels, D.B, D.H, D.W = len(dsts), B, H, W
    D.src_dtype, D.method, D.flags, D.reserved = TGT_SRC[src.dtype], int(method), int(flags), 0
    D.scratch, D.scratch_bytes = (None, 0) if scratch is None else (scratch.data_ptr(), scratch.numel())


# ---- the Detect maps of the two descriptors below (detmaps.py, csrc/detmaps.cuh)
def fill_maps(D, feats, strides, max_levels: int) -> None:
    """feats, H, W and stride of every level (NULL and 0 past the last map) and n_levels."""
    for l in range(max_levels):
        on = l < len(feats)
        D.feats[l] = feats[l].data_ptr() if on else None
        D.H[l], D.W[l], D.stride[l] = (feats[l].shape[2], feats[l].shape[3], int(strides[l])) if on else (0, 0, 0)
    D.n_levels = len(feats)


# ---- the detection criterion (include/mgadet.h): one struct for both directions
def fill_det(D: _lib.DetDesc, feats, strides, nc: int, topk: int, m_cap: int, gains, batch_idx, cls, bboxes, n, assign_gt, assign_score,
             out, items, status, ws=None, g_feats=None, upstream=None) -> None:
    """feats: the Detect maps (B, 64 + nc, H_l, W_l), NCHW contiguous, one element type; batch_idx / cls (n_cap) and bboxes (n_cap, 4)
    fp32; n: the int32 device word of live rows or None (= n_cap); assign_gt int32 / assign_score fp32 (B, A), out / items fp32 (3) and
    status int32 (1) are written by the forward.  The backward passes g_feats and upstream (3, fp32) as well, and the forward's ws
    (uint8, _lib.det_ws_bytes of the filled struct: fill once without it to ask, then again with it)."""
    fill_maps(D, feats, strides, _lib.DET_MAX_LEVELS)
    for l in range(_lib.DET_MAX_LEVELS):
        D.g_feats[l] = g_feats[l].data_ptr() if l < len(feats) and g_feats is not None else None
    D.B, D.nc, D.reg_max = feats[0].shape[0], int(nc), _lib.DET_REG_MAX
    D.dtype, D.topk, D.n_cap, D.m_cap = DTYPES[feats[0].dtype], int(topk), batch_idx.shape[0], int(m_cap)
    D.gains[0], D.gains[1], D.gains[2] = (float(g) for g in gains)
    D.reserved = 0
    has = batch_idx.shape[0] > 0
    D.batch_idx, D.cls, D.bboxes = (batch_idx.data_ptr(), cls.data_ptr(), bboxes.data_ptr()) if has else (None, None, None)
    D.n = _ptr(n)
    D.assign_gt, D.assign_score, D.out, D.items, D.status = (t.data_ptr() for t in (assign_gt, assign_score, out, items, status))
    D.upstream = _ptr(upstream)
    D.ws, D.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


# ---- the detection post-process (include/mganms.h)
def fill_nms(D: _lib.NmsDesc, feats, pred, strides, nc: int, conf_thres: float, iou_thres: float, max_det: int, max_nms: int, flags: int,
             cand_cap: int, dets, count, keep, status, ws=None) -> None:
    """Exactly one of feats (the Detect maps (B, 64 + nc, H_l, W_l), NCHW contiguous, one element type, with their strides) and pred (the
    decoded (B, 4 + nc, A) tensor) is given, the other is None; dets fp32 (B, max_det, 6), count int32 (B), keep int32 (B, max_det) and
    status int32 (1) are written; flags: _lib.NMS_MULTI_LABEL | _lib.NMS_AGNOSTIC; ws: uint8, _lib.nms_ws_bytes of the filled struct (fill
    once without it to ask, then again with it), zero-filled once before its first call."""
    feats = list(feats) if feats is not None else []
    fill_maps(D, feats, strides, _lib.NMS_MAX_LEVELS)
    src = feats[0] if feats else pred
    D.pred = _ptr(pred)
    D.A, D.B, D.nc = (0 if feats else pred.shape[2]), src.shape[0], int(nc)
    D.dtype, D.max_det, D.max_nms, D.flags = DTYPES[src.dtype], int(max_det), int(max_nms), int(flags)
    D.conf_thres, D.iou_thres, D.cand_cap, D.reserved = float(conf_thres), float(iou_thres), int(cand_cap), 0
    D.dets, D.count, D.keep, D.status = (t.data_ptr() for t in (dets, count, keep, status))
    D.ws, D.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())


# ---- detections matched to labels (include/ext/mgamatch.h)
def fill_match(D: _lib.MatchDesc, dets, count, batch_idx, cls, bboxes, n, m_cap: int, img_w: float, img_h: float, iouv, flags: int,
               tp, best_iou, best_gt, status, acc=None, ws=None) -> None:
    """dets fp32 (B, max_det, 6) and count int32 (B) as mganms_run writes them; batch_idx / cls (n_cap) and bboxes (n_cap, 4) fp32; n: the
    int32 device word of live label rows or None (= n_cap); iouv: the thresholds as Python floats; flags: _lib.MATCH_SINGLE_CLS; tp uint8
    (B, max_det, niou), best_iou fp32 and best_gt int32 (B, max_det) and status int32 (1) are written.  acc: None, or the accumulation
    buffers (rows_tp uint8 (rows_cap, niou), rows_conf, rows_cls fp32 and rows_img int32 (rows_cap), tgt_cls fp32 and tgt_img int32
    (tgt_cap), state int32 (4)); ws: uint8, _lib.match_ws_bytes of the filled struct (fill once without it to ask, then again with it)."""
    D.dets, D.count = dets.data_ptr(), count.data_ptr()
    has = batch_idx.shape[0] > 0
    D.batch_idx, D.cls, D.bboxes = (batch_idx.data_ptr(), cls.data_ptr(), bboxes.data_ptr()) if has else (None, None, None)
    D.n = _ptr(n)
    D.B, D.max_det, D.n_cap, D.m_cap = dets.shape[0], dets.shape[1], batch_idx.shape[0], int(m_cap)
    D.img_w, D.img_h, D.niou, D.flags = float(img_w), float(img_h), len(iouv), int(flags)
    for t in range(_lib.MATCH_MAX_IOU):
        D.iouv[t] = float(iouv[t]) if t < len(iouv) else 0.0
    D.tp, D.best_iou, D.best_gt, D.status = (t.data_ptr() for t in (tp, best_iou, best_gt, status))
    rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state = acc if acc is not None else (None,) * 7
    D.rows_cap, D.tgt_cap = (rows_conf.shape[0], tgt_cls.shape[0]) if acc is not None else (0, 0)
    D.rows_tp, D.rows_conf, D.rows_cls, D.rows_img = _ptr(rows_tp), _ptr(rows_conf), _ptr(rows_cls), _ptr(rows_img)
    D.tgt_cls, D.tgt_img, D.state = _ptr(tgt_cls), _ptr(tgt_img), _ptr(state)
    D.ws, D.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
    D.reserved = 0


# ---- the validator's confusion matrix (include/ext/mgaconfusion.h)
def fill_confusion(D: _lib.ConfusionDesc, dets, count, batch_idx, cls, bboxes, n, m_cap: int, nc: int, flags: int, img_w: float, img_h: float,
                   conf_thres: float, iou_thres: float, det_out, lab_out, cm, acc, status, ws=None) -> None:
    """dets, count and the labels as fill_match takes them; n: the int32 device word of live label rows or None (= n_cap); flags:
    _lib.CM_SINGLE_CLS; conf_thres: what a counted detection's confidence exceeds (after detconfusion.reference_conf); det_out int32
    (B, max_det), lab_out int32 (n_cap), cm int32 (nc + 1, nc + 1) and status int32 (1) are written; acc: the run-long int64
    (nc + 1, nc + 1) matrix or None; ws: uint8, _lib.confusion_ws_bytes of the filled struct (fill once without it to ask, then again with it)."""
    D.dets, D.count = dets.data_ptr(), count.data_ptr()
    has = batch_idx.shape[0] > 0
    D.batch_idx, D.cls, D.bboxes, D.lab_out = (batch_idx.data_ptr(), cls.data_ptr(), bboxes.data_ptr(), lab_out.data_ptr()) if has else (None,) * 4
    D.n = _ptr(n)
    D.B, D.max_det, D.n_cap, D.m_cap, D.nc, D.flags = dets.shape[0], dets.shape[1], batch_idx.shape[0], int(m_cap), int(nc), int(flags)
    D.img_w, D.img_h, D.conf_thres, D.iou_thres = float(img_w), float(img_h), float(conf_thres), float(iou_thres)
    D.det_out, D.cm, D.acc, D.status = det_out.data_ptr(), cm.data_ptr(), _ptr(acc), status.data_ptr()
    D.ws, D.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
    D.reserved = 0


# ---- average precision per class from the accumulated rows (include/ext/mgaap.h)
def fill_ap(D: _lib.ApDesc, rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state, nc: int, grid_ap, grid_curve, result, status,
            ws=None) -> None:
    """The accumulation as fill_match's acc holds it: rows_tp uint8 (rows_cap, niou), rows_conf, rows_cls fp32 (rows_cap), tgt_cls fp32
    (tgt_cap), state int32 (4); rows_img and tgt_img int32 or None (they are not read); grid_ap fp64 (101) and grid_curve fp64 (1000): the
    two linspaces; result uint8, _lib.ap_result_layout(nc, niou)["total"] bytes, and status int32 (1) are written; ws: uint8,
    _lib.ap_ws_bytes of the filled struct (fill once without it to ask, then again with it)."""
    D.rows_tp, D.rows_conf, D.rows_cls, D.rows_img = rows_tp.data_ptr(), rows_conf.data_ptr(), rows_cls.data_ptr(), _ptr(rows_img)
    D.tgt_cls, D.tgt_img, D.state = tgt_cls.data_ptr(), _ptr(tgt_img), state.data_ptr()
    D.rows_cap, D.tgt_cap, D.niou, D.nc = rows_conf.shape[0], tgt_cls.shape[0], rows_tp.shape[1], int(nc)
    D.grid_ap, D.grid_curve, D.result, D.status = grid_ap.data_ptr(), grid_curve.data_ptr(), result.data_ptr(), status.data_ptr()
    D.ws, D.ws_bytes = (None, 0) if ws is None else (ws.data_ptr(), ws.numel())
    D.reserved = 0


# ---- a batch of uint8 images prepared in one launch (include/ext/mgaimage.h)
def fill_image(D: _lib.ImageDesc, src, dst, src_nhwc: bool = False, reverse_channels: bool = False) -> None:
    """src: uint8, contiguous, (B,C,H,W) or with src_nhwc (B,H,W,C); dst: (B,C,H',W') fp32 / fp16 / bf16, contiguous or channels_last (its
    strides say which: a destination that is both -- C = 1, or H' = W' = 1 -- is written as contiguous, the same bytes).  H', W' other than
    H, W: the bilinear resize."""
    B, Cc, oh, ow = dst.shape
    ih, iw = (src.shape[1], src.shape[2]) if src_nhwc else (src.shape[2], src.shape[3])
    D.src, D.dst = src.data_ptr(), dst.data_ptr()
    D.B, D.C, D.in_h, D.in_w, D.out_h, D.out_w = B, Cc, ih, iw, oh, ow
    D.dtype = DTYPES[dst.dtype]
    D.flags = (_lib.IMG_SRC_NHWC if src_nhwc else 0) | (0 if dst.is_contiguous() else _lib.IMG_DST_NHWC) | (_lib.IMG_REVERSE_C if reverse_channels else 0)
    D.reserved = 0


# ---- the feature-block families: what the eager frame (functional.py) and the static plans (plan.py, slice.py) both need of one
class Family(NamedTuple):
    """One block family.  ``shape`` = (B,C,H,W); ``cfg`` = the block's config dataclass, for the mask head the tuple (hidden, eps, momentum,
    training); ``flags`` = the level flags, of which the byte counts read the layout bit only.  The fills take a level's buffers BY NAME and
    use the ones their struct has: x, mask, y (the head's logits), ctx, ws, params, running, save_gamma forward; x, mask, gy (the head's
    dL/dlogits), gy2 (its second one, fill_head_bwd), ctx, scratch, gx, gmask, grads, params, running backward."""
    kind: str                                   # "cbam" | "eca" | "head" | "spade"
    fwd_level: type                             # the ctypes structs of the two level tables
    bwd_level: type
    layout_nhwc: int                            # the level flag of torch.channels_last features
    param_names: Tuple[str, ...]                # a level's parameters, in the order of the bucket (and of the state_dict's keys where dotted)
    fwd_entry: str                              # the two entry points: (levels, n[, stages], stream)
    bwd_entry: str
    ctx_bytes: Callable[[tuple, object, int], int]
    scratch_bytes: Callable[[tuple, object, int], int]
    ws_bytes: Callable[[tuple, object, int], int]      # the forward's workspace: 0 = none
    fill_fwd: Callable[..., None]               # (L, cfg, flags, **buffers)
    fill_bwd: Callable[..., None]


def spade_eager_ctx_bytes(shape, cfg, gamma_elem: int) -> int:
    """MaskSPADE's ctx on the eager path: the full mgaspade_ctx_bytes (SPADE.ctx_bytes, what a static plan allocates) keeps gamma as fp32;
    an eager forward keeps it at the feature's own element size ``gamma_elem``, or not at all (0: no backward will come, or no mask)."""
    B, Cc, H, W = shape
    a16 = lambda v: (v + 15) & ~15
    base = _lib.spade_ctx_bytes(B, Cc, H, W, cfg.hidden) - a16(B * Cc * H * W * 4)
    return base + (a16(B * Cc * H * W * gamma_elem) if gamma_elem else 0)


# (s, c, f = shape, cfg, flags; b = the level's buffers by name.  The fill_* signatures above are pinned: these lines only hand the names over)
CBAM = Family(
    "cbam", _lib.FwdLevel, _lib.BwdLevel, _lib.LAYOUT_NHWC, ("w1", "b1", "w2", "b2", "wsa", "beta"), "mgacbam_forward_stages", "mgacbam_backward_stages",
    lambda s, c, f: _lib.ctx_bytes(*s, c.hidden), lambda s, c, f: _lib.scratch_bytes(*s, c.hidden, c.k, f), lambda s, c, f: _lib.fwd_ws_bytes(*s, c.hidden, f),
    lambda L, c, f, **b: fill_cbam_fwd(L, b["x"], b["mask"], b["y"], b["ctx"], b["params"], c, f, b.get("ws")),
    lambda L, c, f, **b: fill_cbam_bwd(L, b["x"], b["mask"], b["gy"], b["ctx"], b["scratch"], b["gx"], b["gmask"], b["grads"], b["params"], c, f))
ECA = Family(
    "eca", _lib.EcaFwdLevel, _lib.EcaBwdLevel, _lib.LAYOUT_NHWC, ("conv1d.weight", "beta"), "mgacbam_eca_forward", "mgacbam_eca_backward",
    lambda s, c, f: _lib.eca_ctx_bytes(*s, f), lambda s, c, f: _lib.eca_scratch_bytes(*s, f), lambda s, c, f: 0,
    lambda L, c, f, **b: fill_eca_fwd(L, b["x"], b["mask"], b["y"], b["ctx"], *b["params"], c, f),
    lambda L, c, f, **b: fill_eca_bwd(L, b["x"], b["mask"], b["gy"], b["ctx"], b["scratch"], b["gx"], b["gmask"], *b["grads"], *b["params"], c, f))
HEAD = Family(
    "head", _lib.HeadFwdLevel, _lib.HeadBwdLevel, _lib.HEAD_LAYOUT_NHWC, ("proj.0.weight", "proj.1.weight", "proj.1.bias", "head.weight", "head.bias"),
    "mgahead_forward", "mgahead_backward",
    lambda s, c, f: _lib.head_ctx_bytes(*s, c[0], f), lambda s, c, f: _lib.head_scratch_bytes(*s, c[0], f), lambda s, c, f: 0,
    lambda L, c, f, **b: fill_head_fwd(L, b["x"], b["y"], b["ctx"], b["params"], b["running"], *c, f),
    lambda L, c, f, **b: fill_head_bwd(L, b["x"], b["gy"], b.get("gy2"), b["ctx"], b["scratch"], b["gx"], b["grads"], b["params"], b["running"], *c, f))
SPADE = Family(
    "spade", _lib.SpadeLevel, _lib.SpadeLevel, _lib.SPADE_LAYOUT_NHWC,
    ("shared.0.weight", "shared.0.bias", "conv_gamma.weight", "conv_gamma.bias", "conv_beta.weight", "conv_beta.bias"), "mgaspade_forward", "mgaspade_backward",
    lambda s, c, f: _lib.spade_ctx_bytes(*s, c.hidden), lambda s, c, f: _lib.spade_scratch_bytes(*s, c.hidden), lambda s, c, f: 0,
    lambda L, c, f, **b: fill_spade(L, b["x"], b["mask"], b["params"], c, b["running"], b["ctx"], y=b["y"], save_gamma=b["save_gamma"], flags=f),
    lambda L, c, f, **b: fill_spade(L, b["x"], b["mask"], b["params"], c, b["running"], b["ctx"], gy=b["gy"], gx=b["gx"], gmask=b["gmask"],
                                    pgrads=b["grads"], scratch=b["scratch"], flags=f))


