"""ctypes binding of libmgacbam.so (C ABI: the headers under include/, one record of HEADERS each).  There is NO fallback: if the library is missing
or an entry point is absent, loading raises -- device tensors never take another path."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import NamedTuple

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGACBAM_LIB") or os.path.join(_PKG, "libmgacbam.so")   # MGACBAM_LIB: A/B builds in tuning sweeps
ABI_VERSION = 15
MAX_LEVELS = 8
F32, F16, BF16 = 0, 1, 2
E_NULL, E_SHAPE, E_DTYPE, E_ALIGN, E_LEVELS, E_SIZE = -1, -2, -3, -4, -5, -6
E_ARG = -7         # include/mgatargets.h: an argument outside what the entry point takes
# stage bit masks (include/mgacbam.h)
FWD_STAGES = dict(pool=1, chan=2, apply=4)
BWD_STAGES = dict(reduce1=1, convT=2, reduce2=4, wsa=8, params=16, apply=32)
BWD_FUSE = 64
FWD_SAVE_PROJ, BWD_HAVE_PROJ, PROJ_MAX_HIDDEN = 1, 1, 4
LAYOUT_NHWC = 2   # level flag (MaskCBAM and MaskECA, forward and backward): x, y, gy, gx are (B,H,W,C) -- torch's channels_last
FWD_ALL, BWD_PARAMS, BWD_INPUTS, BWD_ALL = 7, 31, 32, 127
BWD_FOLD = 128   # with BWD_ALL: transposed conv folded into the k_bwd_reduce1 launch (ctx.sync zero-filled once by the caller)
FWD_FUSE = 8   # with FWD_ALL: one launch, in-launch hand-off through ctx.sync (caller zero-fills it once)

_c_float_p = C.POINTER(C.c_float)


class Params(C.Structure):                       # mgacbam_params_t
    _fields_ = [("w1", C.c_void_p), ("b1", C.c_void_p), ("w2", C.c_void_p), ("b2", C.c_void_p),
                ("wsa", C.c_void_p), ("beta", C.c_void_p),
                ("hidden", C.c_int32), ("k", C.c_int32), ("use_sigmoid_mask", C.c_int32),
                ("tiny_thr", C.c_float), ("eps", C.c_float)]


class FwdLevel(C.Structure):                     # mgacbam_fwd_level_t
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("y", C.c_void_p), ("ctx", C.c_void_p), ("ctx_bytes", C.c_size_t),
                ("p", Params), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_int32), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class BwdLevel(C.Structure):                     # mgacbam_bwd_level_t
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("gy", C.c_void_p), ("ctx", C.c_void_p),
                ("scratch", C.c_void_p), ("ctx_bytes", C.c_size_t), ("scratch_bytes", C.c_size_t), ("gx", C.c_void_p), ("gmask", C.c_void_p),
                ("gw1", C.c_void_p), ("gb1", C.c_void_p), ("gw2", C.c_void_p), ("gb2", C.c_void_p),
                ("gwsa", C.c_void_p), ("gbeta", C.c_void_p),
                ("p", Params), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_int32)]


class EcaParams(C.Structure):                    # mgacbam_eca_params_t
    _fields_ = [("w", C.c_void_p), ("beta", C.c_void_p), ("k", C.c_int32), ("use_sigmoid_mask", C.c_int32),
                ("tiny_thr", C.c_float), ("eps", C.c_float)]


class EcaFwdLevel(C.Structure):                  # mgacbam_eca_fwd_level_t
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("y", C.c_void_p), ("ctx", C.c_void_p), ("ctx_bytes", C.c_size_t), ("p", EcaParams),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_int32)]


class EcaBwdLevel(C.Structure):                  # mgacbam_eca_bwd_level_t
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("gy", C.c_void_p), ("ctx", C.c_void_p), ("scratch", C.c_void_p),
                ("ctx_bytes", C.c_size_t), ("scratch_bytes", C.c_size_t),
                ("gx", C.c_void_p), ("gmask", C.c_void_p), ("gw", C.c_void_p), ("gbeta", C.c_void_p), ("p", EcaParams),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_int32)]


CTX_FIELDS = ("S", "use", "den", "avg", "mx", "mavg", "valid", "amax", "h_avg", "h_mx", "ca", "planes", "cidx", "sa", "proj", "sync", "total", "status")


class CtxLayout(C.Structure):                    # mgacbam_ctx_layout_t
    _fields_ = [(n, C.c_int64) for n in CTX_FIELDS]


class SegLevel(C.Structure):                     # mgaseg_level_t
    _fields_ = [("logits", C.c_void_p), ("target", C.c_void_p), ("glogits", C.c_void_p),
                ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Ht", C.c_int32), ("Wt", C.c_int32),
                ("dtype", C.c_int32), ("scale_weight", C.c_float), ("resize", C.c_int32)]


class SegCfg(C.Structure):                       # mgaseg_cfg_t
    _fields_ = [("bce_weight", C.c_float), ("dice_weight", C.c_float), ("smooth", C.c_float), ("loss_lambda", C.c_float),
                ("use_unified_focal", C.c_int32), ("ufl_lambda", C.c_float), ("ufl_delta", C.c_float), ("ufl_gamma", C.c_float)]


SEG_MAX_LEVELS = 4
SEG_NEAREST, SEG_BILINEAR = 0, 1


class HeadParams(C.Structure):                   # mgahead_params_t
    _fields_ = [("w1", C.c_void_p), ("bn_weight", C.c_void_p), ("bn_bias", C.c_void_p), ("running_mean", C.c_void_p),
                ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p), ("wh", C.c_void_p), ("bh", C.c_void_p),
                ("hidden", C.c_int32), ("eps", C.c_float), ("momentum", C.c_float), ("training", C.c_int32)]


class HeadFwdLevel(C.Structure):                 # mgahead_fwd_level_t
    _fields_ = [("x", C.c_void_p), ("logits", C.c_void_p), ("ctx", C.c_void_p), ("ctx_bytes", C.c_size_t), ("p", HeadParams),
                ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("dtype", C.c_int32), ("flags", C.c_int32)]


class HeadBwdLevel(C.Structure):                 # mgahead_bwd_level_t
    _fields_ = [("x", C.c_void_p), ("g_logits", C.c_void_p), ("g_logits2", C.c_void_p), ("ctx", C.c_void_p), ("scratch", C.c_void_p),
                ("ctx_bytes", C.c_size_t), ("scratch_bytes", C.c_size_t), ("gx", C.c_void_p),
                ("gw1", C.c_void_p), ("gbn_weight", C.c_void_p), ("gbn_bias", C.c_void_p), ("gwh", C.c_void_p), ("gbh", C.c_void_p),
                ("p", HeadParams), ("B", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("dtype", C.c_int32),
                ("flags", C.c_int32)]


HEAD_BWD_ACCUM_GX, HEAD_LOGITS_F32 = 1, 2
HEAD_LAYOUT_NHWC = 4   # mask head level flag (forward and backward): x, gx are (B,H,W,C) -- torch's channels_last


class PmgCfg(C.Structure):                       # mgapmg_cfg_t
    _fields_ = [("tau", C.c_float), ("p_min", C.c_float), ("threshold", C.c_float), ("hard", C.c_int32)]


NORM_IN, NORM_BN = 0, 1


SPADE_LAYOUT_NHWC = 2  # MaskSPADE level flag (MGASPADE_LAYOUT_NHWC, forward and backward): x, y, gy, gx are (B,H,W,C); sizes are unchanged


class SpadeLevel(C.Structure):                   # mgaspade_level_t (include/mgaspade.h)
    _fields_ = ([(n, C.c_void_p) for n in ("x", "mask", "y", "gy", "gx", "gmask", "w0", "b0", "wg", "bg", "wb", "bb", "running_mean",
                                           "running_var", "num_batches_tracked", "gw0", "gb0", "gwg", "gbg", "gwb", "gbb")] +
                [("ctx", C.c_void_p), ("ctx_bytes", C.c_size_t), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)] +
                [(n, C.c_int32) for n in ("B", "C", "H", "W", "hidden", "dtype", "norm_type", "training", "use_sigmoid_mask", "save_gamma")] +
                [("eps", C.c_float), ("momentum", C.c_float), ("flags", C.c_int32)])


class ResampleLevel(C.Structure):                # mgaspade_resample_level_t (include/mgaresample.h)
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("B", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32),
                ("out_h", C.c_int32), ("out_w", C.c_int32)]


# ProbMaskGater on a pyramid with in-kernel noise (include/mgagate.h): mgagate_level_t.mode, by the module's mode name
GATE_DETERMINISTIC, GATE_GUMBEL, GATE_HARD_ST, GATE_BERNOULLI_DETACH = 0, 1, 2, 3
GATE_MODES = dict(deterministic=GATE_DETERMINISTIC, gumbel=GATE_GUMBEL, hard_st=GATE_HARD_ST, bernoulli_detach=GATE_BERNOULLI_DETACH)


class GateLevel(C.Structure):                    # mgagate_level_t (include/mgagate.h)
    _fields_ = [("p", C.c_void_p), ("out", C.c_void_p), ("msoft", C.c_void_p), ("gout", C.c_void_p), ("gp", C.c_void_p),
                ("n", C.c_uint32), ("mode", C.c_int32), ("stream_id", C.c_int32),
                ("tau", C.c_float), ("p_min", C.c_float), ("threshold", C.c_float)]


# the fused optimizer step over the plans' gradient bucket (include/mgaopt.h: a header of its own as well)
OPT_SGD, OPT_ADAMW = 0, 1
OPT_KINDS = dict(sgd=OPT_SGD, adamw=OPT_ADAMW)
OPT_GROUPS, OPT_MAX_SEGMENTS, OPT_CHUNK = 3, 4096, 1024


class OptSegment(C.Structure):                   # mgaopt_segment_t
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state0", C.c_void_p), ("state1", C.c_void_p), ("ema", C.c_void_p),
                ("n", C.c_int64), ("group", C.c_int32), ("reserved", C.c_int32)]


class OptCfg(C.Structure):                       # mgaopt_cfg_t
    _fields_ = [("kind", C.c_int32), ("check_finite", C.c_int32), ("zero_grad", C.c_int32), ("reserved", C.c_int32),
                ("beta2", C.c_double), ("eps", C.c_double), ("max_norm", C.c_double), ("ema_decay", C.c_double), ("ema_tau", C.c_double)]


class OptHyper(C.Structure):                     # mgaopt_hyper_t: device memory; the mirror gives optim.py the word offsets
    _fields_ = ([(n, C.c_float * OPT_GROUPS) for n in ("lr", "momentum", "one_minus_momentum", "ln_momentum", "weight_decay")] +
                [("inv_scale", C.c_float), ("ext_sumsq", C.c_float), ("ext_found_inf", C.c_int32), ("updates", C.c_int32),
                 ("t", C.c_int32 * 2), ("grad_norm", C.c_float), ("clip_coef", C.c_float), ("found_inf", C.c_int32),
                 ("reserved", C.c_int32 * 8)])


# the multi-scale segmentation targets from full-resolution masks (include/mgatargets.h: a header of its own as well)
TGT_AVGPOOL, TGT_MAXPOOL = 0, 1
TGT_METHODS = dict(avgpool=TGT_AVGPOOL, maxpool=TGT_MAXPOOL)
TGT_SRC_U8, TGT_SRC_F32 = 0, 1
TGT_CLOSE3 = 1
TGT_MAX_LEVELS = 4


class TargetsDesc(C.Structure):                  # mgatgt_desc_t
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p * TGT_MAX_LEVELS), ("stride", C.c_int32 * TGT_MAX_LEVELS),
                ("n_levels", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("src_dtype", C.c_int32), ("method", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


# the detection criterion -- TAL assignment, CIoU, DFL, BCE -- on the Detect maps (include/mgadet.h: a header of its own as well)
DET_MAX_LEVELS, DET_MAX_TOPK, DET_MAX_GT, DET_REG_MAX = 4, 16, 256, 16


class DetDesc(C.Structure):                      # mgadet_desc_t
    _fields_ = [("feats", C.c_void_p * DET_MAX_LEVELS), ("g_feats", C.c_void_p * DET_MAX_LEVELS),
                ("H", C.c_int32 * DET_MAX_LEVELS), ("W", C.c_int32 * DET_MAX_LEVELS), ("stride", C.c_int32 * DET_MAX_LEVELS),
                ("n_levels", C.c_int32), ("B", C.c_int32), ("nc", C.c_int32), ("reg_max", C.c_int32),
                ("dtype", C.c_int32), ("topk", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("gains", C.c_float * 3), ("reserved", C.c_int32),
                ("batch_idx", C.c_void_p), ("cls", C.c_void_p), ("bboxes", C.c_void_p), ("n", C.c_void_p),
                ("assign_gt", C.c_void_p), ("assign_score", C.c_void_p), ("out", C.c_void_p), ("items", C.c_void_p), ("status", C.c_void_p),
                ("upstream", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


# the detection post-process -- Detect decode, candidates, greedy NMS -- (include/mganms.h: a header of its own as well)
NMS_MAX_LEVELS, NMS_MULTI_LABEL, NMS_AGNOSTIC = 4, 1, 2


class NmsDesc(C.Structure):                      # mganms_desc_t
    _fields_ = [("feats", C.c_void_p * NMS_MAX_LEVELS), ("pred", C.c_void_p),
                ("H", C.c_int32 * NMS_MAX_LEVELS), ("W", C.c_int32 * NMS_MAX_LEVELS), ("stride", C.c_int32 * NMS_MAX_LEVELS),
                ("n_levels", C.c_int32), ("A", C.c_int32), ("B", C.c_int32), ("nc", C.c_int32),
                ("dtype", C.c_int32), ("max_det", C.c_int32), ("max_nms", C.c_int32), ("flags", C.c_int32),
                ("conf_thres", C.c_float), ("iou_thres", C.c_float), ("cand_cap", C.c_int32), ("reserved", C.c_int32),
                ("dets", C.c_void_p), ("count", C.c_void_p), ("keep", C.c_void_p), ("status", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


# detections matched to labels for the validation metrics (include/ext/mgamatch.h: a header in a directory of its own, EXT_HEADERS below)
MATCH_MAX_IOU, MATCH_SINGLE_CLS = 16, 1


class MatchDesc(C.Structure):                    # mgamatch_desc_t
    _fields_ = [("dets", C.c_void_p), ("count", C.c_void_p), ("batch_idx", C.c_void_p), ("cls", C.c_void_p), ("bboxes", C.c_void_p),
                ("n", C.c_void_p), ("B", C.c_int32), ("max_det", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("img_w", C.c_float), ("img_h", C.c_float), ("niou", C.c_int32), ("flags", C.c_int32), ("iouv", C.c_float * MATCH_MAX_IOU),
                ("rows_cap", C.c_int32), ("tgt_cap", C.c_int32),
                ("tp", C.c_void_p), ("best_iou", C.c_void_p), ("best_gt", C.c_void_p),
                ("rows_tp", C.c_void_p), ("rows_conf", C.c_void_p), ("rows_cls", C.c_void_p), ("rows_img", C.c_void_p),
                ("tgt_cls", C.c_void_p), ("tgt_img", C.c_void_p), ("state", C.c_void_p), ("status", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("reserved", C.c_int32)]


# the validator's confusion matrix (include/ext/mgaconfusion.h: the third stage behind the post-process and the matching, METRIC_HEADERS below)
CM_MAX_NC, CM_SINGLE_CLS = 119, 1


class ConfusionDesc(C.Structure):                # mgacm_desc_t
    _fields_ = [("dets", C.c_void_p), ("count", C.c_void_p), ("batch_idx", C.c_void_p), ("cls", C.c_void_p), ("bboxes", C.c_void_p),
                ("n", C.c_void_p), ("B", C.c_int32), ("max_det", C.c_int32), ("n_cap", C.c_int32), ("m_cap", C.c_int32),
                ("nc", C.c_int32), ("flags", C.c_int32),
                ("img_w", C.c_float), ("img_h", C.c_float), ("conf_thres", C.c_float), ("iou_thres", C.c_float),
                ("det_out", C.c_void_p), ("lab_out", C.c_void_p), ("cm", C.c_void_p), ("acc", C.c_void_p), ("status", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("reserved", C.c_int32)]


# average precision per class from the accumulated rows (include/ext/mgaap.h: the fourth stage, CURVE_HEADERS below)
AP_MAX_NC, AP_TILE, AP_POINTS, AP_CURVE_POINTS = 1024, 2048, 101, 1000


class ApDesc(C.Structure):                       # mgaap_desc_t
    _fields_ = [("rows_tp", C.c_void_p), ("rows_conf", C.c_void_p), ("rows_cls", C.c_void_p), ("rows_img", C.c_void_p),
                ("tgt_cls", C.c_void_p), ("tgt_img", C.c_void_p), ("state", C.c_void_p),
                ("rows_cap", C.c_int32), ("tgt_cap", C.c_int32), ("niou", C.c_int32), ("nc", C.c_int32),
                ("grid_ap", C.c_void_p), ("grid_curve", C.c_void_p), ("result", C.c_void_p), ("status", C.c_void_p),
                ("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("reserved", C.c_int32)]


def ap_result_layout(nc: int, niou: int) -> dict:
    """The result block of mgaap_run in bytes: name -> (offset, shape, numpy dtype string); "total": its size."""
    out, o = {}, 0
    for name, shape, dt in (("ap", (nc, niou), "f8"), ("p_curve", (nc, AP_CURVE_POINTS), "f8"), ("r_curve", (nc, AP_CURVE_POINTS), "f8"),
                            ("prec_values", (nc, AP_CURVE_POINTS), "f8"), ("nt", (nc,), "i4"), ("n_det", (nc,), "i4")):
        out[name] = (o, shape, dt)
        o += shape[0] * (shape[1] if len(shape) > 1 else 1) * int(dt[1])
    out["total"] = o
    return out


# a batch of uint8 images prepared in one launch (include/ext/mgaimage.h: /255, element type, layout, channel order, resize; IMAGE_HEADERS below)
IMG_SRC_NHWC, IMG_DST_NHWC, IMG_REVERSE_C = 1, 2, 4
IMG_MAX_C, IMG_TILE_PX, IMG_TILE_W, IMG_TILE_H = 4, 1024, 1024, 64


class ImageDesc(C.Structure):                    # mgaimg_desc_t
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p),
                ("B", C.c_int32), ("C", C.c_int32), ("in_h", C.c_int32), ("in_w", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("dtype", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class Header(NamedTuple):
    """What one file under include/ declares and this module mirrors (tests/test_abi_headers.py holds each record against its header)."""
    symbols: dict        # function -> (restype, argtypes)
    structs: dict        # C struct tag -> ctypes mirror
    constants: dict      # C #define / enumerator -> the Python value that mirrors it


_BWD_STAGE_NAMES = dict(reduce1="REDUCE1", convT="CONVT", reduce2="REDUCE2", wsa="WSA", params="PARAMGRAD", apply="APPLY")
_i = C.c_int
HEADERS = {
    "mgacbam.h": Header(
        symbols={
            "mgacbam_abi_version": (_i, []),
            "mgacbam_last_error": (C.c_char_p, []),
            "mgacbam_build_info": (C.c_char_p, []),
            "mgacbam_reload_env": (None, []),
            "mgacbam_ctx_bytes": (C.c_size_t, [_i] * 5),
            "mgacbam_bwd_scratch_bytes": (C.c_size_t, [_i] * 6),
            "mgacbam_ctx_layout": (_i, [_i] * 5 + [C.POINTER(CtxLayout)]),
            "mgacbam_fwd_ws_bytes": (C.c_size_t, [_i] * 6),
            "mgacbam_bwd_scratch_bytes_flags": (C.c_size_t, [_i] * 7),
            "mgacbam_forward": (_i, [C.POINTER(FwdLevel), _i, C.c_void_p]),
            "mgacbam_backward": (_i, [C.POINTER(BwdLevel), _i, C.c_void_p]),
            "mgacbam_forward_stages": (_i, [C.POINTER(FwdLevel), _i, _i, C.c_void_p]),
            "mgacbam_backward_stages": (_i, [C.POINTER(BwdLevel), _i, _i, C.c_void_p]),
            "mgacbam_resize_nearest": (_i, [C.c_void_p, C.c_void_p] + [_i] * 5 + [C.c_void_p]),
            "mgacbam_eca_ctx_bytes": (C.c_size_t, [_i] * 4),
            "mgacbam_eca_scratch_bytes": (C.c_size_t, [_i] * 4),
            "mgacbam_eca_ctx_bytes_flags": (C.c_size_t, [_i] * 5),
            "mgacbam_eca_scratch_bytes_flags": (C.c_size_t, [_i] * 5),
            "mgacbam_eca_forward": (_i, [C.POINTER(EcaFwdLevel), _i, C.c_void_p]),
            "mgacbam_eca_backward": (_i, [C.POINTER(EcaBwdLevel), _i, C.c_void_p]),
            "mgaseg_ws_bytes": (C.c_size_t, [C.POINTER(SegLevel), _i]),
            "mgaseg_forward": (_i, [C.POINTER(SegLevel), _i, C.POINTER(SegCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
            "mgaseg_backward": (_i, [C.POINTER(SegLevel), _i, C.POINTER(SegCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
            "mgahead_ctx_bytes": (C.c_size_t, [_i] * 5),
            "mgahead_bwd_scratch_bytes": (C.c_size_t, [_i] * 5),
            "mgahead_ctx_bytes_flags": (C.c_size_t, [_i] * 6),
            "mgahead_bwd_scratch_bytes_flags": (C.c_size_t, [_i] * 6),
            "mgahead_forward": (_i, [C.POINTER(HeadFwdLevel), _i, C.c_void_p]),
            "mgahead_backward": (_i, [C.POINTER(HeadBwdLevel), _i, C.c_void_p]),
            "mgakendall_forward": (_i, [C.c_void_p, _i, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
            "mgakendall_backward": (_i, [C.c_void_p, _i] + [C.c_void_p] * 7),
            "mgaseg_kendall_forward": (_i, [C.POINTER(SegLevel), _i, C.POINTER(SegCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, _i,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
            "mgaseg_kendall_backward": (_i, [C.POINTER(SegLevel), _i, C.POINTER(SegCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, _i] +
                                        [C.c_void_p] * 6),
            "mgapmg_forward": (_i, [C.c_void_p] * 5 + [C.c_size_t, C.POINTER(PmgCfg), C.c_void_p]),
            "mgapmg_backward": (_i, [C.c_void_p] * 4 + [C.c_size_t, C.POINTER(PmgCfg), C.c_void_p]),
        },
        structs=dict(mgacbam_params=Params, mgacbam_fwd_level=FwdLevel, mgacbam_bwd_level=BwdLevel, mgacbam_ctx_layout=CtxLayout,
                     mgacbam_eca_params=EcaParams, mgacbam_eca_fwd_level=EcaFwdLevel, mgacbam_eca_bwd_level=EcaBwdLevel,
                     mgaseg_level=SegLevel, mgaseg_cfg=SegCfg, mgahead_params=HeadParams, mgahead_fwd_level=HeadFwdLevel,
                     mgahead_bwd_level=HeadBwdLevel, mgapmg_cfg=PmgCfg),
        constants=dict(
            MGACBAM_ABI_VERSION=ABI_VERSION, MGACBAM_MAX_LEVELS=MAX_LEVELS, MGACBAM_F32=F32, MGACBAM_F16=F16, MGACBAM_BF16=BF16,
            MGACBAM_PROJ_MAX_HIDDEN=PROJ_MAX_HIDDEN, MGACBAM_FWD_SAVE_PROJ=FWD_SAVE_PROJ, MGACBAM_BWD_HAVE_PROJ=BWD_HAVE_PROJ,
            MGACBAM_LAYOUT_NHWC=LAYOUT_NHWC, MGACBAM_E_NULL=E_NULL, MGACBAM_E_SHAPE=E_SHAPE, MGACBAM_E_DTYPE=E_DTYPE, MGACBAM_E_ALIGN=E_ALIGN,
            MGACBAM_E_LEVELS=E_LEVELS, MGACBAM_E_SIZE=E_SIZE,
            **{"MGACBAM_FWD_" + k.upper(): v for k, v in FWD_STAGES.items()}, MGACBAM_FWD_ALL=FWD_ALL, MGACBAM_FWD_FUSE=FWD_FUSE,
            **{"MGACBAM_BWD_" + _BWD_STAGE_NAMES[k]: v for k, v in BWD_STAGES.items()}, MGACBAM_BWD_FUSE=BWD_FUSE,
            MGACBAM_BWD_PARAMS=BWD_PARAMS, MGACBAM_BWD_INPUTS=BWD_INPUTS, MGACBAM_BWD_ALL=BWD_ALL, MGACBAM_BWD_FOLD=BWD_FOLD,
            MGASEG_MAX_LEVELS=SEG_MAX_LEVELS, MGASEG_NEAREST=SEG_NEAREST, MGASEG_BILINEAR=SEG_BILINEAR,
            MGAHEAD_BWD_ACCUM_GX=HEAD_BWD_ACCUM_GX, MGAHEAD_LOGITS_F32=HEAD_LOGITS_F32, MGAHEAD_LAYOUT_NHWC=HEAD_LAYOUT_NHWC)),
    "mgaspade.h": Header(                            # brings mgaresample.h in; each declaration belongs to the file that spells it
        symbols={
            "mgaspade_ctx_bytes": (C.c_size_t, [_i] * 5),
            "mgaspade_scratch_bytes": (C.c_size_t, [_i] * 5),
            "mgaspade_forward": (_i, [C.POINTER(SpadeLevel), _i, C.c_void_p]),
            "mgaspade_backward": (_i, [C.POINTER(SpadeLevel), _i, C.c_void_p]),
        },
        structs=dict(mgaspade_level=SpadeLevel),
        constants=dict(MGASPADE_NORM_IN=NORM_IN, MGASPADE_NORM_BN=NORM_BN, MGASPADE_LAYOUT_NHWC=SPADE_LAYOUT_NHWC)),
    "mgaresample.h": Header(
        symbols={
            "mgaspade_resample_forward": (_i, [C.POINTER(ResampleLevel), _i, C.c_void_p]),
            "mgaspade_resample_backward": (_i, [C.POINTER(ResampleLevel), _i, C.c_void_p]),
        },
        structs=dict(mgaspade_resample_level=ResampleLevel),
        constants={}),
    "mgagate.h": Header(
        symbols={
            "mgagate_forward": (_i, [C.POINTER(GateLevel), _i, C.c_void_p, C.c_void_p]),
            "mgagate_backward": (_i, [C.POINTER(GateLevel), _i, C.c_void_p]),
            "mgagate_philox4x32": (None, [C.POINTER(C.c_uint32)] * 3),
            "mgagate_uniforms": (None, [C.c_int64, C.c_int64, C.c_int32, C.c_uint32, C.POINTER(C.c_float)]),
        },
        structs=dict(mgagate_level=GateLevel),
        constants={"MGAGATE_" + k.upper(): v for k, v in GATE_MODES.items()}),
    "mgaopt.h": Header(
        symbols={
            "mgaopt_ws_bytes": (C.c_size_t, [C.POINTER(OptSegment), _i]),
            "mgaopt_ws_init": (_i, [C.POINTER(OptSegment), _i, C.c_void_p, C.c_size_t]),
            "mgaopt_accumulate": (_i, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
            "mgaopt_step": (_i, [C.POINTER(OptSegment), _i, C.POINTER(OptCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
        },
        structs=dict(mgaopt_segment=OptSegment, mgaopt_cfg=OptCfg, mgaopt_hyper=OptHyper),
        constants=dict({"MGAOPT_" + k.upper(): v for k, v in OPT_KINDS.items()},
                       MGAOPT_GROUPS=OPT_GROUPS, MGAOPT_MAX_SEGMENTS=OPT_MAX_SEGMENTS, MGAOPT_CHUNK=OPT_CHUNK)),
    "mgatargets.h": Header(
        symbols={
            "mgatgt_scratch_bytes": (C.c_size_t, [C.POINTER(TargetsDesc)]),
            "mgatgt_forward": (_i, [C.POINTER(TargetsDesc), C.c_void_p]),
        },
        structs=dict(mgatgt_desc=TargetsDesc),
        constants=dict({"MGATGT_" + k.upper(): v for k, v in TGT_METHODS.items()}, MGACBAM_E_ARG=E_ARG, MGATGT_SRC_U8=TGT_SRC_U8,
                       MGATGT_SRC_F32=TGT_SRC_F32, MGATGT_CLOSE3=TGT_CLOSE3, MGATGT_MAX_LEVELS=TGT_MAX_LEVELS)),
    "mgadet.h": Header(
        symbols={
            "mgadet_ws_bytes": (C.c_size_t, [C.POINTER(DetDesc)]),
            "mgadet_forward": (_i, [C.POINTER(DetDesc), C.c_void_p]),
            "mgadet_backward": (_i, [C.POINTER(DetDesc), C.c_void_p]),
        },
        structs=dict(mgadet_desc=DetDesc),
        constants=dict(MGADET_MAX_LEVELS=DET_MAX_LEVELS, MGADET_MAX_TOPK=DET_MAX_TOPK, MGADET_MAX_GT=DET_MAX_GT)),
    "mganms.h": Header(
        symbols={
            "mganms_ws_bytes": (C.c_size_t, [C.POINTER(NmsDesc)]),
            "mganms_run": (_i, [C.POINTER(NmsDesc), C.c_void_p]),
        },
        structs=dict(mganms_desc=NmsDesc),
        constants=dict(MGANMS_MAX_LEVELS=NMS_MAX_LEVELS, MGANMS_MULTI_LABEL=NMS_MULTI_LABEL, MGANMS_AGNOSTIC=NMS_AGNOSTIC)),
}
# the headers in directories below include/, keyed by their path from it: bound exactly as HEADERS, held to their files by their own tests
# (tests/test_abi_match.py)
EXT_HEADERS = {
    "ext/mgamatch.h": Header(
        symbols={
            "mgamatch_ws_bytes": (C.c_size_t, [C.POINTER(MatchDesc)]),
            "mgamatch_run": (_i, [C.POINTER(MatchDesc), C.c_void_p]),
        },
        structs=dict(mgamatch_desc=MatchDesc),
        constants=dict(MGAMATCH_MAX_IOU=MATCH_MAX_IOU, MGAMATCH_SINGLE_CLS=MATCH_SINGLE_CLS)),
}
# the headers of the validation metrics behind the matching, keyed and bound the same way (tests/test_abi_confusion.py)
METRIC_HEADERS = {
    "ext/mgaconfusion.h": Header(
        symbols={
            "mgacm_ws_bytes": (C.c_size_t, [C.POINTER(ConfusionDesc)]),
            "mgacm_run": (_i, [C.POINTER(ConfusionDesc), C.c_void_p]),
        },
        structs=dict(mgacm_desc=ConfusionDesc),
        constants=dict(MGACM_MAX_NC=CM_MAX_NC, MGACM_SINGLE_CLS=CM_SINGLE_CLS)),
}
# the Detect maps in either memory layout (include/ext/mgamaps.h: the descriptors of mgadet.h and mganms.h with a flags argument; a table of
# its own, bound by load() as the others; tests/test_abi_maps.py)
MAPS_LAYOUT_NHWC = 1
LAYOUT_HEADERS = {
    "ext/mgamaps.h": Header(
        symbols={
            "mgamaps_det_forward": (_i, [C.POINTER(DetDesc), C.c_int32, C.c_void_p]),
            "mgamaps_det_backward": (_i, [C.POINTER(DetDesc), C.c_int32, C.c_void_p]),
            "mgamaps_nms_run": (_i, [C.POINTER(NmsDesc), C.c_int32, C.c_void_p]),
        },
        structs={},
        constants=dict(MGAMAPS_LAYOUT_NHWC=MAPS_LAYOUT_NHWC)),
}
# average precision per class behind the matching's accumulation (include/ext/mgaap.h; a table of its own as well; tests/test_abi_ap.py)
CURVE_HEADERS = {
    "ext/mgaap.h": Header(
        symbols={
            "mgaap_ws_bytes": (C.c_size_t, [C.POINTER(ApDesc)]),
            "mgaap_run": (_i, [C.POINTER(ApDesc), C.c_void_p]),
        },
        structs=dict(mgaap_desc=ApDesc),
        constants=dict(MGAAP_MAX_NC=AP_MAX_NC, MGAAP_TILE=AP_TILE, MGAAP_AP_POINTS=AP_POINTS, MGAAP_CURVE_POINTS=AP_CURVE_POINTS)),
}
# the image batch in front of the network (include/ext/mgaimage.h; a table of its own as well; tests/test_abi_image.py)
IMAGE_HEADERS = {
    "ext/mgaimage.h": Header(
        symbols={"mgaimg_run": (_i, [C.POINTER(ImageDesc), C.c_void_p])},
        structs=dict(mgaimg_desc=ImageDesc),
        constants=dict(MGAIMG_SRC_NHWC=IMG_SRC_NHWC, MGAIMG_DST_NHWC=IMG_DST_NHWC, MGAIMG_REVERSE_C=IMG_REVERSE_C, MGAIMG_MAX_C=IMG_MAX_C,
                       MGAIMG_TILE_PX=IMG_TILE_PX, MGAIMG_TILE_W=IMG_TILE_W, MGAIMG_TILE_H=IMG_TILE_H)),
}
_TABLES = dict(HEADERS=HEADERS, EXT_HEADERS=EXT_HEADERS, METRIC_HEADERS=METRIC_HEADERS, LAYOUT_HEADERS=LAYOUT_HEADERS,
               CURVE_HEADERS=CURVE_HEADERS, IMAGE_HEADERS=IMAGE_HEADERS)
ALL_HEADERS = {**HEADERS, **EXT_HEADERS, **METRIC_HEADERS}       # the three tables of the descriptors' headers
_EVERY_HEADER = {**ALL_HEADERS, **LAYOUT_HEADERS, **CURVE_HEADERS, **IMAGE_HEADERS}
_bound = [name for h in _EVERY_HEADER.values() for name in h.symbols]
if len(_EVERY_HEADER) != sum(len(t) for t in _TABLES.values()):
    _keys = [k for t in _TABLES.values() for k in t]
    raise ImportError(f"_lib.{', _lib.'.join(_TABLES)}: two tables hold a record for {sorted(k for k in set(_keys) if _keys.count(k) > 1)}")
if len(_bound) != len(set(_bound)):
    raise ImportError(f"_lib.{', _lib.'.join(_TABLES)} bind a symbol in two records: {sorted(n for n in set(_bound) if _bound.count(n) > 1)}")

_lib = None
_lock = threading.Lock()


class LibraryMissing(RuntimeError):
    pass


def load():
    """dlopen libmgacbam.so (once).  Raises LibraryMissing with the build command if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise LibraryMissing(
                f"{LIB_PATH} not found: the HIP library is required (there is no fallback path). "
                "Build it with `python -m mga_yolo_amd.build` or `python -c 'import __graft_entry__ as g; g.build()'`.")
        import torch  # noqa: F401  -- loads torch's libamdhip64.so.7 first so the library binds to the same HIP runtime
        lib = C.CDLL(LIB_PATH)
        for h in _EVERY_HEADER.values():
            for name, (res, args) in h.symbols.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError as e:
                    raise LibraryMissing(f"{LIB_PATH} does not export {name}; rebuild it") from e
                fn.restype, fn.argtypes = res, args
        v = lib.mgacbam_abi_version()
        if v != ABI_VERSION:
            raise LibraryMissing(f"{LIB_PATH} has ABI version {v}, expected {ABI_VERSION}; rebuild it")
        _lib = lib
        return lib


ENV_EPOCH = 0      # bumped by reload_env(): launch geometry may have changed, so pooled hand-off state of older epochs is not reused


def reload_env():
    """Make the library re-read its MGACBAM_* knobs (they are read once; tests and tuning sweeps change them in-process)."""
    global ENV_EPOCH
    load().mgacbam_reload_env()
    ENV_EPOCH += 1
    _size_cache.clear()          # scratch sizes depend on the launch geometry (tile counts), which the knobs can change


def available() -> bool:
    return os.path.exists(LIB_PATH)


def check(rc: int, what: str):
    if rc != 0:
        msg = load().mgacbam_last_error().decode(errors="replace")
        kind = "argument error" if rc < 0 else "HIP error"
        if rc == E_SIZE:
            kind = "work buffer too small (MGACBAM_E_SIZE)"
        raise RuntimeError(f"{what}: {kind} {rc}: {msg}")


_size_cache = {}     # (symbol, ints...) -> bytes: the eager path asks on every call; the answer only depends on the shape and the knobs


def size(symbol: str, *ints) -> int:
    """The one size query: `symbol`(*ints) in bytes, cached until reload_env(); 0 is the library's refusal and raises as E_SHAPE."""
    key = (symbol, *ints)
    n = _size_cache.get(key)
    if n is None:
        n = getattr(load(), symbol)(*ints)
        if n == 0:
            check(E_SHAPE, symbol)
        _size_cache[key] = n
    return n


# The plain and the _flags form of a query agree at flags = 0 (tests/test_abi.py pins every pair), so each block asks the _flags form only.
def ctx_bytes(B, Cc, H, W, hidden) -> int:
    return size("mgacbam_ctx_bytes", B, Cc, H, W, hidden)


def scratch_bytes(B, Cc, H, W, hidden, k, flags: int = 0) -> int:
    return size("mgacbam_bwd_scratch_bytes_flags", B, Cc, H, W, hidden, k, flags & LAYOUT_NHWC)


def fwd_ws_bytes(B, Cc, H, W, hidden, flags: int) -> int:
    """Forward workspace of a level: 0 for NCHW levels, the per-chunk pooling partials for LAYOUT_NHWC levels."""
    return size("mgacbam_fwd_ws_bytes", B, Cc, H, W, hidden, LAYOUT_NHWC) if flags & LAYOUT_NHWC else 0


def eca_ctx_bytes(B, Cc, H, W, flags: int = 0) -> int:
    """ctx of a MaskECA level: the saved statistics, plus the per-chunk pooling partials for LAYOUT_NHWC levels."""
    return size("mgacbam_eca_ctx_bytes_flags", B, Cc, H, W, flags & LAYOUT_NHWC)


def eca_scratch_bytes(B, Cc, H, W, flags: int = 0) -> int:
    """Backward scratch of a MaskECA level: gg, plus its per-chunk partials for LAYOUT_NHWC levels."""
    return size("mgacbam_eca_scratch_bytes_flags", B, Cc, H, W, flags & LAYOUT_NHWC)


def head_ctx_bytes(B, Cc, H, W, hidden, flags: int = 0) -> int:
    """ctx of a mask-head level; only HEAD_LAYOUT_NHWC changes the size (the other level flags do not)."""
    return size("mgahead_ctx_bytes_flags", B, Cc, H, W, hidden, flags & HEAD_LAYOUT_NHWC)


def head_scratch_bytes(B, Cc, H, W, hidden, flags: int = 0) -> int:
    """Backward scratch of a mask-head level; only HEAD_LAYOUT_NHWC changes the size."""
    return size("mgahead_bwd_scratch_bytes_flags", B, Cc, H, W, hidden, flags & HEAD_LAYOUT_NHWC)


def spade_ctx_bytes(B, Cc, H, W, hidden) -> int:
    """ctx of a MaskSPADE level: statistics, the packed conv weights and the saved gamma (sized for fp32 features)."""
    return size("mgaspade_ctx_bytes", B, Cc, H, W, hidden)


def spade_scratch_bytes(B, Cc, H, W, hidden) -> int:
    """Backward scratch of a MaskSPADE level: plane sums, the split-K partials of dW, the tap planes of ds, the dW0 partials."""
    return size("mgaspade_scratch_bytes", B, Cc, H, W, hidden)


def _table_size(symbol: str, refusal: int, *args, zero_is_an_answer: bool = False) -> int:
    """A size query that reads a whole level table or descriptor, so it is asked every time: 0 is the library's refusal and raises as
    `refusal` with its message -- unless 0 can be the answer, which a refusal is told apart from by its message."""
    lib = load()
    nbytes = getattr(lib, symbol)(*args)
    if nbytes == 0 and (not zero_is_an_answer or lib.mgacbam_last_error()):
        check(refusal, symbol)
    return nbytes


def seg_ws_bytes(levels, n: int) -> int:
    """Workspace of a segmentation-loss call."""
    return _table_size("mgaseg_ws_bytes", E_SHAPE, levels, n)


def targets_scratch_bytes(desc) -> int:
    """Scratch of a target-pyramid call: 0 without TGT_CLOSE3."""
    return _table_size("mgatgt_scratch_bytes", E_ARG, C.byref(desc), zero_is_an_answer=True)


def det_ws_bytes(desc) -> int:
    """Workspace of a detection-criterion call."""
    return _table_size("mgadet_ws_bytes", E_ARG, C.byref(desc))


def nms_ws_bytes(desc) -> int:
    """Workspace of a detection post-process call."""
    return _table_size("mganms_ws_bytes", E_ARG, C.byref(desc))


def match_ws_bytes(desc) -> int:
    """Workspace of a detection-matching call."""
    return _table_size("mgamatch_ws_bytes", E_ARG, C.byref(desc))


def confusion_ws_bytes(desc) -> int:
    """Workspace of a confusion-matrix call."""
    return _table_size("mgacm_ws_bytes", E_ARG, C.byref(desc))


def ap_ws_bytes(desc) -> int:
    """Workspace of an average-precision call."""
    return _table_size("mgaap_ws_bytes", E_ARG, C.byref(desc))


ARRIVE_STRIDE = 64     # int32 words between the arrival words of two samples (csrc/args.cuh: kArriveStride)


def sync_regions(B, Cc, H, W) -> dict:
    """The hand-off state at ctx_layout()["sync"], in int32 words from its start: name -> (offset, length).  Every word is a generation
    counter the caller zero-fills once.  This is the one Python copy of csrc/host.cuh's sync_layout (tests/test_abi.py pins the two
    against each other): gate = (B, nflag) k_gate tile flags, status = [time-out, 3 spare], ca = (B) per-sample flags, tiles / conv_tiles =
    (B, nflag) flags of the folded backward launch, merged_* / wsa_tiles = the same and the dWsa-tile flags of the merged launch
    (k_bwd_r12), sweeps = its (B, C) per-channel flags, arrive = (B, ARRIVE_STRIDE), column 0 = the arrival word of
    k_pool's workgroups of a sample at the levels where its last arriver forms ca (the one region that does not count calls: every launch
    leaves it at 0)."""
    nf = B * ((H * W + 15) // 16 + 1)              # nflag per sample: one per 16 pixels (kSyncPx) + 1
    out, o = {}, 0
    for name, n in (("gate", nf), ("status", 4), ("ca", B), ("tiles", nf), ("conv_tiles", nf), ("merged_tiles", nf),
                    ("merged_conv_tiles", nf), ("wsa_tiles", nf), ("sweeps", B * Cc), ("arrive", B * ARRIVE_STRIDE)):
        out[name] = (o, n)
        o += n
    return out


def sync_len(B, Cc, H, W) -> int:
    o, n = sync_regions(B, Cc, H, W)["arrive"]
    return o + n


def sync_slices(B, Cc, H, W) -> dict:
    """sync_regions as slice objects: ctx_views(...)["sync"][sync_slices(...)["status"]]"""
    return {name: slice(o, o + n) for name, (o, n) in sync_regions(B, Cc, H, W).items()}


def ctx_layout(B, Cc, H, W, hidden) -> dict:
    key = ("layout", B, Cc, H, W, hidden)
    lay = _size_cache.get(key)
    if lay is None:
        L = CtxLayout()
        check(load().mgacbam_ctx_layout(B, Cc, H, W, hidden, C.byref(L)), "mgacbam_ctx_layout")
        lay = _size_cache[key] = {n: getattr(L, n) for n in CTX_FIELDS}
    return dict(lay)
