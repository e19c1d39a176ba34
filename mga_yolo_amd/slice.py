"""Static executor of the LAYER-LOOP SLICE of one training step around the hot path (SURVEY 8d images/s definition (2), 8f-1):

    feature_l --MGAMaskHead_l--> logits_l --[feature_l, logits_l]--> MaskCBAM_l --> refined_l (-> Detect)        model/model.py:57-74
    seg_total = SegmentationLoss({p3,p4,p5: logits}, masks_multi)                                                  model/model.py:196-202
    total     = e^{-s_det} det_loss + s_det + e^{-s_seg} seg_total + s_seg                                         model/model.py:204-206
    backward of all of it; the gradient of feature_l = what MaskCBAM sends back + what its mask head sends back (the feature
    feeds both), accumulated in the head's GEMM epilogue instead of a feature-sized add.

Everything between the neck's P3/P4/P5 features and the Detect head's inputs -- i.e. every MGA-specific layer of the reference model
plus its loss terms -- runs as C-ABI calls on pre-allocated buffers: 3 + 2 + 2 launches forward, 1 + 2 + 5 backward for
all three levels together, recorded into one hipGraph.  The backbone / neck / Detect / detection loss are out of scope:
their contribution enters as given tensors -- `gy_l` (dL/d refined_l, what Detect's backward would deliver) and `det_loss`
(the criterion's 3-vector).

Buffers (per level l): x (feature), logits (= MaskCBAM's mask input, fp32), y, gy, gx, targets; one flat fp32 gradient bucket for
every parameter of the slice (three MaskCBAM blocks, three mask heads, the two Kendall log-variances): what DDP all-reduces.

With ``gate=`` the slice is the one an MGA_PROB_MODE run trains (the default of every shipped hyper-parameter file): logits_l go through
ProbMaskGater before MaskCBAM_l (masked_cbam.py:163-164) while the loss keeps reading the logits -- one launch more each way for all
levels, the noise drawn in the kernel (include/mgagate.h).

``SlicePlan.create(..., block="cbam" | "eca" | "spade", channels_last=, target_resize=, block_running=)`` builds the same slice around MaskECA or
MaskSPADE (configs/models/yolov8_eca.yaml, yolov8_spade.yaml share the layer loop) and in either feature layout; the constructor builds the
MaskCBAM / NCHW slice.  The block is one of plan.py's pyramid plans (``plan.block``), whose buffers the heads and the loss are wired to; the
slice issues and captures its library calls the way they do (``plan._Executor``).

``SlicePlan.create(..., target_source=(Hm, Wm), target_method=, target_bridge=)`` makes the targets part of the step: the plan owns
``mask_full`` (B,Hm,Wm) uint8 -- the batch's masks at image resolution, what the caller fills instead of ``targets`` -- and ``forward`` starts
with the pyramid launch that writes ``targets`` from it (include/mgatargets.h; mga_yolo/data/dataset.py:94-103 on the device)."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._binding import HEAD, fill_seg
from .functional import BlockConfig, GateConfig, TargetPyramidCall, target_pyramid_check, target_pyramid_shapes
from .plan import EcaPyramidPlan, PyramidPlan, SpadePyramidPlan, _carve, _Executor

BLOCKS = ("cbam", "eca", "spade")
TARGET_RESIZE = {"nearest": _lib.SEG_NEAREST, "bilinear": _lib.SEG_BILINEAR}
HEAD_PARAM_NAMES = HEAD.param_names


def target_strides(shapes, target_source) -> Tuple[int, ...]:
    """Per level the stride that takes a (Hm, Wm) mask to the level's (H, W): the smallest power of two s in 2..64 with ceil(Hm / s) == H and
    ceil(Wm / s) == W (Hm / H itself where the sizes divide).  ValueError where none does, or the strides do not ascend."""
    Hm, Wm = (int(v) for v in target_source)
    if Hm < 1 or Wm < 1:
        raise ValueError(f"SlicePlan: target_source {target_source}")
    out = []
    for (_, _, H, W) in shapes:
        fit_h = [s for s in (2, 4, 8, 16, 32, 64) if -(-Hm // s) == H]
        fit_w = [s for s in (2, 4, 8, 16, 32, 64) if -(-Wm // s) == W]
        fit = [s for s in fit_h if s in fit_w]
        if not fit:
            why = "H and W ask for different strides" if fit_h and fit_w else "no power-of-two stride in 2..64 gives that size"
            raise ValueError(f"SlicePlan: a {Hm}x{Wm} mask and a {H}x{W} level: {why}")
        out.append(fit[0])
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"SlicePlan: the levels' strides {out} do not ascend")
    return tuple(out)


class SlicePlan(_Executor):
    def __init__(self, shapes: Sequence[Tuple[int, int, int, int]], hidden: Sequence[int], cbam_params, cbam_cfgs: Sequence[BlockConfig],
                 head_states: Sequence[dict], target_hw: Sequence[Tuple[int, int]] = None, scale_weights=(1.0, 1.0, 1.0),
                 bn_eps: float = 1e-3, bn_momentum: float = 0.03, device="cuda", training: bool = True, dtype: torch.dtype = torch.float32,
                 gate: Optional[Sequence[GateConfig]] = None, seed: int = 0):
        """shapes: (B,C,H,W) of the P3/P4/P5 features; hidden: mask-head widths; cbam_params: per level (w1,b1,w2,b2,wsa,beta);
        head_states: per level a MGAMaskHead state_dict; target_hw: resolution of the segmentation targets (default: feature size);
        bn_eps / bn_momentum: what Ultralytics' initialize_weights gives every BatchNorm2d (U/utils/torch_utils.py:570-572);
        dtype: element type of the FEATURES and their gradients (x, y, gy, gx: fp32 | fp16 | bf16).  The mask logits, the targets, every
        statistic and every parameter gradient stay fp32: the heads emit fp32 logits directly (MGAHEAD_LOGITS_F32), which is what
        MaskCBAM's mask input and the loss take -- no conversion pass anywhere in the slice.
        gate / seed: one GateConfig per level puts the reference's ProbMaskGater between each head and its MaskCBAM (masked_cbam.py:67-78,
        163-164: what MGA_PROB_MODE, set in every shipped hyper-parameter file, builds).  The heads then write `logits`, which the loss reads
        as before; the gate (plan.PyramidPlan, one launch each way) fills MaskCBAM's mask from them and turns its dL/dmask into the second
        dL/dlogits of the head's backward.  Its noise is the in-kernel Philox stream of include/mgagate.h, seeded with `seed`."""
        self._setup(shapes, hidden, cbam_params, cbam_cfgs, head_states, target_hw, scale_weights, bn_eps, bn_momentum, device, training, dtype,
                    gate, seed, "cbam", False, "nearest", None)

    @classmethod
    def create(cls, shapes, hidden, block_params, block_cfgs, head_states, *, block: str = "cbam", channels_last: bool = False,
               target_resize: str = "nearest", block_running=None, **kw) -> "SlicePlan":
        """The constructor for every model file of the reference (yolov8_cbam / _eca / _spade.yaml share this slice) and both feature layouts
        (why there are two: plan._BlockPlan).
        block: "cbam" | "eca" | "spade" -- block_params / block_cfgs are then per level (w1,b1,w2,b2,wsa,beta) with BlockConfig,
        (conv1d.weight, beta) with EcaConfig, or the six MaskSPADE tensors with SpadeConfig; block_running: per level MaskSPADE's batch-norm
        buffers (running_mean, running_var, num_batches_tracked) or None.  The matching pyramid plan is ``plan.block`` (``plan.cbam`` as well
        for "cbam"); the bucket is [block grads of all levels][head grads of all levels][log_vars].
        channels_last: x / y / gy / gx in torch.channels_last, the block's and the heads' channels-last kernels (what tools/harness.py trains in).
        target_resize: "nearest" | "bilinear" -- how targets at another size are read (losses/segmentation.py:103-110: bilinear is what an
        MGA_PROB_MODE run does).  gate: MaskCBAM only (the reference builds a ProbMaskGater nowhere else): ValueError otherwise.
        target_source=, target_method=, target_bridge= (keywords taken out of **kw: the named arguments are the ones callers bind by position or
        inspect).  target_source: (Hm, Wm) of the batch's full-resolution masks.  The plan then owns ``mask_full`` (B,Hm,Wm) uint8 (foreground: > 0), which
        the caller fills instead of ``targets``; forward() first builds ``targets`` from it -- one launch more, two with target_bridge -- with
        target_method "avgpool" (MGA_PROB_MODE's block-mean targets) or "maxpool", target_bridge: the 3x3 closing of the binary levels.  Level
        l's stride is the power of two s in 2..64 with ceil(Hm / s) == H_l and ceil(Wm / s) == W_l (the smallest, should several fit), its
        target is that size; ValueError if there is none -- the ratio is no such integer, or H and W disagree -- or the strides do not ascend,
        and if target_hw is passed as well.
        **kw: those three and the constructor's keyword arguments (target_hw, scale_weights, bn_eps, bn_momentum, device, training, dtype, gate,
        seed)."""
        self = cls.__new__(cls)
        target_source, target_method = kw.pop("target_source", None), kw.pop("target_method", "avgpool")
        target_bridge = kw.pop("target_bridge", False)
        args = dict(target_hw=None, scale_weights=(1.0, 1.0, 1.0), bn_eps=1e-3, bn_momentum=0.03, device="cuda", training=True,
                    dtype=torch.float32, gate=None, seed=0)
        unknown = set(kw) - set(args)
        if unknown:
            raise TypeError(f"SlicePlan.create: unexpected arguments {sorted(unknown)}")
        args.update(kw)
        strides = None
        if target_source is not None:                                  # checked on the shapes alone, before anything touches the device
            if args["target_hw"] is not None:
                raise ValueError("SlicePlan.create: target_hw is derived from target_source; pass one of the two")
            strides = target_strides(shapes, target_source)
            target_pyramid_check(strides, target_method, target_bridge)
            args["target_hw"] = [shp[2:] for shp in target_pyramid_shapes(1, *target_source, strides)]
        elif target_bridge or target_method != "avgpool":
            raise ValueError("SlicePlan.create: target_method / target_bridge without target_source")
        self._setup(shapes, hidden, block_params, block_cfgs, head_states, block=block, channels_last=channels_last,
                    target_resize=target_resize, block_running=block_running, **args)
        if strides is not None:
            B = shapes[0][0]
            self.target_strides, self.target_method, self.target_bridge = strides, target_method, bool(target_bridge)
            self.mask_full = torch.zeros(B, *target_source, dtype=torch.uint8, device=self.device)
            self._tgt = TargetPyramidCall(self.mask_full, self.targets, strides, target_method, target_bridge)
        return self

    def _setup(self, shapes, hidden, block_params, block_cfgs, head_states, target_hw, scale_weights, bn_eps, bn_momentum, device, training,
               dtype, gate, seed, block, channels_last, target_resize, block_running) -> None:
        if block not in BLOCKS:
            raise ValueError(f"SlicePlan: block {block!r} is none of {BLOCKS}")
        if target_resize not in TARGET_RESIZE:
            raise ValueError(f"SlicePlan: target_resize {target_resize!r} is none of {sorted(TARGET_RESIZE)}")
        if gate is not None and block != "cbam":
            raise ValueError(f"SlicePlan: gate= with block={block!r} (the reference builds a ProbMaskGater inside MaskCBAM only)")
        self.lib = _lib.load()
        self.device = torch.device(device)
        dev = self.device
        self.n = len(shapes)
        self._tgt = None                                               # create(target_source=...): the pyramid call that fills self.targets
        self.shapes, self.hidden = list(shapes), list(hidden)
        self.block_name, self.channels_last, self.target_resize = block, bool(channels_last), target_resize
        f32 = torch.float32
        # ---- one flat gradient bucket: [block grads of all levels][head grads of all levels][log_vars] --------------------------------
        n_block = sum(p.numel() for ps in block_params for p in ps)
        self.head_params: List[List[torch.Tensor]] = []
        self.head_buffers: List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = []
        for sd in head_states:
            self.head_params.append([sd[k].detach().to(dev, f32).contiguous().clone() for k in HEAD_PARAM_NAMES])
            self.head_buffers.append((sd["proj.1.running_mean"].detach().to(dev, f32).clone(), sd["proj.1.running_var"].detach().to(dev, f32).clone(),
                                      sd["proj.1.num_batches_tracked"].detach().to(dev).clone()))
        n_head = sum(p.numel() for ps in self.head_params for p in ps)
        self.grad_bucket = torch.zeros(n_block + n_head + 2, dtype=f32, device=dev)
        self.dtype = dtype
        common = dict(dtype=dtype, device=dev, with_mask=True, want_gmask=True, channels_last=channels_last, grad_bucket=self.grad_bucket[:n_block])
        if block == "cbam":
            self.block = self.cbam = PyramidPlan.create(shapes, block_params, block_cfgs, gate=gate, seed=seed, **common)
        elif block == "eca":
            self.block = EcaPyramidPlan.create(shapes, block_params, block_cfgs, **common)
        else:
            self.block = SpadePyramidPlan(shapes, block_params, block_cfgs, running=block_running, **common)
        blk = self.block
        self.gated = gate is not None
        # without a gate the heads write straight into the block's mask input; with one, into the gate's input
        self.x, self.logits, self.y, self.gy, self.gx = blk.x, (blk.logits if self.gated else blk.mask), blk.y, blk.gy, blk.gx
        g_logits2 = blk.glogits if self.gated else blk.gmask
        self.head_grads, off = _carve(self.grad_bucket, self.head_params, n_block)       # behind the block's views
        self.g_log_vars = self.grad_bucket[off:off + 2]
        # ---- loss side --------------------------------------------------------------------------------------------------------------
        self.log_vars = torch.zeros(2, dtype=f32, device=dev)          # mtl_log_vars (model.py:119-121)
        self.det_loss = torch.zeros(3, dtype=f32, device=dev)          # the detection criterion's (box, cls, dfl) vector: given
        self.total = torch.zeros(3, dtype=f32, device=dev)
        self.g_total = torch.ones(3, dtype=f32, device=dev)            # trainer: loss.sum().backward()
        self.g_det = torch.zeros(3, dtype=f32, device=dev)
        self.g_seg = torch.zeros((), dtype=f32, device=dev)
        target_hw = list(target_hw) if target_hw is not None else [(H, W) for _, _, H, W in shapes]
        self.targets = [torch.zeros(B, 1, th, tw, dtype=f32, device=dev) for (B, _, _, _), (th, tw) in zip(shapes, target_hw)]
        self.seg_glogits = [torch.zeros(B, 1, H, W, dtype=f32, device=dev) for B, _, H, W in shapes]
        self.seg_out = torch.zeros(1 + 3 * self.n, dtype=f32, device=dev)
        self._seg = (_lib.SegLevel * self.n)()
        for l in range(self.n):
            fill_seg(self._seg[l], self.logits[l], self.targets[l], self.seg_glogits[l], float(scale_weights[l]), TARGET_RESIZE[target_resize])
        self._seg_cfg = _lib.SegCfg(1.0, 1.0, 1.0, 1.0, 0, 0.5, 0.6, 0.5)      # SegLossConfig defaults (losses/segmentation.py:9-21)
        self.seg_ws = torch.zeros(_lib.seg_ws_bytes(self._seg, self.n), dtype=torch.uint8, device=dev)
        # ---- mask heads -------------------------------------------------------------------------------------------------------------
        self._hf, self._hb = (HEAD.fwd_level * self.n)(), (HEAD.bwd_level * self.n)()
        self.head_ctx, self.head_scratch = [], []
        hfl = HEAD.layout_nhwc if self.channels_last else 0             # x, gx channels_last: the NHWC forms of the heads' GEMM kernels
        for l, shp in enumerate(shapes):
            bn = (self.hidden[l], bn_eps, bn_momentum, training)
            self.head_ctx.append(torch.zeros(HEAD.ctx_bytes(shp, bn, hfl), dtype=torch.uint8, device=dev))
            self.head_scratch.append(torch.zeros(HEAD.scratch_bytes(shp, bn, hfl), dtype=torch.uint8, device=dev))
            # dL/dlogits = the loss's part (seg_glogits) + the block's dL/dmask, through the gate's backward when there is one (g_logits2):
            # summed while the head's backward loads them
            b = dict(x=self.x[l], y=self.logits[l], gy=self.seg_glogits[l], gy2=g_logits2[l], gx=self.gx[l], ctx=self.head_ctx[l],
                     scratch=self.head_scratch[l], params=self.head_params[l], grads=self.head_grads[l], running=self.head_buffers[l])
            HEAD.fill_fwd(self._hf[l], bn, hfl | _lib.HEAD_LOGITS_F32, **b)
            HEAD.fill_bwd(self._hb[l], bn, hfl | _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32, **b)

    # ------------------------------------------------------------------------------------------------------------------------------
    def forward(self):
        if self._tgt is not None:
            self._tgt.run()                                                                            # mask_full -> targets
        self._call(HEAD.fwd_entry, self._hf, self.n)                                                # features -> mask logits
        self.block.forward()                                                                           # [feature, logits] -> refined (a gate first: logits -> mask)
        # logits, targets -> seg_total (+ log entries) -> Kendall total, the combine riding in the loss's last launch
        self._call("mgaseg_kendall_forward", self._seg, self.n, C.byref(self._seg_cfg), self.seg_ws.data_ptr(), self.seg_ws.numel(), self.seg_out.data_ptr(),
                   self.det_loss.data_ptr(), 3, self.log_vars.data_ptr(), self.total.data_ptr())

    def backward(self):
        self._call("mgaseg_kendall_backward", self._seg, self.n, C.byref(self._seg_cfg), self.seg_ws.data_ptr(), self.seg_ws.numel(), self.seg_out.data_ptr(),
                   self.det_loss.data_ptr(), 3, self.log_vars.data_ptr(), self.g_total.data_ptr(),
                   self.g_det.data_ptr(), self.g_seg.data_ptr(), self.g_log_vars.data_ptr())          # -> seg_glogits, g_det, g_log_vars
        self.block.backward()                                                                          # gy -> gx (MaskCBAM's part), dL/dmask (its part of dL/dlogits; a gate's backward last)
        self._call(HEAD.bwd_entry, self._hb, self.n)                                               # gx += head's part; head parameter gradients

    def step(self):
        self.forward()
        self.backward()

    def check_handoff(self):
        if self.block_name == "cbam":                                  # the other blocks have no in-launch hand-off
            self.block.check_handoff()

    def launches(self) -> dict:
        t = "" if self._tgt is None else f"{self._tgt.launches} (targets) + "
        name = dict(cbam="MaskCBAM", eca="MaskECA", spade="MaskSPADE")[self.block_name]
        g = " + 1 (gate)" if self.gated else ""
        fwd, bwd = self.block.launch_counts()                          # what the block's library calls enqueue (plan.py)
        return dict(forward=f"{t}3 (heads){g} + {fwd} ({name}) + 2 (seg loss + Kendall)",
                    backward=f"1 (seg loss + Kendall) + {bwd} ({name}){g} + 5 (heads)")
