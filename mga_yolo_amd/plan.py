"""Static executor for the block over a feature pyramid: pre-allocated buffers, pre-built C-ABI level tables and
hipGraph capture of the step.  This is the launch path for steady-state training loops on MI355X -- the YOLOv8n shapes
are launch-latency bound (a full pass over the 52 MB P3 feature is ~10 us of HBM time), so the ~30 kernel launches of a
step are recorded once and replayed, instead of being issued from Python every step.

A ``PyramidPlan`` owns, per level: x, mask, y, gy, gx, gmask, ctx, scratch; and ONE flat fp32 bucket holding the parameter
gradients of all levels (what data-parallel training all-reduces, see ``dp.py``).  ``forward`` / ``backward`` each make ONE
library call on the current stream (5 kernel launches per step in total).  ``backward_params`` + ``backward_inputs`` is
the split form for callers that want the parameter gradients early (see ``dp.py``).

With ``gate`` (one ``GateConfig`` per level) the plan also runs the reference's ProbMaskGater between the mask it is given and the block
-- what a ``MGA_PROB_MODE`` training run does: it then owns ``logits`` (the gate's input, what the caller fills instead of ``mask``),
``msoft``, ``glogits`` (dL/dlogits, the gate's backward of ``gmask``) and ``rng_state``; ``forward`` is gate -> block and ``backward``
block -> gate, one more launch each.  The noise is drawn in the kernel from the Philox stream of include/mgagate.h, keyed by the
device-resident (seed, step) of ``rng_state`` that every forward advances: a captured graph replays with fresh noise.

``EcaPyramidPlan`` and ``SpadePyramidPlan`` are the same executor for MaskECA and MaskSPADE.  Every plan runs on NCHW or on
``torch.channels_last`` features.  ``PyramidPlan`` and ``EcaPyramidPlan`` keep the constructor arguments they always had; their ``create``
classmethods are the same constructors with the newer keywords (``channels_last=`` / ``grad_bucket=``).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import os

import torch

from . import _lib
from ._binding import fill_cbam_bwd, fill_cbam_fwd, fill_eca_bwd, fill_eca_fwd, fill_gate, fill_resample, fill_spade
from .functional import BlockConfig, GateConfig, HandoffTimeout, SpadeConfig, ctx_views, gate_state, spade_check_norm, spade_kernel_reason

PARAM_NAMES = ("w1", "b1", "w2", "b2", "wsa", "beta")
ECA_PARAM_NAMES = ("conv1d.weight", "beta")
SPADE_PARAM_NAMES = ("shared.0.weight", "shared.0.bias", "conv_gamma.weight", "conv_gamma.bias", "conv_beta.weight", "conv_beta.bias")
GROUP_MAX = 4      # levels of one signature per launch (csrc/args.cuh: kGroupMax)


def _bucket(params, grad_bucket, dev):
    """The flat fp32 gradient bucket of `params` (per level a list of tensors) and, per level, views into it in the order of the parameters.
    grad_bucket: a slice of a larger bucket owned by the caller (slice.SlicePlan), or None."""
    n_grad = sum(p.numel() for ps in params for p in ps)
    if grad_bucket is not None:
        assert grad_bucket.numel() == n_grad and grad_bucket.dtype == torch.float32 and grad_bucket.is_contiguous()
    else:
        grad_bucket = torch.zeros(n_grad, dtype=torch.float32, device=dev)
    views, off = [], 0
    for ps in params:
        lv = []
        for p in ps:
            lv.append(grad_bucket[off:off + p.numel()].view(p.shape))
            off += p.numel()
        views.append(lv)
    return grad_bucket, views


class PyramidPlan:
    def __init__(self, shapes: Sequence[Tuple[int, int, int, int]], params: Sequence[Sequence[torch.Tensor]],
                 cfgs: Sequence[BlockConfig], dtype: torch.dtype = torch.float32, device="cuda",
                 with_mask: bool = True, want_gmask: bool = True, use_proj: bool = False,
                 fuse_forward: Optional[bool] = None, grad_bucket: Optional[torch.Tensor] = None,
                 gate: Optional[Sequence[GateConfig]] = None, seed: int = 0):
        self._setup(shapes, params, cfgs, dtype, device, with_mask, want_gmask, use_proj, fuse_forward, grad_bucket, gate, seed, False)

    @classmethod
    def create(cls, shapes, params, cfgs, *, channels_last: bool = False, **kw) -> "PyramidPlan":
        """The constructor with the feature layout as an argument (the constructor's own argument list is what every caller passes today
        and stays as it is).  channels_last=True allocates x / y / gy / gx in torch.channels_last and runs the channels-last kernels
        (MGACBAM_LAYOUT_NHWC: 4 launches forward, 7 backward, groups of their own without in-launch hand-offs); masks, parameters,
        their gradients and the gate are the same in both layouts.  **kw: the constructor's keyword arguments."""
        self = cls.__new__(cls)
        defaults = dict(dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True, use_proj=False, fuse_forward=None,
                        grad_bucket=None, gate=None, seed=0)
        unknown = set(kw) - set(defaults)
        if unknown:
            raise TypeError(f"PyramidPlan.create: unexpected arguments {sorted(unknown)}")
        defaults.update(kw)
        self._setup(shapes, params, cfgs, channels_last=channels_last, **defaults)
        return self

    def _setup(self, shapes, params, cfgs, dtype, device, with_mask, want_gmask, use_proj, fuse_forward, grad_bucket, gate, seed,
               channels_last) -> None:
        self.channels_last = bool(channels_last)
        if self.channels_last and use_proj:
            raise ValueError("PyramidPlan: use_proj with channels_last (the channels-last backward ignores the projection planes)")
        flags = _lib.LAYOUT_NHWC if self.channels_last else 0
        fmt = torch.channels_last if self.channels_last else torch.contiguous_format
        # fuse_forward: k_chan + k_apply as ONE x-resident launch, k_gate (MGACBAM_FWD_FUSE); None = env MGACBAM_FUSE_FWD (on)
        self.fuse_forward = bool(int(os.environ.get("MGACBAM_FUSE_FWD", "1"))) if fuse_forward is None else bool(fuse_forward)
        # transposed conv folded into the k_bwd_reduce1 launch (MGACBAM_BWD_FOLD) whenever the whole backward is one call
        self.fold_backward = bool(int(os.environ.get("MGACBAM_FOLD_BWD", "1")))
        assert len(shapes) == len(params) == len(cfgs) and 1 <= len(shapes) <= _lib.MAX_LEVELS
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n = len(shapes)
        self.shapes, self.cfgs, self.dtype = list(shapes), list(cfgs), dtype
        self.params = [[p.detach().to(self.device, torch.float32).contiguous() for p in ps] for ps in params]
        dev = self.device
        self.x, self.mask, self.y, self.gy, self.gx, self.gmask, self.ctx, self.scratch = ([] for _ in range(8))
        self.ws: List[Optional[torch.Tensor]] = []          # channels_last: the forward's per-chunk pooling partials
        self.grad_bucket, self.param_grads = _bucket(self.params, grad_bucket, dev)     # (a caller's slice: slice.SlicePlan)
        self._fwd = (_lib.FwdLevel * self.n)()
        self._bwd = (_lib.BwdLevel * self.n)()
        for l, ((B, C, H, W), ps, cfg) in enumerate(zip(shapes, self.params, cfgs)):
            mk = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt, device=dev)
            mkf = lambda: torch.zeros(B, C, H, W, dtype=dtype, device=dev).contiguous(memory_format=fmt)
            self.x.append(mkf()); self.y.append(mkf()); self.gy.append(mkf()); self.gx.append(mkf())
            self.mask.append(mk(B, 1, H, W, dt=torch.float32) if with_mask else None)
            self.gmask.append(mk(B, 1, H, W, dt=torch.float32) if (with_mask and want_gmask) else None)
            self.ctx.append(torch.zeros(_lib.ctx_bytes(B, C, H, W, cfg.hidden), dtype=torch.uint8, device=dev))
            self.scratch.append(torch.zeros(_lib.scratch_bytes(B, C, H, W, cfg.hidden, cfg.k, flags), dtype=torch.uint8, device=dev))
            self.ws.append(torch.zeros(_lib.fwd_ws_bytes(B, C, H, W, cfg.hidden, flags), dtype=torch.uint8, device=dev) if flags else None)
            views = self.param_grads[l]
            proj = with_mask and want_gmask and use_proj     # the forward saves the W1-projection planes, the backward reads them
            fill_cbam_fwd(self._fwd[l], self.x[l], self.mask[l], self.y[l], self.ctx[l], ps, cfg, flags | (_lib.FWD_SAVE_PROJ if proj else 0),
                          self.ws[l])
            fill_cbam_bwd(self._bwd[l], self.x[l], self.mask[l], self.gy[l], self.ctx[l], self.scratch[l], self.gx[l], self.gmask[l],
                          views, ps, cfg, flags | (_lib.BWD_HAVE_PROJ if proj else 0))
        self.gate = None if gate is None else list(gate)
        if self.gate is not None:
            self._init_gate(seed)

    def _init_gate(self, seed: int) -> None:
        """logits -> [gate] -> mask, gmask -> [gate backward] -> glogits: the buffers and the two level tables (include/mgagate.h)"""
        assert len(self.gate) == self.n and all(m is not None for m in self.mask), "a gate needs one GateConfig per level and with_mask"
        self.logits = [torch.zeros_like(m) for m in self.mask]
        self.msoft = [torch.zeros_like(m) for m in self.mask]
        self.glogits = [None if g is None else torch.zeros_like(g) for g in self.gmask]
        self.rng_state = gate_state(seed, 0, self.device)
        self._gate_fwd, self._gate_bwd = (_lib.GateLevel * self.n)(), (_lib.GateLevel * self.n)()
        for l, c in enumerate(self.gate):
            a = (c.code(), c.stream(l), c.tau, c.p_min, c.threshold)
            fill_gate(self._gate_fwd[l], self.logits[l], self.mask[l], self.msoft[l], None, None, *a)
            if self.glogits[l] is not None:
                fill_gate(self._gate_bwd[l], self.logits[l], None, self.msoft[l], self.gmask[l], self.glogits[l], *a)

    # ------------------------------------------------------------------ library calls on the current stream
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def forward(self, stages: int = _lib.FWD_ALL):
        if self.gate is not None and stages & _lib.FWD_STAGES["pool"]:     # the first stage reads the mask: the gate fills it before
            _lib.check(self.lib.mgagate_forward(self._gate_fwd, self.n, self.rng_state.data_ptr(), self._stream()), "mgagate_forward")
        both = _lib.FWD_STAGES["chan"] | _lib.FWD_STAGES["apply"]
        if self.fuse_forward and (stages & both) == both:
            stages |= _lib.FWD_FUSE     # ctx is zero-filled at allocation, as the flag's contract asks
        _lib.check(self.lib.mgacbam_forward_stages(self._fwd, self.n, stages, self._stream()), "mgacbam_forward_stages")

    def check_handoff(self) -> None:
        """Synchronise and raise HandoffTimeout if any in-launch hand-off of any call on this plan timed out (status word of each
        level's ctx, include/mgacbam.h).  Callers invoke it where they synchronise anyway: bench.py after the timed region,
        training loops after a batch of graph replays."""
        torch.cuda.synchronize(self.device)
        words = []
        for l, (B, C, H, W) in enumerate(self.shapes):
            off = _lib.ctx_layout(B, C, H, W, self.cfgs[l].hidden)["status"]
            words.append(self.ctx[l][off:off + 4].view(torch.int32))
        bad = [self.shapes[l] for l, w in enumerate(torch.cat(words).cpu().tolist()) if w != 0]
        if bad:
            raise HandoffTimeout(f"in-launch hand-off timed out for levels {bad}: affected tiles were poisoned with NaN "
                                 "(is the GPU shared with other work?  MGACBAM_FUSE_FWD=0 runs without hand-offs)")

    def gate_active(self) -> bool:
        """True when the last fused forward really ran k_gate (the library falls back to k_chan + k_apply for groups with a
        level whose shape is not eligible): k_gate bumps the hand-off flags at the end of ctx, the fallback never touches them."""
        if not self.fuse_forward or self.channels_last:      # channels-last levels run in groups of their own, without hand-offs
            return False
        torch.cuda.synchronize(self.device)
        return all(int(self.ctx_view(l)["sync"][_lib.sync_slices(*shp)["gate"]].max()) != 0 for l, shp in enumerate(self.shapes))

    def fold_active(self) -> bool:
        """True when MGACBAM_BWD_FOLD really folds the transposed conv into the k_bwd_reduce1 launch for these shapes (the library
        falls back to two launches for ineligible groups): the folded launch bumps the backward hand-off counters."""
        if not self.fold_backward or self.channels_last:     # the channels-last backward has no folded launch
            return False
        B = _lib.BWD_STAGES

        def counters():
            torch.cuda.synchronize(self.device)
            out = []
            for l, shp in enumerate(self.shapes):
                out.append(self.ctx_view(l)["sync"][_lib.sync_slices(*shp)["tiles"]].clone())
            return out
        self.forward()
        before = counters()
        self.backward(B["reduce1"] | B["convT"] | _lib.BWD_FOLD)
        after = counters()
        self.backward(_lib.BWD_ALL & ~(B["reduce1"] | B["convT"]))      # finishes the step
        torch.cuda.synchronize(self.device)
        return all(not torch.equal(a, b) for a, b in zip(before, after))

    def backward(self, stages: int = _lib.BWD_ALL):
        if stages == _lib.BWD_ALL and self.fold_backward:
            stages |= _lib.BWD_FOLD     # ctx is zero-filled at allocation, as the flag's contract asks
        _lib.check(self.lib.mgacbam_backward_stages(self._bwd, self.n, stages, self._stream()), "mgacbam_backward_stages")
        if self.gate is not None and stages & _lib.BWD_STAGES["apply"] and self.glogits[0] is not None:   # k_bwd_apply has written gmask
            _lib.check(self.lib.mgagate_backward(self._gate_bwd, self.n, self._stream()), "mgagate_backward")

    def backward_params(self):
        """Every stage the parameter gradients depend on, as separate launches: they are complete when this returns to the
        stream, so a data-parallel caller can start their all-reduce and overlap it with ``backward_inputs``."""
        self.backward(_lib.BWD_PARAMS)

    def backward_inputs(self):
        """k_bwd_apply: gx and gmask."""
        self.backward(_lib.BWD_INPUTS)

    # ------------------------------------------------------------------ hipGraph capture
    def capture(self, fn) -> "torch.cuda.CUDAGraph":
        """Record ``fn()`` (library calls on this plan) into a graph; warm up on a side stream first, as capture requires."""
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        return g

    # ------------------------------------------------------------------ sizes / inspection
    def elements(self) -> int:
        """E = sum over levels of B*C*H*W."""
        return sum(B * C * H * W for B, C, H, W in self.shapes)

    def images(self) -> int:
        return self.shapes[0][0]

    def ctx_view(self, level: int) -> dict:
        B, C, H, W = self.shapes[level]
        return ctx_views(self.ctx[level], B, C, H, W, self.cfgs[level].hidden)

    def named_param_grads(self, level: int) -> dict:
        return dict(zip(("g" + n for n in PARAM_NAMES), self.param_grads[level]))

    def launch_counts(self) -> Tuple[int, int]:
        """Kernel launches of forward() and of backward() without the gate's (one each way): what csrc/api_fwd.hip / api_bwd.hip enqueue for
        one group of levels (the pyramid's levels share a signature)."""
        groups = -(-self.n // GROUP_MAX)
        return (4 * groups, 7 * groups) if self.channels_last else (2 * groups, 2 * groups)


class EcaPyramidPlan:
    """The same static executor for MaskECA: per level x, mask, y, gy, gx, gmask, ctx, scratch and one flat bucket
    with the parameter gradients (conv1d.weight, beta) of all levels; ``forward`` / ``backward`` = one library call each
    (2 kernel launches each for all levels together).  ``channels_last=True`` allocates x / y / gy / gx in torch.channels_last and runs the
    channels-last kernels (MGACBAM_LAYOUT_NHWC; 3 launches each way); masks and parameter gradients are the same in both layouts.
    ``create`` is the constructor with ``grad_bucket=``: a slice of a larger bucket owned by the caller (slice.SlicePlan), as in PyramidPlan."""

    def __init__(self, shapes, params, cfgs, dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True,
                 channels_last: bool = False):
        self._setup(shapes, params, cfgs, dtype, device, with_mask, want_gmask, channels_last, None)

    @classmethod
    def create(cls, shapes, params, cfgs, *, grad_bucket: Optional[torch.Tensor] = None, **kw) -> "EcaPyramidPlan":
        """The constructor with the gradient bucket as an argument (the constructor's own argument list stays as it is).  **kw: the
        constructor's keyword arguments."""
        self = cls.__new__(cls)
        args = dict(dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True, channels_last=False)
        unknown = set(kw) - set(args)
        if unknown:
            raise TypeError(f"EcaPyramidPlan.create: unexpected arguments {sorted(unknown)}")
        args.update(kw)
        self._setup(shapes, params, cfgs, grad_bucket=grad_bucket, **args)
        return self

    def _setup(self, shapes, params, cfgs, dtype, device, with_mask, want_gmask, channels_last, grad_bucket) -> None:
        assert len(shapes) == len(params) == len(cfgs) and 1 <= len(shapes) <= _lib.MAX_LEVELS
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n, self.shapes, self.cfgs, self.dtype = len(shapes), list(shapes), list(cfgs), dtype
        self.channels_last = bool(channels_last)
        flags = _lib.LAYOUT_NHWC if self.channels_last else 0
        fmt = torch.channels_last if self.channels_last else torch.contiguous_format
        dev = self.device
        self.params = [[p.detach().to(dev, torch.float32).contiguous() for p in ps] for ps in params]
        self.x, self.mask, self.y, self.gy, self.gx, self.gmask, self.ctx, self.scratch = ([] for _ in range(8))
        self.grad_bucket, self.param_grads = _bucket(self.params, grad_bucket, dev)
        self._fwd, self._bwd = (_lib.EcaFwdLevel * self.n)(), (_lib.EcaBwdLevel * self.n)()
        for l, ((B, C, H, W), (w, beta), cfg) in enumerate(zip(shapes, self.params, cfgs)):
            mk = lambda *s_, dt=dtype: torch.zeros(*s_, dtype=dt, device=dev)
            mkf = lambda: torch.zeros(B, C, H, W, dtype=dtype, device=dev).contiguous(memory_format=fmt)
            self.x.append(mkf()); self.y.append(mkf()); self.gy.append(mkf()); self.gx.append(mkf())
            self.mask.append(mk(B, 1, H, W, dt=torch.float32) if with_mask else None)
            self.gmask.append(mk(B, 1, H, W, dt=torch.float32) if (with_mask and want_gmask) else None)
            self.ctx.append(torch.zeros(_lib.eca_ctx_bytes(B, C, H, W, flags), dtype=torch.uint8, device=dev))
            self.scratch.append(torch.zeros(_lib.eca_scratch_bytes(B, C, H, W, flags), dtype=torch.uint8, device=dev))
            gw, gb = self.param_grads[l]
            fill_eca_fwd(self._fwd[l], self.x[l], self.mask[l], self.y[l], self.ctx[l], w, beta, cfg, flags)
            fill_eca_bwd(self._bwd[l], self.x[l], self.mask[l], self.gy[l], self.ctx[l], self.scratch[l], self.gx[l], self.gmask[l],
                         gw, gb, w, beta, cfg, flags)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def forward(self):
        _lib.check(self.lib.mgacbam_eca_forward(self._fwd, self.n, self._stream()), "mgacbam_eca_forward")

    def backward(self):
        _lib.check(self.lib.mgacbam_eca_backward(self._bwd, self.n, self._stream()), "mgacbam_eca_backward")

    capture = PyramidPlan.capture

    def elements(self) -> int:
        return sum(B * C * H * W for B, C, H, W in self.shapes)

    def images(self) -> int:
        return self.shapes[0][0]

    def named_param_grads(self, level: int) -> dict:
        return dict(zip(ECA_PARAM_NAMES, self.param_grads[level]))

    def launch_counts(self) -> Tuple[int, int]:
        """Kernel launches of forward() and of backward() (csrc/api_eca.hip, per group of levels of one signature)."""
        groups = -(-self.n // GROUP_MAX)
        return (3 * groups, 3 * groups) if self.channels_last else (2 * groups, 2 * groups)


class SpadePyramidPlan:
    """The static executor for MaskSPADE (include/mgaspade.h): per level x, mask, y, gy, gx, gmask, ctx (the full mgaspade_ctx_bytes: the
    forward keeps gamma for the backward), scratch, for norm_type 'bn' the running statistics (updated in place by a training forward), and
    ONE flat fp32 bucket with the six parameter gradients of all levels in the order of ``params`` = (shared.0.weight, shared.0.bias,
    conv_gamma.weight, conv_gamma.bias, conv_beta.weight, conv_beta.bias).  ``forward`` / ``backward`` = one library call each on the current
    stream.  ``channels_last=True`` allocates x / y / gy / gx in torch.channels_last (MGASPADE_LAYOUT_NHWC): the results are the NCHW plan's
    bit for bit.  A configuration the kernels do not take (functional.spade_kernel_reason) raises ValueError: a static plan has no torch
    composition to run instead.

    ``mask_hw`` = per level (h, w) or None: such a level gets its mask at that resolution (masked_spade.py:102-110).  The plan then owns
    ``mask_src[l]`` (B,1,h,w) fp32, which the caller fills instead of ``mask[l]``, and ``gmask_src[l]``; ``forward`` first resamples
    mask_src -> mask and ``backward`` last resamples gmask -> gmask_src (include/mgaresample.h), one launch each for all such levels."""

    def __init__(self, shapes, params, cfgs: Sequence[SpadeConfig], dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True,
                 channels_last: bool = False, grad_bucket: Optional[torch.Tensor] = None, running=None, mask_hw=None):
        assert len(shapes) == len(params) == len(cfgs) and 1 <= len(shapes) <= _lib.MAX_LEVELS
        for (B, C, H, W), cfg in zip(shapes, cfgs):
            x = torch.empty(B, C, H, W, dtype=dtype, device="meta")              # shape and element type only: nothing is allocated
            why = spade_kernel_reason(x, torch.empty(B, 1, H, W, device="meta") if with_mask else None, cfg)
            if why is None and cfg.mask_channels > 1:
                why = "mask_channels > 1"
            if why is not None:
                raise ValueError(f"SpadePyramidPlan: {why}")
            spade_check_norm(x, cfg)
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n, self.shapes, self.cfgs, self.dtype = len(shapes), list(shapes), list(cfgs), dtype
        self.with_mask, self.channels_last = bool(with_mask), bool(channels_last)
        flags = _lib.SPADE_LAYOUT_NHWC if self.channels_last else 0
        fmt = torch.channels_last if self.channels_last else torch.contiguous_format
        dev = self.device
        f32 = torch.float32
        self.params = [[p.detach().to(dev, f32).contiguous() for p in ps] for ps in params]
        self.x, self.mask, self.y, self.gy, self.gx, self.gmask, self.ctx, self.scratch = ([] for _ in range(8))
        self.running: List[Optional[tuple]] = []
        self.grad_bucket, self.param_grads = _bucket(self.params, grad_bucket, dev)
        self._fwd, self._bwd = (_lib.SpadeLevel * self.n)(), (_lib.SpadeLevel * self.n)()
        mask_hw = [None] * self.n if mask_hw is None else list(mask_hw)
        assert len(mask_hw) == self.n and (with_mask or all(hw is None for hw in mask_hw)), "mask_hw: one entry per level, and with_mask"
        self.mask_hw = mask_hw
        self.mask_src: List[Optional[torch.Tensor]] = []
        self.gmask_src: List[Optional[torch.Tensor]] = []
        for l, ((B, C, H, W), ps, cfg) in enumerate(zip(shapes, self.params, cfgs)):
            mkf = lambda: torch.zeros(B, C, H, W, dtype=dtype, device=dev).contiguous(memory_format=fmt)
            self.x.append(mkf()); self.y.append(mkf()); self.gy.append(mkf()); self.gx.append(mkf())
            self.mask.append(torch.zeros(B, 1, H, W, dtype=f32, device=dev) if with_mask else None)
            self.gmask.append(torch.zeros(B, 1, H, W, dtype=f32, device=dev) if (with_mask and want_gmask) else None)
            self.ctx.append(torch.zeros(_lib.spade_ctx_bytes(B, C, H, W, cfg.hidden), dtype=torch.uint8, device=dev))
            self.scratch.append(torch.zeros(_lib.spade_scratch_bytes(B, C, H, W, cfg.hidden), dtype=torch.uint8, device=dev))
            run = (None, None, None)
            if cfg.bn:
                given = running[l] if running is not None and running[l] is not None else None
                if given is not None:
                    run = (given[0].detach().to(dev, f32).clone(), given[1].detach().to(dev, f32).clone(),
                           given[2].detach().to(dev, torch.int64).clone())
                else:
                    run = (torch.zeros(C, dtype=f32, device=dev), torch.ones(C, dtype=f32, device=dev), torch.zeros((), dtype=torch.int64, device=dev))
            self.running.append(run)
            lp, lg = (ps, self.param_grads[l]) if with_mask else ([None] * 6, [None] * 6)      # a level without a mask reads no parameter
            fill_spade(self._fwd[l], self.x[l], self.mask[l], lp, cfg, run, self.ctx[l], y=self.y[l], save_gamma=with_mask, flags=flags)
            fill_spade(self._bwd[l], self.x[l], self.mask[l], lp, cfg, run, self.ctx[l], gy=self.gy[l], gx=self.gx[l], gmask=self.gmask[l],
                       pgrads=lg, scratch=self.scratch[l], flags=flags)
            hw = mask_hw[l]
            self.mask_src.append(None if hw is None else torch.zeros(B, 1, *hw, dtype=f32, device=dev))
            self.gmask_src.append(None if hw is None or self.gmask[l] is None else torch.zeros(B, 1, *hw, dtype=f32, device=dev))
        # ---- the resample tables: the levels whose mask comes at another resolution, one launch per direction
        rs = [l for l in range(self.n) if mask_hw[l] is not None]
        self._n_rs = len(rs)
        self._n_rs_bwd = sum(self.gmask_src[l] is not None for l in rs)
        self._rs_fwd, self._rs_bwd = (_lib.ResampleLevel * max(self._n_rs, 1))(), (_lib.ResampleLevel * max(self._n_rs_bwd, 1))()
        j = 0
        for i, l in enumerate(rs):
            H, W = shapes[l][2:]
            fill_resample(self._rs_fwd[i], self.mask_src[l], self.mask[l], mask_hw[l], (H, W))
            if self.gmask_src[l] is not None:
                fill_resample(self._rs_bwd[j], self.gmask[l], self.gmask_src[l], mask_hw[l], (H, W))
                j += 1

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def forward(self):
        st = self._stream()
        if self._n_rs:
            _lib.check(self.lib.mgaspade_resample_forward(self._rs_fwd, self._n_rs, st), "mgaspade_resample_forward")
        _lib.check(self.lib.mgaspade_forward(self._fwd, self.n, st), "mgaspade_forward")

    def backward(self):
        st = self._stream()
        _lib.check(self.lib.mgaspade_backward(self._bwd, self.n, st), "mgaspade_backward")
        if self._n_rs_bwd:
            _lib.check(self.lib.mgaspade_resample_backward(self._rs_bwd, self._n_rs_bwd, st), "mgaspade_resample_backward")

    capture = PyramidPlan.capture

    def elements(self) -> int:
        return sum(B * C * H * W for B, C, H, W in self.shapes)

    def images(self) -> int:
        return self.shapes[0][0]

    def named_param_grads(self, level: int) -> dict:
        return dict(zip(SPADE_PARAM_NAMES, self.param_grads[level]))

    def launch_counts(self) -> Tuple[int, int]:
        """Kernel launches of forward() and of backward(), as csrc/api_spade.hip enqueues them per group of levels (a plan's levels share
        element type, layout, mask and dL/dmask: one signature).  Forward: statistics, weight pack, the fused conv + FiLM launch; a
        channels-last group with a batch-norm level in training runs three more statistics launches; without a mask: statistics and the
        element-wise apply.  Backward: reduce, fin, dW, dW fin, dh, dW0 fin, [dL/dmask], apply; without a mask: reduce, fin, apply.  A mask
        at another resolution adds one launch each way."""
        groups = -(-self.n // GROUP_MAX)
        bn_train = any(c.bn and c.training for c in self.cfgs)
        stats = 4 if (self.channels_last and bn_train) else 1
        fwd = (stats + 2 if self.with_mask else stats + 1) * groups + (1 if self._n_rs else 0)
        has_gmask = any(g is not None for g in self.gmask)
        bwd = ((7 + (1 if has_gmask else 0)) if self.with_mask else 3) * groups + (1 if self._n_rs_bwd else 0)
        return fwd, bwd
