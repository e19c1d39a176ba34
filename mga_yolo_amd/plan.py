"""Static executor for the block over a feature pyramid: pre-allocated buffers, pre-built C-ABI level tables and
hipGraph capture of the step.  This is the launch path for steady-state training loops on MI355X -- the YOLOv8n shapes
are launch-latency bound (a full pass over the 52 MB P3 feature is ~10 us of HBM time), so the ~30 kernel launches of a
step are recorded once and replayed, instead of being issued from Python every step.

``PyramidPlan`` (MaskCBAM), ``EcaPyramidPlan`` and ``SpadePyramidPlan`` are one executor, ``_BlockPlan``: it owns, per level, x, mask, y,
gy, gx, gmask, ctx, scratch, the level tables, and ONE flat fp32 bucket holding the parameter gradients of all levels (what data-parallel
training all-reduces, see ``dp.py``), on NCHW or on ``torch.channels_last`` features.  A subclass states its ``family`` (_binding.Family:
level structs, layout flag, byte counts, fills, entry points, parameter names) and adds what only it has.

``PyramidPlan.forward`` / ``backward`` each make ONE library call on the current stream (5 kernel launches per step in total).
``backward_params`` + ``backward_inputs`` is the split form for callers that want the parameter gradients early (see ``dp.py``).

With ``gate`` (one ``GateConfig`` per level) the plan also runs the reference's ProbMaskGater between the mask it is given and the block
-- what a ``MGA_PROB_MODE`` training run does: it then owns ``logits`` (the gate's input, what the caller fills instead of ``mask``),
``msoft``, ``glogits`` (dL/dlogits, the gate's backward of ``gmask``) and ``rng_state``; ``forward`` is gate -> block and ``backward``
block -> gate, one more launch each.  The noise is drawn in the kernel from the Philox stream of include/mgagate.h, keyed by the
device-resident (seed, step) of ``rng_state`` that every forward advances: a captured graph replays with fresh noise.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._binding import CBAM, ECA, SPADE, Family, fill_gate, fill_resample
from .functional import (BlockConfig, GateConfig, SpadeConfig, ctx_views, gate_state, handoff_check, spade_check_norm, spade_kernel_reason,
                         stage_switches)

PARAM_NAMES, ECA_PARAM_NAMES, SPADE_PARAM_NAMES = CBAM.param_names, ECA.param_names, SPADE.param_names
GROUP_MAX = 4      # levels of one signature per launch (csrc/args.cuh: kGroupMax)


def _carve(bucket, params, off=0):
    """Views into the flat `bucket` from element `off` on, per level a list in the order and shape of `params` -> (views, the offset after
    them).  A block plan carves its own bucket from 0; slice.SlicePlan goes on behind it for the heads."""
    views = []
    for ps in params:
        lv = []
        for p in ps:
            lv.append(bucket[off:off + p.numel()].view(p.shape))
            off += p.numel()
        views.append(lv)
    return views, off


class _Executor:
    """What every static plan does with its library calls (the block plans below and slice.SlicePlan): issue them on the stream that is
    current on ``self.device``, and record them into a hipGraph."""

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, name: str, *args) -> None:
        """``lib.name(*args, current stream)``, checked: an attribute lookup and the call, as cheap as the line written out"""
        _lib.check(getattr(self.lib, name)(*args, self._stream()), name)

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

    def images(self) -> int:
        return self.shapes[0][0]


class _BlockPlan(_Executor):
    """The set-up the three pyramid plans share.  Per level it owns x / y / gy / gx (element type ``dtype``, NCHW or torch.channels_last),
    mask / gmask (fp32 (B,1,H,W), or None), ctx / scratch (zero-filled bytes: MaskCBAM's hand-off counters in ctx count from zero), the fp32
    clones of the parameters, their gradients as views into ONE flat fp32 ``grad_bucket`` -- the plan's own, or a caller's slice of a larger
    one -- and the two C-ABI level tables ``_fwd`` / ``_bwd``.

    A subclass states its ``family``, from which the struct types, the layout flag, the byte counts, the fills and the parameter names
    come; whatever else is its own (MaskCBAM's gate, workspace and projection flags, MaskSPADE's running statistics and mask sources) it
    builds in a ``_setup`` of its own around this one and in ``_level_own``.

    ``__init__`` and ``create`` of a subclass only name its arguments and hand them to ``_setup``.  There are two because the argument lists
    of the constructors are public and pinned (tests/test_gate_abi.py, test_opt_abi.py, test_abi_eca_nhwc.py): an option added later
    (PyramidPlan's ``channels_last``, EcaPyramidPlan's ``grad_bucket``) is a keyword of ``create``, which takes every argument of
    ``_setup``."""
    family: Family
    kind: str                                   # family.kind: what optim.plan_segments classifies the parameters by
    param_names: Tuple[str, ...]                # family.param_names: a level's parameters, in the order of ``params[l]`` and of the bucket
    grad_names: Tuple[str, ...]                 # the keys of named_param_grads: param_names unless the subclass says otherwise
    _defaults = dict(dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True, channels_last=False, grad_bucket=None)
    running: Sequence[tuple] = ()               # what _setup fills per level; optim.plan_segments finds none on a plan that was not set up

    def __init_subclass__(cls):
        cls.kind, cls.param_names = cls.family.kind, cls.family.param_names
        cls.grad_names = cls.__dict__.get("grad_names", cls.param_names)

    @classmethod
    def _create(cls, shapes, params, cfgs, kw):
        unknown = set(kw) - set(cls._defaults)
        if unknown:
            raise TypeError(f"{cls.__name__}.create: unexpected arguments {sorted(unknown)}")
        self = cls.__new__(cls)
        self._setup(shapes, params, cfgs, **{**cls._defaults, **kw})
        return self

    @staticmethod
    def _check_counts(shapes, params, cfgs) -> None:
        assert len(shapes) == len(params) == len(cfgs) and 1 <= len(shapes) <= _lib.MAX_LEVELS

    def _setup(self, shapes, params, cfgs, *, dtype, device, with_mask, want_gmask, channels_last, grad_bucket, running=None) -> None:
        """running: per level (running_mean, running_var, num_batches_tracked), (None, None, None) for a level that keeps no statistics --
        every level of MaskCBAM and MaskECA; MaskSPADE's plan passes its own."""
        self._check_counts(shapes, params, cfgs)
        self.running = [(None, None, None)] * len(shapes) if running is None else running
        self.lib = _lib.load()
        self.device = dev = torch.device(device)
        self.n, self.shapes, self.cfgs, self.dtype = len(shapes), list(shapes), list(cfgs), dtype
        self.with_mask, self.channels_last = bool(with_mask), bool(channels_last)
        fam = self.family
        flags = fam.layout_nhwc if self.channels_last else 0
        fmt = torch.channels_last if self.channels_last else torch.contiguous_format
        self.params = [[p.detach().to(dev, torch.float32).contiguous() for p in ps] for ps in params]
        n_grad = sum(p.numel() for ps in self.params for p in ps)
        if grad_bucket is None:
            grad_bucket = torch.zeros(n_grad, dtype=torch.float32, device=dev)
        assert grad_bucket.numel() == n_grad and grad_bucket.dtype == torch.float32 and grad_bucket.is_contiguous()
        self.grad_bucket, (self.param_grads, _) = grad_bucket, _carve(grad_bucket, self.params)
        self.x, self.mask, self.y, self.gy, self.gx, self.gmask, self.ctx, self.scratch = ([] for _ in range(8))
        self._fwd, self._bwd = (fam.fwd_level * self.n)(), (fam.bwd_level * self.n)()
        for l, ((B, C, H, W), cfg) in enumerate(zip(shapes, cfgs)):
            mk = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
            mkf = lambda: torch.zeros(B, C, H, W, dtype=dtype, device=dev).contiguous(memory_format=fmt)
            self.x.append(mkf()); self.y.append(mkf()); self.gy.append(mkf()); self.gx.append(mkf())
            self.mask.append(mk(B, 1, H, W) if with_mask else None)
            self.gmask.append(mk(B, 1, H, W) if (with_mask and want_gmask) else None)
            self.ctx.append(mk(fam.ctx_bytes((B, C, H, W), cfg, flags), dt=torch.uint8))
            self.scratch.append(mk(fam.scratch_bytes((B, C, H, W), cfg, flags), dt=torch.uint8))
            b = dict(x=self.x[l], mask=self.mask[l], y=self.y[l], gy=self.gy[l], gx=self.gx[l], gmask=self.gmask[l], ctx=self.ctx[l],
                     scratch=self.scratch[l], params=self.params[l], grads=self.param_grads[l], running=self.running[l],
                     save_gamma=self.with_mask)                 # (MaskSPADE: a plan's forward always keeps gamma for its backward)
            fwd_flags, bwd_flags = self._level_own(l, cfg, flags, b)
            fam.fill_fwd(self._fwd[l], cfg, fwd_flags, **b)
            fam.fill_bwd(self._bwd[l], cfg, bwd_flags, **b)

    def _level_own(self, l, cfg, flags, b: dict) -> Tuple[int, int]:
        return flags, flags     # what a subclass adds to level l before its tables are filled: buffers into `b` -> (forward's, backward's flags)

    def elements(self) -> int:
        """E = sum over levels of B*C*H*W."""
        return sum(B * C * H * W for B, C, H, W in self.shapes)

    def named_param_grads(self, level: int) -> dict:
        return dict(zip(self.grad_names, self.param_grads[level]))


class PyramidPlan(_BlockPlan):
    family, grad_names = CBAM, tuple("g" + n for n in CBAM.param_names)
    _defaults = dict(_BlockPlan._defaults, use_proj=False, fuse_forward=None, gate=None, seed=0)

    def __init__(self, shapes: Sequence[Tuple[int, int, int, int]], params: Sequence[Sequence[torch.Tensor]],
                 cfgs: Sequence[BlockConfig], dtype: torch.dtype = torch.float32, device="cuda",
                 with_mask: bool = True, want_gmask: bool = True, use_proj: bool = False,
                 fuse_forward: Optional[bool] = None, grad_bucket: Optional[torch.Tensor] = None,
                 gate: Optional[Sequence[GateConfig]] = None, seed: int = 0):
        self._setup(shapes, params, cfgs, dtype=dtype, device=device, with_mask=with_mask, want_gmask=want_gmask, use_proj=use_proj,
                    fuse_forward=fuse_forward, grad_bucket=grad_bucket, gate=gate, seed=seed, channels_last=False)

    @classmethod
    def create(cls, shapes, params, cfgs, *, channels_last: bool = False, **kw) -> "PyramidPlan":
        """The constructor with the feature layout as an argument.  channels_last=True allocates x / y / gy / gx in torch.channels_last and
        runs the channels-last kernels (MGACBAM_LAYOUT_NHWC: 4 launches forward, 7 backward, groups of their own without in-launch
        hand-offs); masks, parameters, their gradients and the gate are the same in both layouts.  **kw: the constructor's keyword arguments."""
        return cls._create(shapes, params, cfgs, dict(kw, channels_last=channels_last))

    def _setup(self, shapes, params, cfgs, *, use_proj, fuse_forward, gate, seed, channels_last, **common) -> None:
        if channels_last and use_proj:
            raise ValueError("PyramidPlan: use_proj with channels_last (the channels-last backward ignores the projection planes)")
        self._use_proj = bool(use_proj)
        # fuse_forward: k_chan + k_apply as ONE x-resident launch, k_gate (MGACBAM_FWD_FUSE); None = env MGACBAM_FUSE_FWD (on)
        # fold_backward: transposed conv folded into the k_bwd_reduce1 launch (MGACBAM_BWD_FOLD) whenever the whole backward is one call
        env_fuse, self.fold_backward = stage_switches()
        self.fuse_forward = env_fuse if fuse_forward is None else bool(fuse_forward)
        self.ws: List[Optional[torch.Tensor]] = []          # channels_last: the forward's per-chunk pooling partials
        super()._setup(shapes, params, cfgs, channels_last=channels_last, **common)
        self.gate = None if gate is None else list(gate)
        if self.gate is not None:
            self._init_gate(seed)

    def _level_own(self, l, cfg, flags, b):
        nws = CBAM.ws_bytes(self.shapes[l], cfg, flags)
        b["ws"] = torch.zeros(nws, dtype=torch.uint8, device=self.device) if nws else None
        self.ws.append(b["ws"])
        proj = self.gmask[l] is not None and self._use_proj      # the forward saves the W1-projection planes, the backward reads them
        return flags | (_lib.FWD_SAVE_PROJ if proj else 0), flags | (_lib.BWD_HAVE_PROJ if proj else 0)

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
    def forward(self, stages: int = _lib.FWD_ALL):
        if self.gate is not None and stages & _lib.FWD_STAGES["pool"]:     # the first stage reads the mask: the gate fills it before
            self._call("mgagate_forward", self._gate_fwd, self.n, self.rng_state.data_ptr())
        both = _lib.FWD_STAGES["chan"] | _lib.FWD_STAGES["apply"]
        if self.fuse_forward and (stages & both) == both:
            stages |= _lib.FWD_FUSE     # ctx is zero-filled at allocation, as the flag's contract asks
        self._call(CBAM.fwd_entry, self._fwd, self.n, stages)

    def check_handoff(self) -> None:
        """Synchronise and raise HandoffTimeout if any in-launch hand-off of any call on this plan timed out (status word of each
        level's ctx, include/mgacbam.h).  Callers invoke it where they synchronise anyway: bench.py after the timed region,
        training loops after a batch of graph replays."""
        torch.cuda.synchronize(self.device)
        handoff_check(((self.ctx[l], (*shp, self.cfgs[l].hidden)) for l, shp in enumerate(self.shapes)), lambda bad: f"levels {bad}")

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
        self._call(CBAM.bwd_entry, self._bwd, self.n, stages)
        if self.gate is not None and stages & _lib.BWD_STAGES["apply"] and self.glogits[0] is not None:   # k_bwd_apply has written gmask
            self._call("mgagate_backward", self._gate_bwd, self.n)

    def backward_params(self):
        """Every stage the parameter gradients depend on, as separate launches: they are complete when this returns to the
        stream, so a data-parallel caller can start their all-reduce and overlap it with ``backward_inputs``."""
        self.backward(_lib.BWD_PARAMS)

    def backward_inputs(self):
        """k_bwd_apply: gx and gmask."""
        self.backward(_lib.BWD_INPUTS)

    # ------------------------------------------------------------------ inspection
    def ctx_view(self, level: int) -> dict:
        B, C, H, W = self.shapes[level]
        return ctx_views(self.ctx[level], B, C, H, W, self.cfgs[level].hidden)

    def launch_counts(self) -> Tuple[int, int]:
        """Kernel launches of forward() and of backward() without the gate's (one each way): what csrc/api_fwd.hip / api_bwd.hip enqueue for
        one group of levels (the pyramid's levels share a signature)."""
        groups = -(-self.n // GROUP_MAX)
        return (4 * groups, 7 * groups) if self.channels_last else (2 * groups, 2 * groups)


class EcaPyramidPlan(_BlockPlan):
    """The same static executor for MaskECA: the parameter gradients are (conv1d.weight, beta) per level; ``forward`` /
    ``backward`` = one library call each (2 kernel launches each for all levels together).  ``channels_last=True`` runs the channels-last
    kernels (MGACBAM_LAYOUT_NHWC; 3 launches each way); masks and parameter gradients are the same in both layouts.  ``create`` takes
    ``grad_bucket=`` as well: a slice of a larger bucket owned by the caller (slice.SlicePlan)."""
    family = ECA

    def __init__(self, shapes, params, cfgs, dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True,
                 channels_last: bool = False):
        self._setup(shapes, params, cfgs, dtype=dtype, device=device, with_mask=with_mask, want_gmask=want_gmask,
                    channels_last=channels_last, grad_bucket=None)

    @classmethod
    def create(cls, shapes, params, cfgs, *, grad_bucket: Optional[torch.Tensor] = None, **kw) -> "EcaPyramidPlan":
        """The constructor with the gradient bucket as an argument.  **kw: the constructor's keyword arguments."""
        return cls._create(shapes, params, cfgs, dict(kw, grad_bucket=grad_bucket))

    def forward(self):
        self._call(ECA.fwd_entry, self._fwd, self.n)

    def backward(self):
        self._call(ECA.bwd_entry, self._bwd, self.n)

    def launch_counts(self) -> Tuple[int, int]:
        """Kernel launches of forward() and of backward() (csrc/api_eca.hip, per group of levels of one signature)."""
        groups = -(-self.n // GROUP_MAX)
        return (3 * groups, 3 * groups) if self.channels_last else (2 * groups, 2 * groups)


class SpadePyramidPlan(_BlockPlan):
    """The static executor for MaskSPADE (include/mgaspade.h): ctx is the full mgaspade_ctx_bytes (the forward keeps gamma for the backward),
    for norm_type 'bn' the plan owns the running statistics (``running``, updated in place by a training forward), and the bucket holds the six
    parameter gradients of all levels in the order of ``params`` = (shared.0.weight, shared.0.bias, conv_gamma.weight, conv_gamma.bias,
    conv_beta.weight, conv_beta.bias).  ``forward`` / ``backward`` = one library call each on the current stream.  ``channels_last=True``
    (MGASPADE_LAYOUT_NHWC) gives the NCHW plan's results bit for bit.  A configuration the kernels do not take
    (functional.spade_kernel_reason) raises ValueError: a static plan has no torch composition to run instead.

    ``mask_hw`` = per level (h, w) or None: such a level gets its mask at that resolution (masked_spade.py:102-110).  The plan then owns
    ``mask_src[l]`` (B,1,h,w) fp32, which the caller fills instead of ``mask[l]``, and ``gmask_src[l]``; ``forward`` first resamples
    mask_src -> mask and ``backward`` last resamples gmask -> gmask_src (include/mgaresample.h), one launch each for all such levels."""
    family = SPADE

    def __init__(self, shapes, params, cfgs: Sequence[SpadeConfig], dtype=torch.float32, device="cuda", with_mask=True, want_gmask=True,
                 channels_last: bool = False, grad_bucket: Optional[torch.Tensor] = None, running=None, mask_hw=None):
        self._setup(shapes, params, cfgs, dtype=dtype, device=device, with_mask=with_mask, want_gmask=want_gmask,
                    channels_last=channels_last, grad_bucket=grad_bucket, running=running, mask_hw=mask_hw)

    def _setup(self, shapes, params, cfgs, *, running, mask_hw, dtype, device, with_mask, **common) -> None:
        self._check_counts(shapes, params, cfgs)
        for (B, C, H, W), cfg in zip(shapes, cfgs):
            x = torch.empty(B, C, H, W, dtype=dtype, device="meta")              # shape and element type only: nothing is allocated
            why = spade_kernel_reason(x, torch.empty(B, 1, H, W, device="meta") if with_mask else None, cfg)
            if why is None and cfg.mask_channels > 1:
                why = "mask_channels > 1"
            if why is not None:
                raise ValueError(f"SpadePyramidPlan: {why}")
            spade_check_norm(x, cfg)
        dev, f32 = torch.device(device), torch.float32
        runs: List[tuple] = []
        for l, ((_, C, _, _), cfg) in enumerate(zip(shapes, cfgs)):
            run = (None, None, None)
            if cfg.bn:
                given = running[l] if running is not None and running[l] is not None else None
                if given is not None:
                    run = (given[0].detach().to(dev, f32).clone(), given[1].detach().to(dev, f32).clone(),
                           given[2].detach().to(dev, torch.int64).clone())
                else:
                    run = (torch.zeros(C, dtype=f32, device=dev), torch.ones(C, dtype=f32, device=dev), torch.zeros((), dtype=torch.int64, device=dev))
            runs.append(run)
        mask_hw = [None] * len(shapes) if mask_hw is None else list(mask_hw)
        assert len(mask_hw) == len(shapes) and (with_mask or all(hw is None for hw in mask_hw)), "mask_hw: one entry per level, and with_mask"
        self.mask_hw = mask_hw
        super()._setup(shapes, params, cfgs, dtype=dtype, device=device, with_mask=with_mask, running=runs, **common)
        # ---- the levels whose mask comes at another resolution: their sources and the resample tables, one launch per direction
        src = lambda l, like: None if mask_hw[l] is None or like is None else torch.zeros(shapes[l][0], 1, *mask_hw[l], dtype=f32, device=dev)
        self.mask_src = [src(l, self.mask[l]) for l in range(self.n)]
        self.gmask_src = [src(l, self.gmask[l]) for l in range(self.n)]
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

    def forward(self):
        if self._n_rs:
            self._call("mgaspade_resample_forward", self._rs_fwd, self._n_rs)
        self._call(SPADE.fwd_entry, self._fwd, self.n)

    def backward(self):
        self._call(SPADE.bwd_entry, self._bwd, self.n)
        if self._n_rs_bwd:
            self._call("mgaspade_resample_backward", self._rs_bwd, self._n_rs_bwd)

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
