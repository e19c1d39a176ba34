"""The optimizer step of the static plans, device-resident and fused over their flat gradient bucket (include/mgaopt.h, csrc/opt.cuh).

What the reference's trainer runs after every backward (U/engine/trainer.py:710-718) -- GradScaler.unscale_ with the non-finite check,
clip_grad_norm_(max_norm=10.0), the optimizer step (nesterov SGD or AdamW, three parameter groups: trainer.py:915-941), ModelEMA.update
(U/utils/torch_utils.py:759-775) -- as TWO kernel launches over every parameter tensor of a plan, plus one per accumulated micro-step:

    plan = SlicePlan.create(...)
    opt = BucketOptimizer.for_plan(plan, OptConfig("adamw", lr=1e-3, weight_decay=5e-4))
    graph = plan.capture(lambda: (plan.step(), opt.step()))
    for it in range(n):
        opt.set_group(0, lr=..., momentum=...)     # warm-up (trainer.py:463-474): a host write into the device block, no re-capture
        graph.replay()

The plans keep the very tensors the kernels read in ``plan.params`` / ``head_params`` / ``log_vars``, so the step updates them in place and the
captured graph sees the result.  Everything that changes from step to step -- learning rates, momentum, the loss scale, the step counters,
the squared gradient norm of the rest of the model -- is read from device memory (``opt.hyper``).  On CPU tensors ``step()`` runs a torch
restatement of the same arithmetic, as the modules do."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from ._binding import call, fill_opt_segment
from .plan import _BlockPlan
from .slice import HEAD_PARAM_NAMES, SlicePlan

GROUP_BIAS, GROUP_DECAY, GROUP_NORM = 0, 1, 2         # optimizer.param_groups after build_optimizer (trainer.py:929, 940, 941)
# plan-side parameter names -> the reference modules' names (MaskECA's, MaskSPADE's and the head's already are the reference's)
CBAM_REFERENCE_NAMES = dict(w1="cam_mlp.0.weight", b1="cam_mlp.0.bias", w2="cam_mlp.2.weight", b2="cam_mlp.2.bias", wsa="sam_conv.weight", beta="beta")
# sub-modules that are normalisation layers (isinstance(module, bn) at trainer.py:920): MGAMaskHead's proj.1 is a BatchNorm2d; MaskSPADE's norm
# has no affine parameters
NORM_MODULES = {"head": ("proj.1",), "cbam": (), "eca": (), "spade": ()}
_F = np.float32


def classify(fullname: str, module_is_norm: bool) -> int:
    """The reference's grouping rule (trainer.py:915-924), restated: a name with "bias" in it is not decayed whatever its module; then the
    weights of normalisation modules; everything else -- MaskCBAM's / MaskECA's beta and mtl_log_vars included -- is decayed."""
    if "bias" in fullname:
        return GROUP_BIAS
    if module_is_norm or "logit_scale" in fullname:
        return GROUP_NORM
    return GROUP_DECAY


def reference_group(kind: str, name: str) -> int:
    """Group of parameter `name` (reference name) of a block of `kind`: "cbam" | "eca" | "spade" | "head" | "model" (mtl_log_vars)."""
    module = name.rsplit(".", 1)[0] if "." in name else ""
    return classify(name, module in NORM_MODULES.get(kind, ()))


@dataclass
class OptConfig:
    """kind: "sgd" (torch.optim.SGD, nesterov) | "adamw" (torch.optim.AdamW, betas=(momentum, beta2)).  lr / momentum: one value or one per
    group; weight_decay: group 1's (groups 0 and 2 are not decayed).  check_finite=False: the reference without a GradScaler -- a non-finite
    gradient no longer skips the step."""
    kind: str = "adamw"
    lr: Union[float, Sequence[float]] = 1e-3
    momentum: Union[float, Sequence[float]] = 0.9
    weight_decay: float = 5e-4
    beta2: float = 0.999
    eps: float = 1e-8
    max_norm: float = 10.0
    ema_decay: float = 0.9999
    ema_tau: float = 2000.0
    check_finite: bool = True

    def __post_init__(self):
        if self.kind not in _lib.OPT_KINDS:
            raise ValueError(f"OptConfig: kind {self.kind!r} is none of {sorted(_lib.OPT_KINDS)}")
        if not (self.max_norm > 0 and 0 < self.beta2 < 1 and self.ema_tau > 0 and self.eps >= 0):
            raise ValueError(f"OptConfig: {self}")

    def per_group(self, v):
        return [float(x) for x in v] if isinstance(v, (list, tuple)) else [float(v)] * _lib.OPT_GROUPS


class Segment(NamedTuple):
    name: str                                   # reference name, prefixed by where the tensor sits: "block0.cam_mlp.0.weight", "head1.proj.1.bias"
    param: torch.Tensor                         # fp32, contiguous: updated in place (EMA-only: the buffer that is averaged)
    grad: Optional[torch.Tensor]                # its gradient view into the bucket; None: EMA-only
    group: int = GROUP_DECAY


_HOST_WORDS = _lib.OptHyper.updates.offset // 4  # the words the host owns: lr .. ext_found_inf; the library's counters and outputs follow


def _word(name: str) -> int:
    return getattr(_lib.OptHyper, name).offset // 4


class BucketOptimizer:
    def __init__(self, segments: Sequence[Segment], cfg: OptConfig, device, ema: bool = True, accumulate: bool = False,
                 bucket: Optional[torch.Tensor] = None):
        """segments: see Segment; ema: keep ModelEMA's average of every segment; accumulate: own a flat fp32 `acc` of `bucket`'s size that
        accumulate() adds the bucket to and step() reads and leaves zero -- every grad must then be a view into `bucket`."""
        self.cfg, self.device = cfg, torch.device(device)
        dev = self.device
        self.segments = [Segment(*s) for s in segments]
        if not self.segments:
            raise ValueError("BucketOptimizer: no segments")
        names = [s.name for s in self.segments]
        if len(set(names)) != len(names):
            raise ValueError("BucketOptimizer: segment names repeat")
        for s in self.segments:
            for t in (s.param, s.grad):
                if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != dev.type):
                    raise ValueError(f"BucketOptimizer: {s.name}: fp32 contiguous tensors on {dev} are needed")
            if s.grad is not None and s.grad.numel() != s.param.numel():
                raise ValueError(f"BucketOptimizer: {s.name}: grad has {s.grad.numel()} elements, param {s.param.numel()}")
            if s.grad is None and not ema:
                raise ValueError(f"BucketOptimizer: {s.name}: a segment without a gradient is EMA-only, and ema=False")
        self.adamw = cfg.kind == "adamw"
        trained = [s for s in self.segments if s.grad is not None]
        n_state = sum(s.param.numel() for s in trained)

        def carve(segs, flat):
            out, off = {}, 0
            for s in segs:
                out[s.name] = flat[off:off + s.param.numel()]
                off += s.param.numel()
            return out
        self._state0 = carve(trained, torch.zeros(n_state, dtype=torch.float32, device=dev))
        self._state1 = carve(trained, torch.zeros(n_state, dtype=torch.float32, device=dev)) if self.adamw else {}
        self.ema: Dict[str, torch.Tensor] = {}
        if ema:                                                          # ModelEMA.__init__: a copy of the model
            self.ema = carve(self.segments, torch.zeros(sum(s.param.numel() for s in self.segments), dtype=torch.float32, device=dev))
            for s in self.segments:
                self.ema[s.name].copy_(s.param.reshape(-1))
        # ---- accumulation: the segments' gradients become views into acc at the offsets their views have in the bucket
        self.bucket, self.acc = bucket, None
        grads = {s.name: s.grad for s in trained}
        if accumulate:
            if bucket is None or bucket.dtype != torch.float32 or not bucket.is_contiguous():
                raise ValueError("BucketOptimizer: accumulate=True needs the flat fp32 bucket")
            self.acc = torch.zeros_like(bucket)
            for s in trained:
                off = (s.grad.data_ptr() - bucket.data_ptr()) // 4
                if not (0 <= off and off + s.grad.numel() <= bucket.numel()):
                    raise ValueError(f"BucketOptimizer: {s.name}: its gradient is no view into the bucket")
                grads[s.name] = self.acc[off:off + s.grad.numel()]
        self._grads = grads
        # ---- the device-resident hyper-parameter block (mgaopt_hyper_t)
        self.hyper = torch.zeros(C.sizeof(_lib.OptHyper) // 4, dtype=torch.int32, device=dev)
        self._hyper_f = self.hyper.view(torch.float32)
        self._host = torch.zeros(_HOST_WORDS, dtype=torch.int32)        # the host's copy of the words it owns
        self._host_f = self._host.view(torch.float32)
        self._host_f[_word("inv_scale")] = 1.0
        lr, mom = cfg.per_group(cfg.lr), cfg.per_group(cfg.momentum)
        for j in range(_lib.OPT_GROUPS):
            self._set_group(j, lr[j], mom[j], cfg.weight_decay if j == GROUP_DECAY else 0.0)
        self._upload()
        # ---- the C-ABI tables
        self._cfg = _lib.OptCfg(_lib.OPT_KINDS[cfg.kind], int(cfg.check_finite), int(accumulate), 0, cfg.beta2, cfg.eps, cfg.max_norm,
                                cfg.ema_decay, cfg.ema_tau)
        self._segs = (_lib.OptSegment * len(self.segments))()
        for S, s in zip(self._segs, self.segments):
            fill_opt_segment(S, s.param, self._grads.get(s.name), self._state0.get(s.name), self._state1.get(s.name), self.ema.get(s.name), s.group)
        self.ws = None
        if dev.type == "cuda":
            nbytes = _lib.load().mgaopt_ws_bytes(self._segs, len(self._segs))
            if nbytes == 0:
                _lib.check(_lib.E_SHAPE, "mgaopt_ws_bytes")
            image = torch.zeros(nbytes, dtype=torch.uint8)
            _lib.check(_lib.load().mgaopt_ws_init(self._segs, len(self._segs), image.data_ptr(), nbytes), "mgaopt_ws_init")
            self.ws = image.to(dev)                                      # the tables, uploaded once; partials follow them

    # ---- construction from a plan -------------------------------------------------------------------------------------------------------
    @classmethod
    def for_plan(cls, plan, cfg: OptConfig, ema: bool = True, accumulate: bool = False) -> "BucketOptimizer":
        """Named segments of everything `plan` trains -- a SlicePlan (blocks, heads, mtl_log_vars) or a pyramid plan (its blocks) -- plus, with
        ema, the floating-point running buffers ModelEMA averages too, as EMA-only segments.  Integer buffers (num_batches_tracked) are none."""
        return cls(plan_segments(plan, ema), cfg, plan.device, ema=ema, accumulate=accumulate, bucket=plan.grad_bucket)

    # ---- host writes into the device block (between replays; none of them is captured) -------------------------------------------------
    def _set_group(self, j, lr=None, momentum=None, weight_decay=None):
        if not 0 <= j < _lib.OPT_GROUPS:
            raise ValueError(f"group {j}")
        f = self._host_f
        if lr is not None:
            f[_word("lr") + j] = float(lr)
        if momentum is not None:
            m = float(momentum)
            if not 0.0 < m < 1.0:                                             # SGD too: at 0 torch leaves momentum_buffer alone, the kernel
                raise ValueError(f"momentum {m}")                             # stores buf = g, and the two part when momentum returns
            f[_word("momentum") + j] = m
            f[_word("one_minus_momentum") + j] = 1.0 - m                      # in double, as torch's Python side forms it
            f[_word("ln_momentum") + j] = math.log(m)
        if weight_decay is not None:
            f[_word("weight_decay") + j] = float(weight_decay)

    def _upload(self):
        self.hyper[:_HOST_WORDS].copy_(self._host)

    def set_group(self, j: int, lr: Optional[float] = None, momentum: Optional[float] = None, weight_decay: Optional[float] = None) -> None:
        """Group j's lr / momentum (AdamW: beta1; either in (0, 1)) / weight decay from now on: what warm-up and the scheduler change every
        iteration."""
        self._set_group(j, lr, momentum, weight_decay)
        self._upload()

    def set_scale(self, scale: float) -> None:
        """The GradScaler's current scale: the gradients in the bucket are `scale` times the true ones."""
        self._host_f[_word("inv_scale")] = 1.0 / float(scale)
        self._upload()

    def set_external(self, sumsq: float = 0.0, found_inf: bool = False) -> None:
        """The rest of the model: the squared norm of its unscaled gradients, and whether one of them was non-finite."""
        self._host_f[_word("ext_sumsq")] = float(sumsq)
        self._host[_word("ext_found_inf")] = int(bool(found_inf))
        self._upload()

    # ---- state --------------------------------------------------------------------------------------------------------------------------
    @property
    def momentum_buffers(self) -> Dict[str, torch.Tensor]:
        assert not self.adamw, "an AdamW optimizer keeps exp_avg / exp_avg_sq"
        return self._state0

    @property
    def exp_avg(self) -> Dict[str, torch.Tensor]:
        assert self.adamw, "an SGD optimizer keeps momentum_buffers"
        return self._state0

    @property
    def exp_avg_sq(self) -> Dict[str, torch.Tensor]:
        assert self.adamw, "an SGD optimizer keeps momentum_buffers"
        return self._state1

    @property
    def counters(self) -> torch.Tensor:
        """int32 [updates, t slot 0, t slot 1] in the device block; the count of applied steps is slot updates & 1 (`t`)."""
        return self.hyper[_word("updates"):_word("updates") + 3]

    @property
    def updates(self) -> int:
        return int(self.hyper[_word("updates")])

    @property
    def t(self) -> int:
        c = self.counters.tolist()
        return c[1 + (c[0] & 1)]

    @property
    def grad_norm(self) -> torch.Tensor:
        return self._hyper_f[_word("grad_norm")]

    @property
    def clip_coef(self) -> torch.Tensor:
        return self._hyper_f[_word("clip_coef")]

    @property
    def found_inf(self) -> torch.Tensor:
        return self.hyper[_word("found_inf")]

    def ema_state(self) -> Dict[str, torch.Tensor]:
        """{reference name: the average, in the parameter's shape}"""
        return {s.name: self.ema[s.name].view(s.param.shape) for s in self.segments} if self.ema else {}

    def state_tensors(self) -> List[torch.Tensor]:
        """Everything a step may change, for tests that compare bits: parameters, optimizer state, averages, the block, the accumulator."""
        out = [s.param for s in self.segments] + list(self._state0.values()) + list(self._state1.values()) + list(self.ema.values()) + [self.hyper]
        return out + ([self.acc] if self.acc is not None else [])

    def capture(self, plan, fn=None) -> "torch.cuda.CUDAGraph":
        """``plan.capture(fn)`` with this optimizer's launches in it (default fn: ``plan.step(); self.step()``).  The warm-up run a capture
        needs is a real step -- parameters move, counters and averages advance -- so everything this optimizer may change is put back
        afterwards (the running buffers it averages included)."""
        if fn is None:
            fn = lambda: (plan.step(), self.step())
        saved = [t.clone() for t in self.state_tensors()]
        graph = plan.capture(fn)
        for t, s in zip(self.state_tensors(), saved):
            t.copy_(s)
        return graph

    # ---- the step -----------------------------------------------------------------------------------------------------------------------
    def accumulate(self) -> None:
        """acc += bucket: one launch on the current stream, capturable."""
        if self.acc is None:
            raise RuntimeError("BucketOptimizer: built with accumulate=False")
        if self.device.type != "cuda":
            self.acc += self.bucket
            return
        call("mgaopt_accumulate", self.device, self.acc.data_ptr(), self.bucket.data_ptr(), self.acc.numel())

    def step(self) -> None:
        """Two launches on the current stream, capturable: k_opt_norm, k_opt_step."""
        if self.device.type != "cuda":
            return self._host_step()
        call("mgaopt_step", self.device, self._segs, len(self._segs), C.byref(self._cfg), self.hyper.data_ptr(), self.ws.data_ptr(), self.ws.numel())

    def _host_step(self) -> None:
        """csrc/opt.cuh on CPU tensors: the same operations on fp32 values in the same order, the norm summed per segment."""
        cfg, H, Hf = self.cfg, self.hyper, self._hyper_f
        w = _word
        u = int(H[w("updates")]) + 1
        H[w("updates")] = u
        t_old = int(H[w("t") + ((u & 1) ^ 1)])
        inv_scale = _F(Hf[w("inv_scale")].item())
        total_sq, found = _F(0.0), False
        for s in self.segments:
            g = self._grads.get(s.name)
            if g is not None:
                found = found or not bool(torch.isfinite(g).all())
                total_sq = _F(total_sq + _F(((g.reshape(-1) * float(inv_scale)) ** 2).sum().item()))
        with np.errstate(all="ignore"):
            total = np.sqrt(_F(total_sq + _F(Hf[w("ext_sumsq")].item())))
            c = _F(cfg.max_norm) / _F(total + _F(1e-6))
            coef = _F(1.0) if c > 1.0 else c
        skip = cfg.check_finite and (found or int(H[w("ext_found_inf")]) != 0)
        t = t_old + (0 if skip else 1)
        H[w("t") + (u & 1)] = t
        Hf[w("grad_norm")], Hf[w("clip_coef")], H[w("found_inf")] = float(total), float(coef), int(found)
        omd = _F(_F(1.0 - cfg.ema_decay) + _F(cfg.ema_decay) * np.exp(_F(-_F(u) * _F(1.0 / cfg.ema_tau))))
        d = _F(_F(1.0) - omd)
        for s in self.segments:
            g, p = self._grads.get(s.name), s.param.reshape(-1)
            if g is not None:
                if not skip:
                    lr, mom, wd = (_F(Hf[w(k) + s.group].item()) for k in ("lr", "momentum", "weight_decay"))
                    gg = g.reshape(-1) * float(inv_scale)
                    gg = gg * float(coef)
                    s0 = self._state0[s.name]
                    if not self.adamw:
                        gg = gg + float(wd) * p
                        s0.mul_(float(mom)).add_(gg)
                        gg = gg + float(mom) * s0
                        p.sub_(float(lr) * gg)
                    else:
                        s1 = self._state1[s.name]
                        om, ln_m = _F(Hf[w("one_minus_momentum") + s.group].item()), _F(Hf[w("ln_momentum") + s.group].item())
                        step_size = lr / -np.expm1(_F(_F(t) * ln_m))
                        bc2_sqrt = np.sqrt(-np.expm1(_F(_F(t) * _F(math.log(cfg.beta2)))))
                        p.mul_(float(_F(_F(1.0) - lr * wd)))
                        s0.copy_(s0 + float(om) * (gg - s0) if om < 0.5 else gg - (gg - s0) * float(_F(1.0) - om))
                        s1.mul_(float(_F(cfg.beta2))).add_(float(_F(1.0 - cfg.beta2)) * gg * gg)
                        p.sub_(float(step_size) * (s0 / (s1.sqrt() / float(bc2_sqrt) + float(_F(cfg.eps)))))
                if self.acc is not None:
                    g.zero_()
            if self.ema:
                self.ema[s.name].mul_(float(d)).add_(float(omd) * p)


def plan_segments(plan, ema: bool = True) -> List[Segment]:
    """for_plan's segment list: every parameter tensor the plan reads, under its reference name, classified with the reference's rule."""
    blk = plan.block if isinstance(plan, SlicePlan) else plan
    if not isinstance(blk, _BlockPlan):
        raise TypeError(f"BucketOptimizer.for_plan: {type(plan).__name__} is none of the static plans")
    kind = blk.kind
    names = [CBAM_REFERENCE_NAMES[n] for n in blk.param_names] if kind == "cbam" else blk.param_names
    segs = []
    for l in range(blk.n):
        segs += [Segment(f"block{l}.{n}", p, g, reference_group(kind, n)) for n, p, g in zip(names, blk.params[l], blk.param_grads[l])]
    if isinstance(plan, SlicePlan):
        for l in range(plan.n):
            segs += [Segment(f"head{l}.{n}", p, g, reference_group("head", n)) for n, p, g in zip(HEAD_PARAM_NAMES, plan.head_params[l], plan.head_grads[l])]
        segs.append(Segment("mtl_log_vars", plan.log_vars, plan.g_log_vars, reference_group("model", "mtl_log_vars")))
    if ema:                                                              # the floating-point buffers of the state dict (torch_utils.py:771-774)
        for l, run in enumerate(blk.running):
            if run is not None and run[0] is not None:
                segs += [Segment(f"block{l}.norm.{n}", b, None, GROUP_DECAY) for n, b in zip(("running_mean", "running_var"), run)]
        if isinstance(plan, SlicePlan):
            for l, bufs in enumerate(plan.head_buffers):
                segs += [Segment(f"head{l}.proj.1.{n}", b, None, GROUP_DECAY) for n, b in zip(("running_mean", "running_var"), bufs)]
    return segs
