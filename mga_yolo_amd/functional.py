"""Autograd entry points of the mask-guided CBAM block on MI355X.

``mask_cbam(x, mask, ...)`` replaces the body of the reference's ``MaskCBAM.forward``
(mga_yolo/nn/modules/masked_cbam.py:154-171) for device tensors: forward and backward are each ONE call
into libmgacbam.so (include/mgacbam.h), which enqueues the hand-written gfx950 kernels on the current stream.
``mask_cbam_pyramid`` does the same for several independent pyramid levels (P3/P4/P5) in one call.

Device tensors never take any other path: a missing library raises (``_lib.LibraryMissing``).
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._binding import CBAM, DTYPES as _DTYPES, ECA, HEAD, SPADE, Family, call as _call, raw_stream as _raw_stream
from ._binding import fill_gate, fill_targets, spade_eager_ctx_bytes, head_params as _head_params  # noqa: F401  (tests fill head levels by hand with it)


@dataclass(frozen=True)
class BlockConfig:
    """Non-tensor constructor state of one block (masked_cbam.py:34-50)."""
    hidden: int
    k: int = 7
    use_sigmoid_mask: bool = True
    tiny_thr: float = 1e-4
    eps: float = 1e-6


def stage_switches() -> Tuple[bool, bool]:
    """(MGACBAM_FUSE_FWD, MGACBAM_FOLD_BWD) as the environment has them NOW, both on by default (the eager path asks at import, a plan when it is
    built).  FUSE_FWD: k_chan + k_apply as ONE x-resident launch, k_gate; FOLD_BWD: the transposed conv folded into the k_bwd_reduce1 launch."""
    return bool(int(os.environ.get("MGACBAM_FUSE_FWD", "1"))), bool(int(os.environ.get("MGACBAM_FOLD_BWD", "1")))


_FUSE_FWD, _FOLD_BWD = stage_switches()
_FOLD_BWD = _FUSE_FWD and _FOLD_BWD       # the folded launch needs the zero-filled ctx tail the fused forward sets up
# MGACBAM_CHECK_HANDOFF=1: synchronise after every library call and raise if an in-launch hand-off timed out (debugging switch;
# without it a time-out is still loud -- the tile is poisoned with NaN -- and handoff_report() reads every status word at once)
_CHECK_HANDOFF = bool(int(os.environ.get("MGACBAM_CHECK_HANDOFF", "0")))
_LEAD = ("blk", "cfgs")      # what the eager frame's Function (_BlockFn.forward) takes in front of the levels' tensors: no gradient


class HandoffTimeout(RuntimeError):
    """An in-launch hand-off (k_gate / folded k_bwd_reduce1) timed out: the device was shared with work that took the CUs its
    co-residency assumption needs.  The affected tiles were poisoned with NaN.  Set MGACBAM_FUSE_FWD=0 to run without hand-offs."""


class _CtxPool:
    """Saved-statistics buffers of the eager path, recycled per (device, stream, shape): the hand-off flags at the end of ctx are
    generation counters that are never reset, so a buffer is zero-filled ONCE when it is created and stays consistent over any
    number of calls -- the per-call zero-fill launch (and the allocation) disappear from the unchanged-trainer path."""

    def __init__(self, keep: int = 8):
        self.free, self.all, self.keep = {}, [], keep

    def take(self, key, nbytes: int, sync_off: int, dev):
        lst = self.free.get(key)
        if lst:
            return lst.pop()
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        buf[sync_off:].zero_()
        self.all.append((weakref.ref(buf), key))
        if len(self.all) > 4096:
            self.all = [(r, k) for r, k in self.all if r() is not None]
        return buf

    def give(self, key, buf):
        lst = self.free.setdefault(key, [])
        if len(lst) < self.keep:
            lst.append(buf)

    def clear(self):
        self.free.clear()
        self.all = [(r, k) for r, k in self.all if r() is not None]


_POOL = _CtxPool()


class _Lease:
    """Returns its buffer to the pool when the autograd context that owns it dies (after backward, or with the graph)."""
    __slots__ = ("key", "buf")

    def __init__(self, key, buf):
        self.key, self.buf = key, buf

    def __del__(self):
        try:
            _POOL.give(self.key, self.buf)
        except Exception:
            pass


def status_words(bufs_and_shapes) -> List[int]:
    """The hand-off status word (include/mgacbam.h) of each ctx buffer, given as (buffer, (B,C,H,W,hidden)), after ONE concatenated device
    read -- which waits for the work queued before it, as any read-back does.  Non-zero: a hand-off into that buffer timed out."""
    words = []
    for buf, (B, Cc, H, W, hidden) in bufs_and_shapes:
        off = _lib.ctx_layout(B, Cc, H, W, hidden)["status"]
        words.append(buf[off:off + 4].view(torch.int32))
    return torch.cat(words).cpu().tolist()


def handoff_check(bufs_and_shapes, where, what: Optional[str] = None) -> int:
    """The one status-word check: read the word of every (ctx buffer, (B,C,H,W,hidden)) given (status_words: it synchronises) and raise
    HandoffTimeout if any is set -> the number of buffers checked.  where(the (B,C,H,W) whose word is set) words them in the message;
    what: a call's name, for the per-call form (MGACBAM_CHECK_HANDOFF), which carries no advice."""
    entries = list(bufs_and_shapes)
    bad = [s[:4] for (_, s), w in zip(entries, status_words(entries)) if w != 0]
    if bad:
        advice = ": affected tiles were poisoned with NaN (is the GPU shared with other work?  MGACBAM_FUSE_FWD=0 runs without hand-offs)"
        raise HandoffTimeout(f"in-launch hand-off timed out for {where(bad)}{advice}" if what is None else
                             f"{what}: in-launch hand-off timed out for {where(bad)}")
    return len(entries)


def handoff_report(clear_pool: bool = False):
    """Synchronise and read the hand-off status word of every ctx buffer the eager path has handed out and that is still alive.
    Returns the number of buffers checked; raises HandoffTimeout if any word is set.  Call it where the training loop synchronises
    anyway (end of an epoch / validation)."""
    live = [(r(), k) for r, k in _POOL.all]
    live = [(b, k[2:7]) for b, k in live if b is not None]
    if not live:
        return 0
    try:
        return handoff_check(live, lambda bad: f"shapes {sorted(set(bad))}")
    finally:
        if clear_pool:
            _POOL.clear()


def _check_status(leases, what: str):
    handoff_check([(ls.buf, ls.key[2:7]) for ls in leases], lambda bad: "level (B,C,H,W)=({},{},{},{})".format(*bad[0]), what)


def _aligned(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def _ready(t: torch.Tensor) -> torch.Tensor:
    """Detached, contiguous, 16-byte aligned view/copy of t; the common case (already so) costs two attribute reads."""
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t                                               # (inside autograd.Function.forward: no graph is recorded)
    return _aligned(t.detach())


def _is_nhwc(x: torch.Tensor) -> bool:
    """A level takes the channels-last kernels when x is channels_last-contiguous and NOT also NCHW-contiguous (C == 1 or H = W = 1 are
    both: those, and every other stride pattern, keep the NCHW path)."""
    return x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()


def _ready_nhwc(t: torch.Tensor) -> torch.Tensor:
    """Detached, channels_last-contiguous, 16-byte aligned view/copy of t (one conversion at most)."""
    if t.is_contiguous(memory_format=torch.channels_last) and t.data_ptr() % 16 == 0:
        return t
    return t.detach().clone(memory_format=torch.channels_last)


def _feature_in(x: torch.Tensor, nhwc_ok: bool = True):
    """-> (x as the kernels read it, whether that is channels_last).  The layout decides the kernels, per level (_is_nhwc); nhwc_ok=False
    keeps a level the channels-last kernels do not take on the NCHW path."""
    nhwc = nhwc_ok and _is_nhwc(x)
    return (_ready_nhwc(x) if nhwc else _ready(x)), nhwc


def _param32(t: torch.Tensor) -> torch.Tensor:
    """A parameter as the kernels read it: fp32, detached, contiguous, aligned (MaskECA, the mask head and MaskSPADE cast; MaskCBAM
    refuses anything but fp32, _check_params)."""
    return _ready(t.float())


def _mask_in(mask: Optional[torch.Tensor], B: int, H: int, W: int):
    """-> (the mask as the kernels read it: fp32 (B,1,H,W), detached, aligned; (dtype, shape) it came in), or (None, None)."""
    if mask is None:
        return None, None
    m = mask.unsqueeze(1) if mask.dim() == 3 else mask                        # masked_cbam.py:81-85
    if tuple(m.shape) != (B, 1, H, W):                                        # the reference's expand() raises too
        raise RuntimeError(f"mask shape {tuple(mask.shape)} does not match feature (B,1,H,W)=({B},1,{H},{W})")
    return _ready(m if m.dtype == torch.float32 else m.float()), (mask.dtype, tuple(mask.shape))


def _grad_in(gy: Optional[torch.Tensor], like: torch.Tensor, nhwc: bool) -> torch.Tensor:
    """The incoming gradient of an output in `like`'s element type and layout: zeros for None, a gy of any other layout converted once."""
    if gy is None:
        return torch.zeros_like(like)
    gy = gy.to(like.dtype)
    return _ready_nhwc(gy) if nhwc else _aligned(gy)


def _gmask_out(grads: list, blk: "_Block", kept: Sequence[tuple]) -> None:
    """Give dL/dmask (the gradient of each level's input "mask") back in the mask's own shape / element type.
    This runs AFTER the launch that writes it: a cast enqueued before it would read unwritten memory (that was the case for
    half-precision masks until the AMP test of round 3)."""
    if blk.mask_at is None:
        return
    for l, (_, _, meta, _, _) in enumerate(kept):
        i = len(_LEAD) + l * blk.slots + blk.mask_at
        if grads[i] is not None:
            grads[i] = grads[i].reshape(meta[1]).to(meta[0])


def _check_feature(x: torch.Tensor, what: str) -> None:
    if x.dim() != 4:
        raise AssertionError(what)
    if x.dtype not in _DTYPES:
        raise TypeError(f"unsupported feature dtype {x.dtype}")


def _check_params(x: torch.Tensor, params: Sequence[torch.Tensor], cfg: BlockConfig) -> None:
    Cc, h, k = x.shape[1], cfg.hidden, cfg.k
    want = {"w1": (h, Cc), "b1": (h,), "w2": (Cc, h), "b2": (Cc,), "wsa": (1, 3, k, k), "beta": ()}
    for name, t in zip(want, params):
        if tuple(t.shape) != want[name] or t.dtype != torch.float32 or t.device != x.device:
            raise ValueError(f"parameter {name}: expected fp32 {want[name]} on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")


# ---------------------------------------------------------------------------------------------------------
# The eager frame: n independent levels of ONE block family (_binding.Family) through autograd, one library call each way.  _BlockFn and
# the two table builders under it hold the only level loops; a family adds a _Block: its checks, its inputs, what it saves, what it returns
# ---------------------------------------------------------------------------------------------------------
class _Block:
    """What one family's eager call adds to the frame.  ``inputs`` names a level's tensors in the order they are passed, ``saved`` the ones
    its backward gets back, in the order they are saved; "params" stands for the family's parameters (``family.param_names``), every other
    name for one tensor.  The frame derives every position from the two: the slice of a level, where a gradient goes in the returned
    tuple, whether dL/dmask is wanted.  An input that is none of "x", "mask", "params" is a buffer: its gradient is None."""
    family: Family
    name: str                                   # what the refusals call the function
    device_only = True                          # host tensors are refused by that name (False: by the same-GPU refusal, as ever)
    same_gpu = True                             # the same-GPU refusal (False: the family's own argument check covers the device)
    pooled = False                              # ctx comes from _POOL, keyed by the stream
    inputs: Tuple[str, ...]
    saved: Tuple[str, ...]
    fwd_args = bwd_args = ()                    # what the entry points take after (levels, n)

    def __init__(self):
        expand = lambda declared: tuple(n for d in declared for n in (self.family.param_names if d == "params" else (d,)))
        self.input_names, self.saved_names = expand(self.inputs), expand(self.saved)         # ("params" written out)
        self.slots, self.n_saved = len(self.input_names), len(self.saved_names)
        self.x_at = self.input_names.index("x")
        self.mask_at = self.input_names.index("mask") if "mask" in self.inputs else None

    def level(self, cfg, inp, dev):
        """The family's argument checks, in their order, and the tensors a level's kernels read, from `inp`, the level's inputs in the
        order of ``inputs`` -> (the cfg its fills take, channels_last?, the mask's (dtype, shape) | None, its running buffers | None,
        {x, mask, params and whatever else ``saved`` names})"""
        raise NotImplementedError

    def out(self, x):
        return torch.empty_like(x)              # (preserve_format: channels_last for a channels_last level)

    def ctx_buffer(self, cfg, flags, x, stream, save_gamma):
        """-> (a level's ctx, the _Lease it came with | None)"""
        return torch.empty(self.family.ctx_bytes(x.shape, cfg, flags), dtype=torch.uint8, device=x.device), None

    def grad_in(self, gy, x, nhwc):
        return _grad_in(gy, x, nhwc)

    def pack(self, b: dict) -> list:
        """a level's tensors for save_for_backward, in the order of ``saved_names``"""
        return [t for k in self.saved for t in (b[k] if k == "params" else (b[k],))]

    def unpack(self, run) -> dict:
        """pack's inverse: {name in ``saved``: tensor, "params": list} from a level's run of saved tensors; "mask": None unless saved"""
        it = iter(run)
        return {"mask": None, **{k: [next(it) for _ in self.family.param_names] if k == "params" else next(it) for k in self.saved}}


def _refuse_host(blk: _Block, xs: Sequence[torch.Tensor]) -> None:
    """The frame runs device tensors of ONE GPU; these refusals stand in front of the table builders, which take host tensors too."""
    if blk.device_only and not xs[0].is_cuda:
        raise RuntimeError(f"{blk.name}: device tensors only (host tensors take the module's host path)")
    if blk.same_gpu and not all(x.is_cuda and x.device == xs[0].device for x in xs):
        raise RuntimeError(f"{blk.name}: all features must live on the same GPU")


def _forward_tables(blk: _Block, cfgs, flat, want_grad: bool, stream=None):
    """The table-building half of a forward, on tensors of any device, nothing launched -> (the filled level table, the outputs, the
    tensors to save, per level what the backward needs besides: (cfg, flags, mask meta, running, lease), the tensors to hold until the call
    is enqueued).  want_grad: a backward may come (MaskSPADE keeps gamma for it); stream: the pool's key (``blk.pooled``)."""
    fam, k, n = blk.family, blk.slots, len(cfgs)
    levels = (fam.fwd_level * n)()
    dev = flat[blk.x_at].device
    outs, keep, kept, hold = [], [], [], []
    for l in range(n):
        cfg, nhwc, mmeta, running, b = blk.level(cfgs[l], flat[l * k:(l + 1) * k], dev)
        x = b["x"]
        flags = fam.layout_nhwc if nhwc else 0
        save_gamma = want_grad and b["mask"] is not None
        y = blk.out(x)
        b["ctx"], lease = blk.ctx_buffer(cfg, flags, x, stream, save_gamma)
        nws = fam.ws_bytes(x.shape, cfg, flags)     # MaskCBAM, channels_last: per-chunk pooling partials, consumed inside this call
        ws = torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None
        fam.fill_fwd(levels[l], cfg, flags, y=y, ws=ws, running=running, save_gamma=save_gamma, **b)
        hold.append(ws)
        keep += blk.pack(b)
        outs.append(y)
        kept.append((cfg, flags, mmeta, running, lease))
    return levels, outs, keep, kept, hold


def _backward_tables(blk: _Block, kept, saved, gys, needs):
    """The table-building half of a backward -> (the filled level table, what _BlockFn.backward returns: None per _LEAD, then the gradients
    of the levels' inputs in the order of ``blk.input_names``, level after level; the tensors to hold until the call is enqueued).  kept,
    saved: what _forward_tables gave; needs: ctx.needs_input_grad (dL/dmask is written only where it is wanted)."""
    fam, k, ns = blk.family, blk.slots, blk.n_saved
    levels = (fam.bwd_level * len(kept))()
    grads, hold, lead = [None] * len(_LEAD), [], len(_LEAD)
    for l, (cfg, flags, _, running, lease) in enumerate(kept):
        b = blk.unpack(saved[l * ns:(l + 1) * ns])
        if lease is not None:
            b["ctx"] = lease.buf
        x, mask = b["x"], b["mask"]
        gy = blk.grad_in(gys[l], x, flags)
        gx = torch.empty_like(x)                                   # (channels_last for NHWC levels, as x)
        gmask = torch.empty_like(mask) if mask is not None and needs[lead + l * k + blk.mask_at] else None
        pg = [None if p is None else torch.empty_like(p) for p in b["params"]]
        scratch = torch.empty(fam.scratch_bytes(x.shape, cfg, flags), dtype=torch.uint8, device=x.device)
        fam.fill_bwd(levels[l], cfg, flags, gy=gy, scratch=scratch, gx=gx, gmask=gmask, grads=pg, running=running, **b)
        hold += [gy, scratch]
        own = {"x": (gx,), "mask": (gmask,), "params": pg}
        for name in blk.inputs:
            grads += own.get(name, (None,))                      # (any other input is a buffer)
    return levels, grads, hold


class _BlockFn(torch.autograd.Function):
    """n levels of the family ``blk``; cfgs: per level its config (the mask head: its BatchNorm state); flat: n x ``blk.input_names``."""

    @staticmethod
    def forward(ctx, blk: _Block, cfgs: tuple, *flat):
        n = len(cfgs)
        assert len(flat) == n * blk.slots and 1 <= n <= _lib.MAX_LEVELS
        _lib.load()                                             # a missing library is the first thing a call reports
        dev = flat[blk.x_at].device
        _refuse_host(blk, flat[blk.x_at::blk.slots])
        levels, outs, keep, kept, hold = _forward_tables(blk, cfgs, flat, any(ctx.needs_input_grad), _raw_stream(dev) if blk.pooled else None)
        _call(blk.family.fwd_entry, dev, levels, n, *blk.fwd_args)
        del hold
        if _CHECK_HANDOFF and blk.pooled:
            _check_status([lease for *_, lease in kept], f"{blk.name} forward")
        ctx.save_for_backward(*keep)
        ctx.blk, ctx.kept, ctx.dev = blk, kept, dev
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gys):
        blk, kept = ctx.blk, ctx.kept
        levels, grads, hold = _backward_tables(blk, kept, ctx.saved_tensors, gys, ctx.needs_input_grad)
        _call(blk.family.bwd_entry, ctx.dev, levels, len(kept), *blk.bwd_args)
        del hold
        _gmask_out(grads, blk, kept)
        if _CHECK_HANDOFF and blk.pooled:
            _check_status([lease for *_, lease in kept], f"{blk.name} backward")
        return tuple(grads)


class _CbamBlock(_Block):
    family, name, pooled = CBAM, "mask_cbam", True
    inputs = saved = ("x", "mask", "params")                    # (ctx is not saved: it is the pool's, held by the level's lease)
    fwd_args = (_lib.FWD_ALL | (_lib.FWD_FUSE if _FUSE_FWD else 0),)
    bwd_args = (_lib.BWD_ALL | (_lib.BWD_FOLD if _FOLD_BWD else 0),)

    def level(self, cfg, inp, dev):         # (the AssertionError / TypeError / RuntimeError / ValueError split mirrors the reference, in its order)
        x, mask, *params = inp
        _check_feature(x, "MaskCBAM expects a (B,C,H,W) feature")                 # masked_cbam.py:160
        B, _, H, W = x.shape
        m32, mmeta = _mask_in(mask, B, H, W)
        _check_params(x, params, cfg)
        xc, nhwc = _feature_in(x)
        return cfg, nhwc, mmeta, None, dict(x=xc, mask=m32, params=[_ready(p) for p in params])

    def ctx_buffer(self, cfg, flags, x, stream, save_gamma):
        # FWD_FUSE / BWD_FOLD contract: the hand-off flags at the end of ctx were zero-filled once (by the pool, at creation)
        # (the flags count calls PER TILE, so a buffer is only reused under the tiling it was used with.  The library derives every
        #  flagged tiling from the level alone -- shape, element type, conv size k, knobs; never from the other levels of the call --
        #  and exactly those are in the key.  The merged backward's sweeps, whose channel groups do depend on the call, count per
        #  channel instead: tests/test_gpu_composition.py)
        # (no SAVE_PROJ in flags: the backward makes the W1-projection planes itself where they pay (include/mgacbam.h), and the
        #  forward keeps k_gate; PyramidPlan(use_proj=True) and forward_with_ctx still drive the forward producer, k_chan)
        (B, Cc, H, W), dev = x.shape, x.device
        key = (dev.index, stream, B, Cc, H, W, cfg.hidden, x.dtype, _lib.ENV_EPOCH, cfg.k) + ((flags,) if flags else ())
        lease = _Lease(key, _POOL.take(key, _lib.ctx_bytes(B, Cc, H, W, cfg.hidden), _lib.ctx_layout(B, Cc, H, W, cfg.hidden)["sync"], dev))
        return lease.buf, lease


_CBAM = _CbamBlock()
SLOTS = _CBAM.slots     # tensors per level in the flat argument list: x, mask, w1, b1, w2, b2, wsa, beta


def mask_cbam_pyramid(levels: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], Sequence[torch.Tensor], BlockConfig]]):
    """levels: [(x, mask|None, (w1,b1,w2,b2,wsa,beta), BlockConfig), ...] -> tuple of outputs (one library call)."""
    return _BlockFn.apply(_CBAM, tuple(cfg for *_, cfg in levels), *(t for x, mask, params, _ in levels for t in (x, mask, *params)))


def mask_cbam(x: torch.Tensor, mask: Optional[torch.Tensor], w1, b1, w2, b2, wsa, beta, cfg: BlockConfig) -> torch.Tensor:
    """y = x + softplus(beta) * (SAM(CAM(x, mask), mask) - x) for a device tensor x (B,C,H,W)."""
    return _BlockFn.apply(_CBAM, (cfg,), x, mask, w1, b1, w2, b2, wsa, beta)[0]


# ---------------------------------------------------------------------------------------------------------
# inspection helpers (tests / tooling): run the forward library call and view the saved statistics by name
# ---------------------------------------------------------------------------------------------------------
def forward_with_ctx(x, mask, params, cfg: BlockConfig, save_proj: bool = True):
    """-> (y, {name: tensor view into ctx}) without autograd; names follow mgacbam_ctx_layout_t.  A channels_last x runs the
    channels-last kernels (y comes back channels_last); the ctx views are the same for both layouts."""
    _, nhwc, _, _, b = _CBAM.level(cfg, (x.detach(), None if mask is None else mask.detach(), *(p.detach() for p in params)), x.device)
    B, Cc, H, W = x.shape
    y, flags = torch.empty_like(b["x"]), (_lib.LAYOUT_NHWC if nhwc else 0)
    cbuf = torch.zeros(_lib.ctx_bytes(B, Cc, H, W, cfg.hidden), dtype=torch.uint8, device=x.device)
    ws = torch.empty(_lib.fwd_ws_bytes(B, Cc, H, W, cfg.hidden, flags), dtype=torch.uint8, device=x.device) if flags else None
    lv = (_lib.FwdLevel * 1)()
    CBAM.fill_fwd(lv[0], cfg, flags | (_lib.FWD_SAVE_PROJ if (save_proj and mask is not None) else 0), y=y, ctx=cbuf, ws=ws, **b)
    _call("mgacbam_forward", x.device, lv, 1)
    return y, ctx_views(cbuf, B, Cc, H, W, cfg.hidden)


def ctx_views(cbuf: torch.Tensor, B, Cc, H, W, hidden) -> dict:
    lay = _lib.ctx_layout(B, Cc, H, W, hidden)
    HW = H * W
    shapes = dict(S=(B,), use=(B,), den=(B,), avg=(B, Cc), mx=(B, Cc), mavg=(B, Cc), valid=(B, Cc), amax=(B, Cc),
                  h_avg=(B, hidden), h_mx=(B, hidden), ca=(B, Cc), planes=(B, 3, HW), cidx=(B, HW), sa=(B, HW))
    if hidden <= _lib.PROJ_MAX_HIDDEN:
        shapes["proj"] = (B, hidden, HW)
    shapes["sync"] = (_lib.sync_len(B, Cc, H, W),)          # hand-off state: _lib.sync_regions
    ints = {"valid", "amax", "cidx", "sync"}
    out = {}
    for name, shp in shapes.items():
        n = 1
        for s in shp:
            n *= s
        raw = cbuf[lay[name]: lay[name] + 4 * n]
        out[name] = raw.view(torch.int32 if name in ints else torch.float32).reshape(shp)
    return out


# ---------------------------------------------------------------------------------------------------------
# MaskECA
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class EcaConfig:
    """Non-tensor state of a MaskECA block (masked_eca.py:57-65)."""
    k: int
    use_sigmoid_mask: bool = True
    tiny_thr: float = 1e-4
    eps: float = 1e-6


# the channels-last MaskECA kernels keep 3 floats per channel in LDS (csrc/api_eca.hip: kEcaNhwcMaxC); a wider channels_last feature keeps
# the path it always had: one copy to NCHW and the NCHW kernels
_ECA_NHWC_MAX_C = 4096


class _EcaBlock(_Block):
    """The layout decides the kernels, per level (MaskCBAM's rule, _is_nhwc): a channels_last x runs the channels-last kernels without a
    copy and y / gx come back channels_last."""
    family, name, device_only = ECA, "mask_eca", False
    inputs, saved = ("x", "mask", "params"), ("x", "mask", "ctx", "params")

    def level(self, cfg, inp, dev):
        x, mask, w, beta = inp
        _check_feature(x, "feature must be (B,C,H,W)")                            # masked_eca.py:174
        B, Cc, H, W = x.shape
        m32, mmeta = _mask_in(mask, B, H, W)
        if tuple(w.shape) != (1, 1, cfg.k) or beta.dim() != 0:
            raise ValueError(f"MaskECA parameters: expected conv1d.weight (1,1,{cfg.k}) and scalar beta")
        xc, nhwc = _feature_in(x, Cc <= _ECA_NHWC_MAX_C)
        return cfg, nhwc, mmeta, None, dict(x=xc, mask=m32, params=[_param32(w), _param32(beta)])


_ECA = _EcaBlock()


def mask_eca(x: torch.Tensor, mask: Optional[torch.Tensor], w: torch.Tensor, beta: torch.Tensor, cfg: EcaConfig) -> torch.Tensor:
    """y = x * (1 + softplus(beta) * (sigmoid(conv1d(masked_avg(x, mask))) - 0.5)) for a device tensor (masked_eca.py:167-196).
    A channels_last x with C <= 4096 is taken as it is (no layout copy); y and dL/dx are then channels_last too.  Any other layout, and a
    wider channels_last feature, is copied to NCHW once and runs the NCHW kernels, as before.  The NCHW kernels take C <= 5117 (the
    backward's LDS, csrc/api_eca.hip: kEcaNchwMaxC); a wider feature raises here, at the forward, with the library's message."""
    return _BlockFn.apply(_ECA, (cfg,), x, mask, w, beta)[0]


def mask_eca_pyramid(levels: Sequence[Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor, EcaConfig]]):
    """levels: [(x, mask|None, conv1d.weight, beta, EcaConfig), ...] -> tuple of outputs (one library call each way).  Levels may mix
    layouts: each channels_last feature runs the channels-last kernels, the others the NCHW ones."""
    return _BlockFn.apply(_ECA, tuple(cfg for *_, cfg in levels), *(t for *tensors, _ in levels for t in tensors))


def resize_nearest(src: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """F.interpolate(src, (out_h,out_w), mode='nearest') for fp32 (...,H,W) device tensors: the integer index path of
    mga_yolo/nn/losses/segmentation.py:103-110, bit-exact (pure gather)."""
    if not src.is_cuda or src.dtype != torch.float32 or src.dim() < 2:
        raise TypeError("resize_nearest expects an fp32 device tensor (..., H, W)")
    _lib.load()
    s = _aligned(src)
    in_h, in_w = s.shape[-2:]
    planes = s.numel() // (in_h * in_w)
    dst = torch.empty(*s.shape[:-2], out_h, out_w, dtype=torch.float32, device=s.device)
    _call("mgacbam_resize_nearest", s.device, s.data_ptr(), dst.data_ptr(), planes, in_h, in_w, out_h, out_w)
    return dst


# ---------------------------------------------------------------------------------------------------------
# The multi-scale segmentation targets (include/mgatargets.h): what the reference's dataset builds per sample on its dataloader workers
# (mga_yolo/data/dataset.py:94-103) and collate_fn stacks into masks_multi, here from the batch's masks where they lie
# ---------------------------------------------------------------------------------------------------------
TARGET_CHAIN = (8, 16, 32)      # the model's strides: every prefix of it reads the source once (k_tgt_pool)


def target_pyramid_check(strides, method: str, bridge: bool) -> Tuple[int, ...]:
    """The argument rules of a target pyramid, the library's own (include/mgatargets.h), raised as ValueError on either device: 1..4
    strides, powers of two in 2..64, strictly ascending; method 'avgpool' | 'maxpool'; the closing with 'maxpool' only."""
    strides = tuple(int(s) for s in strides)
    if not 1 <= len(strides) <= _lib.TGT_MAX_LEVELS:
        raise ValueError(f"mask_pyramid: {len(strides)} strides (1 .. {_lib.TGT_MAX_LEVELS})")
    for i, s in enumerate(strides):
        if s < 2 or s > 64 or s & (s - 1):
            raise ValueError(f"mask_pyramid: stride {s} is no power of two in 2 .. 64")
        if i and s <= strides[i - 1]:
            raise ValueError(f"mask_pyramid: strides {strides} are not strictly ascending")
    if method not in _lib.TGT_METHODS:
        raise ValueError(f"mask_pyramid: method {method!r} is none of {sorted(_lib.TGT_METHODS)} ('area' and 'nearest' through cv2, 'pyrdown' "
                         "and the skeleton path of the reference are not built)")
    if bridge and method != "maxpool":
        raise ValueError("mask_pyramid: bridge=True closes binary levels: it goes with method='maxpool' only")
    return strides


def target_pyramid_shapes(B: int, H: int, W: int, strides) -> List[Tuple[int, int, int, int]]:
    return [(B, 1, -(-H // s), -(-W // s)) for s in strides]


class TargetPyramidCall:
    """One filled mgatgt_desc_t with the scratch it needs: `src` (B,H,W) -> `dsts`, launched by run() on the current stream (one launch,
    two with the closing).  The static plans keep one (slice.SlicePlan); mask_pyramid builds one per call."""

    def __init__(self, src: torch.Tensor, dsts: Sequence[torch.Tensor], strides, method: str, bridge: bool):
        self.src, self.dsts = src, list(dsts)                  # kept alive: the descriptor holds their addresses
        self.launches = 2 if bridge else 1
        self.desc = _lib.TargetsDesc()
        a = (src, self.dsts, strides, _lib.TGT_METHODS[method], _lib.TGT_CLOSE3 if bridge else 0)
        fill_targets(self.desc, *a)
        self.scratch = None
        if bridge:
            self.scratch = torch.empty(_lib.targets_scratch_bytes(self.desc), dtype=torch.uint8, device=src.device)
            fill_targets(self.desc, *a, scratch=self.scratch)

    def run(self) -> None:
        _call("mgatgt_forward", self.src.device, C.byref(self.desc))


def _mask_pyramid_host(m: torch.Tensor, strides, method: str, bridge: bool) -> List[torch.Tensor]:
    """The torch composition (any device): binarise, zero-pad, count per block.  The counts are integers, so this is the reference's
    numpy (a float32 mean of 0/1 over a padded block; a block max) bit for bit."""
    B, H, W = m.shape
    fg = (m > 0).to(torch.int32)
    out = []
    for s in strides:
        Hs, Ws = -(-H // s), -(-W // s)
        cnt = torch.nn.functional.pad(fg, (0, Ws * s - W, 0, Hs * s - H)).view(B, Hs, s, Ws, s).sum(dim=(2, 4))
        lvl = (cnt > 0).to(torch.float32) if method == "maxpool" else cnt.to(torch.float32) / float(s * s)
        lvl = lvl.unsqueeze(1)
        if bridge:                                             # 3x3 dilation, then 3x3 erosion; max_pool2d pads with -inf: outside is ignored
            mp = torch.nn.functional.max_pool2d
            lvl = -mp(-mp(lvl, 3, 1, 1), 3, 1, 1)
        out.append(lvl)
    return out


def mask_pyramid(mask: torch.Tensor, strides=TARGET_CHAIN, method: str = "avgpool", bridge: bool = False,
                 out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """The segmentation targets of a batch -- what ``masks_multi`` is after the reference's collate_fn: per stride one (B,1,ceil(H/s),ceil(W/s))
    fp32 tensor -- from its full-resolution masks ``mask``, (B,H,W) or (B,1,H,W), uint8 (or bool) or fp32.  A pixel is foreground iff its value > 0
    (dataset.py:89 binarises before the call; unlike MaskUtils, uint8 values other than 0 / 1 are binarised too); the mask is zero-padded on
    the bottom and right to a multiple of each stride.
    method: 'avgpool' -- the foreground share of every s x s block, MaskUtils.downsample_mask_prob(method='avgpool'): the exact block-mean
    form of the 'area' targets an MGA_PROB_MODE run trains on; 'maxpool' -- 1 where the block holds a foreground pixel,
    MaskUtils.downsample_mask with MGA_MASK_METHOD=maxpool.  bridge: with 'maxpool', a 3x3 closing of every level (MGA_MASK_BRIDGE).
    Both methods are integer counts: the result equals the reference's bit for bit.
    Device tensors take ONE launch for all levels (two with bridge): include/mgatargets.h; ``out`` = the tensors to write (static buffers),
    returned as they are.  CPU tensors take a torch composition."""
    strides = target_pyramid_check(strides, method, bridge)
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)                 # the same bytes: True is 1
    if mask.dim() != 3 or mask.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"mask_pyramid expects a uint8 or fp32 (B,H,W) or (B,1,H,W) tensor, got {mask.dtype} {tuple(mask.shape)}")
    B, H, W = mask.shape
    shapes = target_pyramid_shapes(B, H, W, strides)
    if out is not None:
        out = list(out)
        if len(out) != len(shapes):
            raise ValueError(f"mask_pyramid: {len(out)} out tensors for {len(shapes)} strides")
        for o, shp in zip(out, shapes):
            if tuple(o.shape) != shp or o.dtype != torch.float32 or o.device != mask.device or not o.is_contiguous():
                raise ValueError(f"mask_pyramid: out tensor {tuple(o.shape)} {o.dtype} on {o.device}: expected contiguous fp32 {shp} on {mask.device}")
    if not mask.is_cuda:
        res = _mask_pyramid_host(mask, strides, method, bridge)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return out
    _lib.load()
    src = mask.detach().contiguous()              # no copy for alignment's sake: the kernel takes an unaligned base through its element loads
    if out is None:
        out = [torch.empty(shp, dtype=torch.float32, device=src.device) for shp in shapes]
    TargetPyramidCall(src, out, strides, method, bridge).run()
    return out


# ---------------------------------------------------------------------------------------------------------
# ProbMaskGater: gumbel / hard_st sampling as one launch; the uniforms come from the caller
# ---------------------------------------------------------------------------------------------------------
class _GaterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, u1, u2, tau: float, p_min: float, threshold: float, hard: bool):
        _lib.load()
        pc, a, b = (_ready(t) for t in (p, u1, u2))
        if pc.dtype != torch.float32 or a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != pc.shape or b.shape != pc.shape:
            raise RuntimeError("prob_mask_gate: p, u1, u2 must be fp32 tensors of one shape")
        out, msoft = torch.empty_like(pc), torch.empty_like(pc)
        cfg = _lib.PmgCfg(float(tau), float(p_min), float(threshold), int(bool(hard)))
        _call("mgapmg_forward", pc.device, pc.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), msoft.data_ptr(), pc.numel(), C.byref(cfg))
        ctx.save_for_backward(pc, msoft)
        ctx.cfg = (float(tau), float(p_min), float(threshold), int(bool(hard)))
        return out

    @staticmethod
    def backward(ctx, gout):
        pc, msoft = ctx.saved_tensors
        g = _ready(gout.to(torch.float32))
        gp = torch.empty_like(pc)
        cfg = _lib.PmgCfg(*ctx.cfg)
        _call("mgapmg_backward", pc.device, pc.data_ptr(), msoft.data_ptr(), g.data_ptr(), gp.data_ptr(), pc.numel(), C.byref(cfg))
        return gp, None, None, None, None, None, None


def prob_mask_gate(p: torch.Tensor, u1: torch.Tensor, u2: torch.Tensor, tau: float = 1.0, p_min: float = 0.0, threshold: float = 0.5,
                   hard: bool = False) -> torch.Tensor:
    """Gumbel-sigmoid gate of ProbMaskGater for device tensors: max(clamp(p,0,1), p_min) -> sigmoid((logit + logistic(u1,u2)) / tau),
    thresholded with a straight-through gradient when ``hard``.  u1, u2: uniform draws, as torch.rand gives them."""
    return _GaterFn.apply(p, u1, u2, tau, p_min, threshold, hard)


# ---------------------------------------------------------------------------------------------------------
# ProbMaskGater on a pyramid (include/mgagate.h): every level in one launch each way, the uniforms drawn IN the kernel from a Philox4x32-10
# stream keyed by a device-resident (seed, step) -- nothing is drawn by torch, so the call can sit inside a captured graph
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GateConfig:
    """One level's ProbMaskGater settings (probmaskgater.py:8-30).  mode: 'gumbel' | 'hard_st' | 'bernoulli_detach' | 'deterministic';
    a gate that is not ``training`` returns the clamped input whatever its mode, as the module does in eval.  stream_id: the level's word in
    the Philox counter; None = the level's position in the call."""
    mode: str = "gumbel"
    tau: float = 1.0
    p_min: float = 0.0
    threshold: float = 0.5
    training: bool = True
    stream_id: Optional[int] = None

    def __post_init__(self):
        if self.mode not in _lib.GATE_MODES:
            raise ValueError(f"GateConfig: mode {self.mode!r} is none of {sorted(_lib.GATE_MODES)}")
        if not self.tau > 0:
            raise ValueError("GateConfig: tau must be > 0")

    def code(self) -> int:
        """mgagate_level_t.mode"""
        return _lib.GATE_MODES[self.mode] if self.training else _lib.GATE_DETERMINISTIC

    def stream(self, level: int) -> int:
        return level if self.stream_id is None else int(self.stream_id)


def gate_state(seed: int = 0, step: int = 0, device="cuda") -> torch.Tensor:
    """The noise state of prob_mask_gate_pyramid: int64 {seed, step, arrivals = 0, 0} on the device.  A noisy forward leaves step + 1."""
    return torch.tensor([int(seed), int(step), 0, 0], dtype=torch.int64, device=device)


def _check_gate_state(state: torch.Tensor, dev: torch.device) -> None:
    if not (isinstance(state, torch.Tensor) and state.dtype == torch.int64 and state.numel() == 4 and state.is_contiguous() and state.device == dev):
        raise RuntimeError("prob_mask_gate_pyramid: state must be a contiguous int64 tensor of 4 elements on the masks' device (gate_state())")


class _GatePyramidFn(torch.autograd.Function):
    """n levels; inputs after (cfgs, state): the n fp32 masks."""

    @staticmethod
    def forward(ctx, cfgs, state, *masks):
        _lib.load()
        n = len(masks)
        ps = [_ready(m) for m in masks]
        dev = ps[0].device
        _check_gate_state(state, dev)
        outs = [torch.empty_like(p) for p in ps]
        soft = [c.code() in (_lib.GATE_GUMBEL, _lib.GATE_HARD_ST) for c in cfgs]
        msoft = [torch.empty_like(p) if s else None for p, s in zip(ps, soft)]
        levels = (_lib.GateLevel * n)()
        for l, (p, c) in enumerate(zip(ps, cfgs)):
            fill_gate(levels[l], p, outs[l], msoft[l], None, None, c.code(), c.stream(l), c.tau, c.p_min, c.threshold)
        _call("mgagate_forward", dev, levels, n, state.data_ptr())
        ctx.cfgs = cfgs
        ctx.save_for_backward(*ps, *(m for m in msoft if m is not None))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        cfgs, n = ctx.cfgs, len(ctx.cfgs)
        ps, rest = ctx.saved_tensors[:n], list(ctx.saved_tensors[n:])
        levels = (_lib.GateLevel * n)()
        gps = []
        for l, (p, c) in enumerate(zip(ps, cfgs)):
            ms = rest.pop(0) if c.code() in (_lib.GATE_GUMBEL, _lib.GATE_HARD_ST) else None
            g = torch.zeros_like(p) if gouts[l] is None else _ready(gouts[l].to(torch.float32))
            gps.append(torch.empty_like(p))
            fill_gate(levels[l], p, None, ms, g, gps[l], c.code(), c.stream(l), c.tau, c.p_min, c.threshold)
        _call("mgagate_backward", ps[0].device, levels, n)
        return (None, None, *gps)


def prob_mask_gate_pyramid(masks: Sequence[torch.Tensor], state: torch.Tensor, cfgs: Sequence[GateConfig]) -> tuple:
    """ProbMaskGater on every level of a pyramid, one launch forward and one backward, for device tensors.  masks: per level (B,1,H,W) or
    (B,H,W) of any float dtype (they enter as ``.float()``, as the module takes them); state: ``gate_state(seed, step)``, advanced in
    place by a forward that draws noise; cfgs: one GateConfig per level.  -> the gated masks, fp32 (B,1,H,W).
    The noise is this library's own Philox stream (include/mgagate.h): statistically, not bitwise, what the ProbMaskGater module draws."""
    if len(masks) != len(cfgs) or not 1 <= len(masks) <= _lib.MAX_LEVELS:
        raise RuntimeError(f"prob_mask_gate_pyramid: {len(masks)} masks, {len(cfgs)} configs (1..{_lib.MAX_LEVELS} of each)")
    ms = []
    for m in masks:
        if not m.is_cuda or not m.is_floating_point():
            raise TypeError("prob_mask_gate_pyramid expects floating-point device tensors")
        m = m.unsqueeze(1) if m.dim() == 3 else m
        ms.append(m.float())
    return _GatePyramidFn.apply(tuple(cfgs), state, *ms)


# ---------------------------------------------------------------------------------------------------------
# MGAMaskHead: Conv1x1 -> BatchNorm2d -> SiLU -> Conv3x3 as 3 launches forward, 5 backward (csrc/head.cuh); a channels_last
# feature takes the NHWC forms of the GEMM kernels (csrc/head_nhwc.cuh) without a copy, and its gx comes back channels_last
# ---------------------------------------------------------------------------------------------------------
class _HeadBlock(_Block):
    """A level's "cfg" is its BatchNorm state (running_mean, running_var, num_batches_tracked | None, eps, momentum, training): buffers
    updated in place.  running_mean / running_var are saved as tensors although the backward's table gets them with the state: autograd
    then refuses a backward after an in-place change of either."""
    family, name, same_gpu = HEAD, "mask_head", False
    inputs, saved = ("x", "params"), ("x", "ctx", "params", "running_mean", "running_var")

    def level(self, state, inp, dev):
        x, w1, gamma, beta, wh, bh = inp
        rmean, rvar, nbt, eps, momentum, training = state
        if x.dim() != 4 or x.dtype not in _DTYPES or x.device != dev:
            raise RuntimeError("mask_head: x must be a (B,C,H,W) fp32 / fp16 / bf16 tensor on one GPU")
        B, Cc, H, W = x.shape
        hid = w1.shape[0]
        if tuple(w1.shape[:2]) != (hid, Cc) or tuple(wh.shape) != (1, hid, 3, 3) or bh.numel() != 1 or gamma.numel() != hid:
            raise ValueError(f"mask_head: parameter shapes do not match C={Cc}, hidden={hid} (out_channels must be 1)")
        if training and B * H * W == 1:                     # torch.nn.functional.batch_norm refuses this too (no variance from one value)
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        xc, nhwc = _feature_in(x)                           # the layout decides the GEMM kernels, per level (MaskCBAM's rule)
        pc = [_param32(t) for t in (w1, gamma, beta, wh, bh)]     # (dL/dw1 comes back in w1's shape: _param32 keeps it)
        for t in (rmean, rvar):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError("mask_head: running statistics must be contiguous fp32 tensors on the feature's device")
        return ((hid, float(eps), float(momentum), bool(training)), nhwc, None, (rmean, rvar, nbt),
                dict(x=xc, mask=None, params=pc, running_mean=rmean, running_var=rvar))

    def out(self, x):
        B, _, H, W = x.shape
        return torch.empty(B, 1, H, W, dtype=x.dtype, device=x.device)

    def grad_in(self, gl, x, nhwc):
        B, _, H, W = x.shape
        return torch.zeros(B, 1, H, W, dtype=x.dtype, device=x.device) if gl is None else _aligned(gl.to(x.dtype))


_HEAD = _HeadBlock()


def mask_head(x: torch.Tensor, w1, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, wh, bh,
              eps: float = 1e-5, momentum: float = 0.1, training: bool = True) -> torch.Tensor:
    """Mask logits (B,1,H,W) = Conv3x3(SiLU(BatchNorm2d(Conv1x1(x)))) for a device tensor x; in training the running statistics
    (and num_batches_tracked) are updated in place exactly as torch's BatchNorm2d does (mga_yolo/nn/modules/segmentation.py:56-110)."""
    return _BlockFn.apply(_HEAD, ((running_mean, running_var, num_batches_tracked, eps, momentum, training),), x, w1, bn_weight, bn_bias, wh, bh)[0]


def mask_head_pyramid(levels):
    """levels: [(x, w1, bn_weight, bn_bias, running_mean, running_var, num_batches_tracked, wh, bh, eps, momentum, training), ...]
    -> tuple of logits; ONE library call each way for all levels (the three heads read different features: they are independent).
    Levels may mix layouts: each channels_last feature runs the NHWC kernels, the others the NCHW ones."""
    state, flat = [], []
    for x, w1, g_, b_, rm, rv, nbt, wh, bh, eps, mom, tr in levels:
        state.append((rm, rv, nbt, eps, mom, tr))
        flat += [x, w1, g_, b_, wh, bh]
    return _BlockFn.apply(_HEAD, tuple(state), *flat)


# ---------------------------------------------------------------------------------------------------------
# MaskSPADE (mga_yolo/nn/modules/masked_spade.py)
# ---------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SpadeConfig:
    """Non-tensor state of a MaskSPADE call: the constructor's fields (masked_spade.py:30-37) and the norm's mode."""
    hidden: int = 64
    mask_channels: int = 1
    norm_type: str = "in"
    use_sigmoid_mask: bool = True
    eps: float = 1e-6
    momentum: float = 0.1
    training: bool = True

    @property
    def bn(self) -> bool:
        return self.norm_type.lower() == "bn"


SPADE_MAX_C, SPADE_MAX_HIDDEN = 1024, 64
_spade_warned = set()


def spade_kernel_reason(x: torch.Tensor, mask: Optional[torch.Tensor], cfg: SpadeConfig) -> Optional[str]:
    """None when the HIP kernels take this call; otherwise why the block's torch composition runs instead (documented limits, not errors)."""
    Cc = x.shape[1]
    if x.dtype not in _DTYPES:
        return f"feature dtype {x.dtype}"
    if mask is not None and (mask.dim() == 4 and mask.shape[1] != 1 or cfg.mask_channels > 1):
        return "mask_channels > 1"
    if cfg.hidden % 16 or cfg.hidden > SPADE_MAX_HIDDEN:
        return f"hidden={cfg.hidden} (kernels: a multiple of 16, at most {SPADE_MAX_HIDDEN})"
    if Cc % 16 or Cc > SPADE_MAX_C:
        return f"C={Cc} (kernels: a multiple of 16, at most {SPADE_MAX_C})"
    if x.numel() >= 2 ** 31:
        return "feature of 2^31 elements or more"
    return None


def spade_check_norm(x: torch.Tensor, cfg: SpadeConfig) -> None:
    """The inputs torch's norms refuse (torch.nn.functional: _verify_spatial_size / _verify_batch_size), refused the same way."""
    B, Cc, H, W = x.shape
    if not cfg.bn and H * W == 1:
        raise ValueError(f"Expected more than 1 spatial element when training, got input size {x.size()}")
    if cfg.bn and cfg.training and B * H * W == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.size()}")


def spade_compose(x, mask, params, cfg: SpadeConfig, running=None) -> torch.Tensor:
    """The block as torch operators, on whatever device x lives (masked_spade.py:113-139): host tensors, and the device shapes outside the
    kernels' limits (spade_kernel_reason)."""
    import torch.nn.functional as F
    w0, b0, wg, bg, wb, bb = params
    if cfg.bn:
        rm, rv, nbt = running
        if cfg.training and nbt is not None:
            nbt.add_(1)
        x_hat = F.batch_norm(x, rm, rv, None, None, cfg.training, cfg.momentum, cfg.eps)
    else:
        x_hat = F.instance_norm(x, None, None, None, None, True, 0.1, cfg.eps)
    if mask is None:
        return x_hat
    m = mask.unsqueeze(1) if mask.dim() == 3 else mask
    H, W = x.shape[-2:]
    if tuple(m.shape[-2:]) != (H, W):
        m = F.interpolate(m, size=(H, W), mode="bilinear", align_corners=False)
    if cfg.use_sigmoid_mask:
        m = m.sigmoid()
    h = F.relu(F.conv2d(m.to(wg.dtype), w0, b0, padding=1))
    gamma = F.conv2d(h, wg, bg, padding=1).to(x.dtype)
    beta = F.conv2d(h, wb, bb, padding=1).to(x.dtype)
    return gamma * x_hat + beta


class _SpadeBlock(_Block):
    """Forward: statistics, weight pack and ONE fused launch (MFMA convs + FiLM); backward: plain launches (csrc/spade.cuh).  The layout
    decides the kernels, per level (_is_nhwc): a channels_last x runs the channels-last kernels (csrc/spade_nhwc.cuh) without a copy, y and
    gx come back channels_last, and the results are the NCHW kernels' bit for bit.  A level without a mask reads no parameter: None each."""
    family, name, device_only = SPADE, "mask_spade", False
    inputs = ("x", "mask", "params", "running_mean", "running_var", "num_batches_tracked")
    saved = ("x", "mask", "ctx", "params")

    def level(self, cfg, inp, dev):
        x, mask, *params, rm, rv, nbt = inp
        B, _, H, W = x.shape
        xc, nhwc = _feature_in(x)
        m32, mmeta = _mask_in(mask, B, H, W)
        ps = [None] * len(params) if mask is None else [_param32(t) for t in params]
        return cfg, nhwc, mmeta, (rm, rv, nbt), dict(x=xc, mask=m32, params=ps)

    def ctx_buffer(self, cfg, flags, x, stream, save_gamma):
        return torch.empty(spade_eager_ctx_bytes(x.shape, cfg, x.element_size() if save_gamma else 0), dtype=torch.uint8, device=x.device), None


_SPADE = _SpadeBlock()


def _spade_apply(cfgs, flat):
    """The levels the kernels take, through autograd.  With gradients off (torch.no_grad) the inputs go in detached: autograd reports a
    parameter that requires grad as needing one whatever the grad mode, and the forward would keep gamma for a backward that cannot come."""
    if not torch.is_grad_enabled():
        flat = [t.detach() if isinstance(t, torch.Tensor) else t for t in flat]
    return _BlockFn.apply(_SPADE, tuple(cfgs), *flat)


def _spade_prepare(x, mask, params, cfg: SpadeConfig, running):
    """Checks shared by the single and the pyramid call; returns the flat slots of a kernel level, or None when the torch composition takes it."""
    if x.dim() != 4:
        raise AssertionError("feature must be (B,C,H,W)")                        # masked_spade.py:119
    spade_check_norm(x, cfg)
    why = spade_kernel_reason(x, mask, cfg)
    if why is not None:
        if why not in _spade_warned:
            _spade_warned.add(why)
            import warnings
            warnings.warn(f"MaskSPADE: {why}: this call runs the block's torch composition on the device, not the HIP kernels")
        return None
    B, Cc, H, W = x.shape
    if mask is not None:
        m = mask.unsqueeze(1) if mask.dim() == 3 else mask
        if m.dim() != 4 or m.shape[0] != B:
            raise RuntimeError(f"mask shape {tuple(mask.shape)} does not match feature batch {B}")
        if tuple(m.shape[-2:]) != (H, W):                                        # resampled on the device, differentiably, then the kernels
            mask = torch.nn.functional.interpolate(m.float(), size=(H, W), mode="bilinear", align_corners=False)
        want = {"shared.0.weight": (cfg.hidden, 1, 3, 3), "shared.0.bias": (cfg.hidden,), "conv_gamma.weight": (Cc, cfg.hidden, 3, 3),
                "conv_gamma.bias": (Cc,), "conv_beta.weight": (Cc, cfg.hidden, 3, 3), "conv_beta.bias": (Cc,)}
        for (name, shape), t in zip(want.items(), params):
            if tuple(t.shape) != shape or t.device != x.device:
                raise ValueError(f"MaskSPADE parameter {name}: expected {shape} on {x.device}, got {tuple(t.shape)} on {t.device}")
    rm, rv, nbt = running if running is not None else (None, None, None)
    if cfg.bn:
        if rm is None or rv is None or rm.dtype != torch.float32 or rv.dtype != torch.float32 or not rm.is_contiguous() or not rv.is_contiguous():
            raise ValueError("MaskSPADE with norm_type='bn' needs contiguous fp32 running_mean / running_var")
    if not x.is_contiguous() and not _is_nhwc(x):
        x = x.contiguous()                                                       # neither NCHW nor channels_last: one copy to NCHW
    return [x, mask] + list(params) + [rm, rv, nbt]


def mask_spade(x: torch.Tensor, mask: Optional[torch.Tensor], params: Sequence[torch.Tensor], cfg: SpadeConfig, running=None) -> torch.Tensor:
    """y = gamma(mask) * norm(x) + beta(mask) for a device tensor.  params = (shared.0.weight, shared.0.bias, conv_gamma.weight,
    conv_gamma.bias, conv_beta.weight, conv_beta.bias); running = (running_mean, running_var, num_batches_tracked) for norm_type 'bn'
    (updated in place by a training call).  Gradients reach x, the mask and the six parameters."""
    return mask_spade_pyramid([(x, mask, params, cfg, running)])[0]


def mask_spade_pyramid(levels):
    """levels: [(x, mask|None, params, SpadeConfig[, running]), ...] -> tuple of outputs.  The levels the kernels take share one library
    call each way; a level outside their limits runs the torch composition."""
    outs: List[Optional[torch.Tensor]] = [None] * len(levels)
    cfgs, flat, idx = [], [], []
    for i, lv in enumerate(levels):
        x, mask, params, cfg = lv[:4]
        running = lv[4] if len(lv) > 4 else None
        f = _spade_prepare(x, mask, params, cfg, running)
        if f is None:
            outs[i] = spade_compose(x, mask, params, cfg, running)
        else:
            cfgs.append(cfg); flat += f; idx.append(i)
    if cfgs:
        for i, y in zip(idx, _spade_apply(cfgs, flat)):
            outs[i] = y
    return tuple(outs)
