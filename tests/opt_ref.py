"""What tests/test_opt_host.py and tests/test_gpu_opt.py share.  Not a test.

TorchTail is the reference's tail after a backward written with torch's own pieces: clip_grad_norm_(max_norm), torch.optim.SGD(nesterov=True) /
torch.optim.AdamW in the three parameter groups of build_optimizer, and ModelEMA.update restated (U/utils/torch_utils.py:759-775), in any
dtype on any device.  bar_check is the rule every comparison uses: the oracle is the fp64 run on the host, and a result may differ from it by
at most max(1e-6 max|oracle|, 4 x the error of torch's own fp32 run against that oracle)."""
import json
import math
import os

import numpy as np
import torch

from conftest import GOLDEN

GOLDEN_KINDS = {"sgd": "SGD", "adamw": "AdamW"}
LENGTHS = (1, 2, 147, 1023, 1024, 1025, 4099)             # one bucket, in this order (tests/test_gpu_opt.py runs the same on the device)
GROUPS = (1, 0, 2, 1, 0, 1, 1)
EMA_ONLY = 65
K = 4
EXT_SUMSQ = (200.0, 0.0, 200.0, 0.0)                      # |g| is about 0.05 sqrt(7321) = 4.3: with 200 more the norm is 14.8 > 10, without it < 10
SCHEDULE = dict(sgd=[dict(lr=[0.1, 0.002, 0.002], momentum=[0.8] * 3), dict(lr=[0.08, 0.004, 0.004], momentum=[0.83] * 3),
                     dict(lr=[0.05, 0.007, 0.007], momentum=[0.88] * 3), dict(lr=[0.01, 0.01, 0.01], momentum=[0.937] * 3)],
                adamw=[dict(lr=[0.0, 0.0005, 0.0005], momentum=[0.8] * 3), dict(lr=[0.0007, 0.001, 0.001], momentum=[0.83] * 3),
                       dict(lr=[0.0014, 0.0015, 0.0015], momentum=[0.88] * 3), dict(lr=[0.002, 0.002, 0.002], momentum=[0.9] * 3)])


class TorchTail:
    def __init__(self, kind, params, groups, decay, dtype, device, buffers=None, ema_decay=0.9999, ema_tau=2000.0, max_norm=10.0, beta2=0.999, eps=1e-8):
        """params / buffers: {name: initial tensor} (cloned here); groups: {name: 0 biases | 1 decayed | 2 norm weights}"""
        self.kind, self.max_norm, self.ema_decay, self.ema_tau, self.dtype, self.device = kind, max_norm, ema_decay, ema_tau, dtype, device
        self.params = {n: torch.nn.Parameter(p.detach().to(device, dtype).clone()) for n, p in params.items()}
        self.buffers = {n: b.detach().to(device, dtype).clone() for n, b in (buffers or {}).items()}
        g = [[self.params[n] for n in params if groups[n] == j] for j in range(3)]
        for j in range(3):                                             # an empty group keeps the groups' order; torch refuses an empty list
            if not g[j]:
                g[j] = [torch.nn.Parameter(torch.zeros(1, dtype=dtype, device=device))]
        if kind == "sgd":                                              # trainer.py:933, 940, 941
            self.opt = torch.optim.SGD(g[0], lr=0.01, momentum=0.9, nesterov=True)
        else:                                                          # trainer.py:929
            self.opt = torch.optim.AdamW(g[0], lr=0.01, betas=(0.9, beta2), eps=eps, weight_decay=0.0)
        self.opt.add_param_group({"params": g[1], "weight_decay": decay})
        self.opt.add_param_group({"params": g[2], "weight_decay": 0.0})
        self.ext = torch.nn.Parameter(torch.zeros(1, dtype=dtype, device=device))      # the rest of the model: in the clip, in no optimizer
        self.ema = {n: p.detach().clone() for n, p in {**self.params, **self.buffers}.items()}
        self.updates = 0

    def step(self, grads, lr, momentum, ext_sumsq=0.0, buffers=None):
        """grads: {name: tensor}; lr / momentum: per group; buffers: the EMA-only tensors' current values -> (total norm, clip coefficient)"""
        for j, pg in enumerate(self.opt.param_groups):                 # trainer.py:463-474
            pg["lr"] = lr[j]
            if "momentum" in pg:
                pg["momentum"] = momentum[j]
            else:
                pg["betas"] = (momentum[j], pg["betas"][1])
        for n, p in self.params.items():
            p.grad = grads[n].detach().to(self.device, self.dtype).reshape(p.shape).clone()
        for pg in self.opt.param_groups:
            for p in pg["params"]:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
        self.ext.grad = torch.full_like(self.ext, math.sqrt(ext_sumsq))
        total = torch.nn.utils.clip_grad_norm_(list(self.params.values()) + [self.ext], max_norm=self.max_norm)
        self.opt.step()
        for n, b in (buffers or {}).items():
            self.buffers[n] = b.detach().to(self.device, self.dtype).clone()
        self.updates += 1                                              # torch_utils.py:767-774
        d = self.ema_decay * (1 - math.exp(-self.updates / self.ema_tau))
        msd = {**self.params, **self.buffers}
        for k, v in self.ema.items():
            v *= d
            v += (1 - d) * msd[k].detach()
        total = float(total)
        return total, min(1.0, self.max_norm / (total + 1e-6))

    def tensors(self):
        """{name: tensor}: parameters as 'param.<name>', averages as 'ema.<name>'"""
        out = {f"param.{n}": p.detach() for n, p in self.params.items()}
        out.update({f"ema.{n}": v for n, v in self.ema.items()})
        return out


def bar_check(what, got, f32, oracle, figures=None):
    """-> the misses [(what, error, bar)] of `got` against `oracle` (fp64), the bar set by torch's own fp32 result `f32`; prints every figure."""
    o = oracle.detach().double().cpu().reshape(-1)
    err = float((got.detach().double().cpu().reshape(-1) - o).abs().max())
    own = float((f32.detach().double().cpu().reshape(-1) - o).abs().max())
    scale = float(o.abs().max())
    bar = max(1e-6 * scale, 4.0 * own)
    print(f"{what}: error {err:.3e}, torch fp32's own {own:.3e}, |oracle|_max {scale:.3e}, bar {bar:.3e}")
    if figures is not None:
        figures.append((what, err, own, scale, bar))
    return [] if err <= bar else [(what, err, bar)]


def load_opt_golden(kind):
    """-> (npz of tests/golden/opt_<kind>.npz, the table of tests/golden/opt_groups.json)"""
    return np.load(os.path.join(GOLDEN, f"opt_{kind}.npz")), json.load(open(os.path.join(GOLDEN, "opt_groups.json")))


def golden_segments(z, table, device):
    """The golden's tiny model as optimizer segments on `device`: (Segment list, {name: gradient view}, bucket).  Parameters in the order of the
    table's shapes, their gradients views into one flat bucket, then the floating-point buffers of the EMA's state dict as EMA-only segments."""
    from mga_yolo_amd.optim import Segment
    names = list(table["shapes"])
    bucket = torch.zeros(sum(int(np.prod(table["shapes"][n])) for n in names), dtype=torch.float32, device=device)
    segs, grads, off = [], {}, 0
    for n in names:
        p = torch.from_numpy(z[f"init.{n}"]).to(device).contiguous()
        grads[n] = bucket[off:off + p.numel()].view(p.shape)
        off += p.numel()
        segs.append(Segment(n, p, grads[n], table["groups"][n]))
    for k in z.files:
        if k.startswith("init_ema.") and k[len("init_ema."):] not in table["shapes"]:
            segs.append(Segment(k[len("init_ema."):], torch.from_numpy(z[k]).to(device).contiguous(), None, 1))
    return segs, grads, bucket


def run_golden(kind, device):
    """The golden's three steps through BucketOptimizer on `device` -> the misses of every parameter and average after every step, against the
    reference's fp64 run, the bar set by the reference's own fp32 run."""
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    z, table = load_opt_golden(kind)
    sched = table["schedule"][GOLDEN_KINDS[kind]]
    segs, grads, _ = golden_segments(z, table, device)
    cfg = OptConfig(kind, lr=sched[0]["lr"], momentum=sched[0]["momentum"], weight_decay=table["decay"], max_norm=table["max_norm"],
                    ema_decay=table["ema"]["decay"], ema_tau=table["ema"]["tau"], check_finite=False)
    opt = BucketOptimizer(segs, cfg, device)
    misses, clipped = [], []
    for t in range(table["steps"]):
        for j in range(3):
            opt.set_group(j, lr=sched[t]["lr"][j], momentum=sched[t]["momentum"][j])
        for n, g in grads.items():
            g.copy_(torch.from_numpy(z[f"grad.{t}.{n}"]))
        opt.step()
        clipped.append(float(opt.clip_coef) < 1.0)
        ema = opt.ema_state()
        for s in segs:
            if s.grad is not None:
                misses += bar_check(f"{kind} step {t} param {s.name}", s.param, torch.from_numpy(z[f"param.{t}.{s.name}"]),
                                    torch.from_numpy(z[f"f64.param.{t}.{s.name}"]))
            misses += bar_check(f"{kind} step {t} ema {s.name}", ema[s.name], torch.from_numpy(z[f"ema.{t}.{s.name}"]),
                                torch.from_numpy(z[f"f64.ema.{t}.{s.name}"]))
    assert clipped == [True, False, True], clipped
    assert opt.updates == table["steps"] and opt.t == table["steps"]
    return misses


# ---- random segments at the sizes at which the chunking can go wrong ----------------------------------------------------------------
def make_case(device, seed=0):
    """The segments of LENGTHS in one flat parameter tensor and one bucket (so every view after the first is misaligned to 16 bytes) and one
    EMA-only segment -> (Segment list, {name: grad view}, bucket, {name: initial parameter}, groups, {name: buffer})"""
    from mga_yolo_amd.optim import Segment
    g = torch.Generator().manual_seed(seed)
    flat = (torch.randn(sum(LENGTHS), generator=g) * 0.5).to(device)
    bucket = torch.zeros(sum(LENGTHS), dtype=torch.float32, device=device)
    segs, grads, groups, off = [], {}, {}, 0
    for n, grp in zip(LENGTHS, GROUPS):
        name = f"seg{n}"
        grads[name], groups[name] = bucket[off:off + n], grp
        segs.append(Segment(name, flat[off:off + n], grads[name], grp))
        off += n
    buf = (torch.rand(EMA_ONLY, generator=g) + 0.5).to(device)
    segs.append(Segment("buffer", buf, None, 1))
    init = {s.name: s.param.clone() for s in segs if s.grad is not None}
    return segs, grads, bucket, init, groups, {"buffer": buf}


def step_grads(t, device, seed=100):
    g = torch.Generator().manual_seed(seed + t)
    return (torch.randn(sum(LENGTHS), generator=g) * 0.05).to(device)


def run_against_torch(kind, device, figures=None):
    """K steps of BucketOptimizer on `device` beside torch's own sequence on the same device (fp32) and on the host in fp64 -> misses"""
    from mga_yolo_amd.optim import BucketOptimizer, OptConfig
    segs, grads, bucket, init, groups, bufs = make_case(device)
    sched = SCHEDULE[kind]
    kw = dict(decay=5e-4, buffers=bufs, ema_decay=0.9999, ema_tau=5.0)
    t32 = TorchTail(kind, init, groups, dtype=torch.float32, device=device, **kw)
    t64 = TorchTail(kind, init, groups, dtype=torch.float64, device="cpu", **kw)
    opt = BucketOptimizer(segs, OptConfig(kind, lr=sched[0]["lr"], momentum=sched[0]["momentum"], weight_decay=5e-4, ema_tau=5.0), device)
    misses = []
    for t in range(K):
        bucket.copy_(step_grads(t, device))
        for j in range(3):
            opt.set_group(j, lr=sched[t]["lr"][j], momentum=sched[t]["momentum"][j])
        opt.set_external(sumsq=EXT_SUMSQ[t])
        gs = {n: g.clone() for n, g in grads.items()}
        opt.step()
        n32, _ = t32.step(gs, sched[t]["lr"], sched[t]["momentum"], ext_sumsq=EXT_SUMSQ[t], buffers=bufs)
        n64, c64 = t64.step(gs, sched[t]["lr"], sched[t]["momentum"], ext_sumsq=EXT_SUMSQ[t], buffers=bufs)
        coef = float(opt.clip_coef)
        assert (coef < 1.0) if EXT_SUMSQ[t] else (coef == 1.0), (t, coef)
        assert abs(float(opt.grad_norm) - n64) <= max(1e-6 * n64, 4 * abs(n32 - n64)), (t, float(opt.grad_norm), n32, n64)
        assert abs(coef - c64) <= 1e-6 and int(opt.found_inf) == 0
        ours = {f"param.{s.name}": s.param for s in segs if s.grad is not None}
        ours.update({f"ema.{n}": v for n, v in opt.ema.items()})
        a32, a64 = t32.tensors(), t64.tensors()
        assert sorted(ours) == sorted(a64)
        for name in ours:
            misses += bar_check(f"{kind} step {t} {name}", ours[name], a32[name], a64[name], figures)
    assert opt.updates == K and opt.t == K
    return misses
