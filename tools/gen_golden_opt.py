"""Write tests/golden/opt_{sgd,adamw}.npz and tests/golden/opt_groups.json from the REFERENCE's own trainer (data only -- no reference text
is copied).

    python tools/gen_golden_opt.py --reference <checkout of the reference project> [--check]

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of DESIGN 8 (a stand-in ``cv2``, an answered ``torchvision`` version).  A tiny model is built from the reference's own
``MGAMaskHead(16, 8)``, ``MaskCBAM(16)``, ``MaskECA(16)``, ``MaskSPADE(16, hidden=4, norm_type="bn")`` and a 2-element ``mtl_log_vars``; the
reference's ``BaseTrainer.build_optimizer`` and ``BaseTrainer.optimizer_step`` are called UNBOUND on a stand-in ``self`` (a disabled
GradScaler, ``ModelEMA(decay=0.9999, tau=5)``), for "SGD" and for "AdamW".  Three steps on seeded gradients -- scaled so that the clip is
active at steps 0 and 2 and inactive at step 1 -- with every group's lr and momentum changed before each step as warm-up does
(trainer.py:463-474).  Recorded: the group of every parameter name, the schedule, the gradients, and after each step every parameter and
every floating-point EMA entry -- from the fp32 run and from the same run with the model in fp64 (the oracle the tests' bars come from)."""
import argparse
import importlib.metadata as md
import json
import os
import sys
from types import SimpleNamespace
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
STEPS = 3
GRAD_SCALE = (1.0, 0.05, 1.0)                    # |g| = 40, 2, 40 against max_norm = 10: clipped, not clipped, clipped
DECAY = 5e-4
# per step, per group (param_groups order): lr, momentum -- warm-up moves the bias group's lr down and the others' up, momentum up
SCHEDULE = dict(
    SGD=[dict(lr=[0.1, 0.002, 0.002], momentum=[0.8, 0.8, 0.8]), dict(lr=[0.07, 0.006, 0.006], momentum=[0.85, 0.85, 0.85]),
         dict(lr=[0.04, 0.01, 0.01], momentum=[0.937, 0.937, 0.937])],
    AdamW=[dict(lr=[0.0, 0.0004, 0.0004], momentum=[0.8, 0.8, 0.8]), dict(lr=[0.001, 0.0012, 0.0012], momentum=[0.85, 0.85, 0.85]),
           dict(lr=[0.002, 0.002, 0.002], momentum=[0.9, 0.9, 0.9])])


def import_reference(ref_root):
    cv2 = MagicMock(name="cv2")                            # absent from the build image; nothing of it runs on this path
    cv2.__version__, cv2.__spec__ = "4.10.0", None
    sys.modules["cv2"] = cv2
    real = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else real(n)
    sys.path.insert(0, ref_root)
    import mga_yolo  # noqa: F401  (puts the vendored detector on the path)
    from mga_yolo.nn.modules.masked_cbam import MaskCBAM
    from mga_yolo.nn.modules.masked_eca import MaskECA
    from mga_yolo.nn.modules.masked_spade import MaskSPADE
    from mga_yolo.nn.modules.segmentation import MGAMaskHead
    from ultralytics.engine.trainer import BaseTrainer
    from ultralytics.utils.torch_utils import ModelEMA
    return SimpleNamespace(MaskCBAM=MaskCBAM, MaskECA=MaskECA, MaskSPADE=MaskSPADE, MGAMaskHead=MGAMaskHead, BaseTrainer=BaseTrainer,
                           ModelEMA=ModelEMA)


def build_model(R, torch):
    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.head = R.MGAMaskHead(16, 8)
            self.cbam = R.MaskCBAM(16)
            self.eca = R.MaskECA(16)
            self.spade = R.MaskSPADE(16, hidden=4, norm_type="bn")
            self.mtl_log_vars = torch.nn.Parameter(torch.zeros(2))
    torch.manual_seed(7)
    m = Tiny()
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():                                   # no parameter at zero, no running statistic at its initial value
        for p in m.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        for k, b in m.named_buffers():
            if b.dtype.is_floating_point:
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return m


def run(R, torch, name, dtype):
    model = build_model(R, torch).to(dtype)
    stub = SimpleNamespace(args=SimpleNamespace(lr0=0.01, momentum=0.9, warmup_bias_lr=0.1), data={}, model=model)
    opt = R.BaseTrainer.build_optimizer(stub, model, name=name, lr=SCHEDULE[name][0]["lr"][1], momentum=0.9, decay=DECAY)
    stub.optimizer = opt
    stub.scaler = torch.amp.GradScaler("cpu", enabled=False)
    stub.ema = R.ModelEMA(model, decay=0.9999, tau=5)
    ids = {id(p): n for n, p in model.named_parameters()}
    groups = {ids[id(p)]: j for j, pg in enumerate(opt.param_groups) for p in pg["params"]}
    decays = [float(pg["weight_decay"]) for pg in opt.param_groups]
    arrays = {}
    for n, p in model.named_parameters():
        arrays[f"init.{n}"] = p.detach().numpy().copy()
    for k, v in stub.ema.ema.state_dict().items():
        if v.dtype.is_floating_point:
            arrays[f"init_ema.{k}"] = v.detach().numpy().copy()
    g = torch.Generator().manual_seed(9)
    for t in range(STEPS):
        for j, pg in enumerate(opt.param_groups):                       # trainer.py:463-474
            pg["lr"] = SCHEDULE[name][t]["lr"][j]
            if "momentum" in pg:
                pg["momentum"] = SCHEDULE[name][t]["momentum"][j]
            else:
                pg["betas"] = (SCHEDULE[name][t]["momentum"][j], pg["betas"][1])
        for n, p in model.named_parameters():
            grad = torch.randn(p.shape, generator=g) * GRAD_SCALE[t]    # drawn in fp32 in both runs: the two see the same gradients
            arrays[f"grad.{t}.{n}"] = grad.numpy().copy()
            p.grad = grad.to(dtype)
        R.BaseTrainer.optimizer_step(stub)
        for n, p in model.named_parameters():
            arrays[f"param.{t}.{n}"] = p.detach().numpy().copy()
        for k, v in stub.ema.ema.state_dict().items():
            if v.dtype.is_floating_point:
                arrays[f"ema.{t}.{k}"] = v.detach().numpy().copy()
    return arrays, groups, decays, type(opt).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--check", action="store_true", help="compare with the stored fixtures instead of writing them")
    a = ap.parse_args()
    R = import_reference(a.reference)
    import torch
    torch.set_num_threads(4)
    table = dict(schedule=SCHEDULE, grad_scale=list(GRAD_SCALE), steps=STEPS, decay=DECAY, ema=dict(decay=0.9999, tau=5), max_norm=10.0,
                 torch=torch.__version__)
    for name in ("SGD", "AdamW"):
        a32, groups, decays, cls = run(R, torch, name, torch.float32)
        a64, groups64, _, _ = run(R, torch, name, torch.float64)
        assert groups == groups64 and cls == name
        arrays = dict(a32)
        arrays.update({"f64." + k: v for k, v in a64.items() if k.startswith(("param.", "ema."))})
        table.setdefault("groups", groups)
        assert table["groups"] == groups, "the two optimizers group the parameters alike"
        table.setdefault("group_weight_decay", decays)
        assert table["group_weight_decay"] == decays
        table["shapes"] = {k[len("init."):]: list(v.shape) for k, v in a32.items() if k.startswith("init.")}
        path = os.path.join(OUT, f"opt_{name.lower()}.npz")
        if a.check:
            z = np.load(path)
            assert sorted(z.files) == sorted(arrays), name
            worst = max(float(np.abs(z[k].astype(np.float64) - arrays[k]).max()) / max(float(np.abs(z[k]).max()), 1e-30) for k in z.files)
            print(name, "reproduced, worst relative difference", worst)
            assert worst < 1e-6
        else:
            np.savez(path, **arrays)
            print(name, os.path.getsize(path), "bytes,", len(groups), "parameters")
    path = os.path.join(OUT, "opt_groups.json")
    if a.check:
        have = json.load(open(path))
        have.pop("torch"); table.pop("torch")
        assert have == json.loads(json.dumps(table)), "opt_groups.json"
        print("opt_groups.json reproduced")
    else:
        json.dump(table, open(path, "w"), indent=1, sort_keys=True)
        print(json.dumps(table["groups"], indent=1))


if __name__ == "__main__":
    main()
