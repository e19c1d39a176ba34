"""Write tests/golden/spade_<name>.npz from the REFERENCE's own MaskSPADE (data only -- no reference text is copied).

    python tools/gen_golden_spade.py --reference <checkout of the reference project>

Run on the build machine, where the reference is available; it never travels with this repository.  The reference's
``mga_yolo/nn/modules/masked_spade.py`` needs torch alone, so the file is loaded by path (the package's __init__ would pull in the
vendored detector).  Per case: inputs from ``tests/conftest.synth``, the reference module built at ``meta.init_seed`` (checksums of that
initial state are kept in ``meta.init_checksums``: the same seed must give this project's class the same values) and then perturbed so
that no bias is zero, one fp32 forward + backward on the CPU, and the running statistics after the step.

ReLU edge: a pre-activation within rounding of zero could take the other branch on the device, which moves gradients by a finite amount.
A seed is rejected unless every fp64 pre-activation has |pre| >= 1e-5 (``meta.min_abs_pre``); no element is excluded from any fixture.
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import checksum, synth  # noqa: E402
import spade_oracle as SO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
KEYS = SO.PARAM_KEYS
# name: dict(shape=(B,C,H,W), hidden, norm, train, and the optional: mask_kind, mask3d, sigmoid, mask_hw, mask_channels)
CASES = {
    "in_train": dict(shape=(2, 64, 12, 12), hidden=64, norm="in", train=True),
    "in_eval": dict(shape=(2, 16, 10, 10), hidden=16, norm="in", train=False),
    "bn_train": dict(shape=(2, 64, 16, 16), hidden=16, norm="bn", train=True),
    "bn_eval": dict(shape=(2, 32, 16, 16), hidden=16, norm="bn", train=False),
    "nomask": dict(shape=(2, 32, 12, 12), hidden=16, norm="in", train=True, mask_kind="none"),
    "nomask_bn": dict(shape=(2, 16, 9, 7), hidden=16, norm="bn", train=True, mask_kind="none"),
    "mask3d": dict(shape=(2, 16, 12, 12), hidden=16, norm="in", train=True, mask3d=True),
    "nosigmoid": dict(shape=(2, 16, 12, 12), hidden=16, norm="in", train=True, mask_kind="prob", sigmoid=False),
    "odd17x23": dict(shape=(2, 32, 17, 23), hidden=32, norm="in", train=True),
    "c192": dict(shape=(1, 192, 8, 8), hidden=16, norm="bn", train=True),
    "c256_b1": dict(shape=(1, 256, 6, 10), hidden=16, norm="in", train=True),
    "halfmask": dict(shape=(2, 16, 16, 16), hidden=16, norm="in", train=True, mask_hw=(8, 8)),
    "stride_probe": dict(shape=(1, 16, 8, 8), hidden=16, norm="bn", train=False),
    "maskc2": dict(shape=(2, 16, 8, 8), hidden=16, norm="in", train=True, mask_channels=2),
    # C a multiple of 16 but not of 32 / of the forward's channel block, on a grid small enough for that block to be halved
    "c80": dict(shape=(2, 80, 12, 12), hidden=16, norm="in", train=True),
    "c144_bn": dict(shape=(2, 144, 8, 8), hidden=32, norm="bn", train=True),
}


def load_reference(path):
    src = os.path.join(path, "mga_yolo", "nn", "modules", "masked_spade.py")
    spec = importlib.util.spec_from_file_location("ref_masked_spade", src)
    mod = importlib.util.module_from_spec(spec)
    sys.modules["ref_masked_spade"] = mod
    spec.loader.exec_module(mod)
    return mod.MaskSPADE


def make_case(Ref, name, c, seed):
    B, C, H, W = c["shape"]
    x, mask, gy = synth(B, C, H, W, seed=seed, mask_kind=c.get("mask_kind", "randn"), mask3d=c.get("mask3d", False))
    g = torch.Generator().manual_seed(seed + 1)
    if mask is not None and "mask_hw" in c:
        mask = torch.randn(B, 1, *c["mask_hw"], generator=g)
    K = c.get("mask_channels", 1)
    if mask is not None and K > 1:
        mask = torch.randn(B, K, H, W, generator=g)
    torch.manual_seed(seed)
    m = Ref(C, hidden=c["hidden"], mask_channels=K, norm_type=c["norm"], use_sigmoid_mask=c.get("sigmoid", True))
    init_sums = {k: checksum(v) for k, v in m.state_dict().items() if k in KEYS}
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k in KEYS:
                v.add_(0.05 * torch.randn(v.shape, generator=g))
        if c["norm"] == "bn":
            m.norm.running_mean.copy_(0.3 * torch.randn(C, generator=g))
            m.norm.running_var.copy_(0.5 + torch.rand(C, generator=g))
    m.train(c["train"])
    params = {k: v.detach().clone() for k, v in m.state_dict().items() if k in KEYS}
    run0 = {k: v.detach().clone() for k, v in m.state_dict().items() if k.startswith("norm.")}
    min_pre = None
    if mask is not None and K == 1:
        _, octx = SO.forward(x, mask, params, c["norm"], c["train"], c.get("sigmoid", True), 1e-6,
                             (run0["norm.running_mean"], run0["norm.running_var"]) if run0 else None)
        min_pre = SO.min_abs_pre(octx)
        if min_pre < 1e-5:
            return None
    xr = x.clone().requires_grad_(True)
    mr = None if mask is None else mask.clone().requires_grad_(True)
    y = m(xr if mr is None else [xr, mr])
    y.backward(gy)
    arrays = dict(x=x.numpy(), gy=gy.numpy())
    if mask is not None:
        arrays["mask"] = mask.numpy()
    for k, v in params.items():
        arrays["param." + k] = v.numpy()
    for k, v in run0.items():
        arrays["run0." + k] = v.numpy()
    arrays["out.y"] = y.detach().numpy()
    arrays["out.gx"] = xr.grad.numpy()
    if mr is not None:
        arrays["out.gmask"] = mr.grad.numpy()
        for k, p in m.named_parameters():
            arrays["out.g." + k] = p.grad.numpy()
    for k, v in m.state_dict().items():
        if k.startswith("norm."):
            arrays["out." + k] = v.detach().numpy()
    meta = dict(name=name, shape=[B, C, H, W], hidden=c["hidden"], norm_type=c["norm"], training=c["train"], mask_channels=K,
                use_sigmoid_mask=c.get("sigmoid", True), eps=1e-6, seed=seed, init_seed=seed, init_checksums=init_sums,
                min_abs_pre=min_pre, torch=torch.__version__)
    arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--check", action="store_true", help="compare with the stored fixtures instead of writing them")
    ap.add_argument("--only", action="append", help="write / check this case alone (repeatable); seeds do not depend on it")
    a = ap.parse_args()
    torch.set_num_threads(4)
    Ref = load_reference(a.reference)
    worst = 0.0
    for i, (name, c) in enumerate(CASES.items()):
        seed = 4100 + 10 * i
        if a.only and name not in a.only:
            continue
        arrays = None
        while arrays is None:
            arrays = make_case(Ref, name, c, seed)
            seed += 1
        path = os.path.join(OUT, f"spade_{name}.npz")
        if a.check:
            z = np.load(path)
            assert sorted(z.files) == sorted(arrays), name
            for k in z.files:
                if k != "meta":
                    den = max(float(np.abs(z[k]).max()), 1e-30)
                    worst = max(worst, float(np.abs(z[k].astype(np.float64) - arrays[k]).max()) / den)
            print(name, "reproduced")
        else:
            np.savez(path, **arrays)
            print(name, os.path.getsize(path), "bytes", json.loads(bytes(arrays["meta"]).decode())["min_abs_pre"])
    if a.check:
        print("worst relative difference", worst)
        assert worst < 1e-6


if __name__ == "__main__":
    main()
