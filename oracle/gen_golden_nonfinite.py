"""Record what the REFERENCE modules themselves do with a NaN or an infinity: which elements of every output come out non-finite, and the
values of the others.  These fixtures pin the autograd eager forms (``oracle/*_oracle.py: reference_form*``, ``tests/spade_oracle.py``)
that tests/test_gpu_nonfinite.py uses as the expected values of the HIP kernels under a poisoned input.

TEST INFRASTRUCTURE.  Run where the upstream reference is mounted read-only:

    PYTHONDONTWRITEBYTECODE=1 YOLO_CONFIG_DIR=/tmp/yolo_cfg python oracle/gen_golden_nonfinite.py

(the cv2 / torchvision stand-ins are those of oracle/gen_golden_head.py).  Written: ``tests/golden/nonfinite_<family>.npz``, per case the
inputs and every state_dict entry before the call, and per poison -- (target, index, value), recorded in the file -- for every output a
boolean finite-mask and the values with the non-finite ones set to 0.  One thread, so a second run writes the same bytes.

Only data is written -- no reference source text.
"""
import importlib.metadata as md
import io
import json
import os
import sys
import zipfile
from unittest.mock import MagicMock

import numpy as np

cv2 = MagicMock(name="cv2"); cv2.__version__ = "4.10.0"; cv2.__spec__ = None
sys.modules["cv2"] = cv2
_real_version = md.version
md.version = lambda n: "0.25.0" if n == "torchvision" else _real_version(n)
sys.path.insert(0, "/root/reference")

import torch  # noqa: E402

import mga_yolo  # noqa: E402,F401
from mga_yolo.nn.modules.masked_cbam import MaskCBAM  # noqa: E402  (the reference itself)
from mga_yolo.nn.modules.masked_eca import MaskECA  # noqa: E402
from mga_yolo.nn.modules.masked_spade import MaskSPADE  # noqa: E402
from mga_yolo.nn.modules.segmentation import MGAMaskHead  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
torch.set_num_threads(1)
NAN, INF = float("nan"), float("inf")
B, H, W = 3, 6, 5

# family -> [(case name, constructor, has a mask, training, [(poison id, target, value)])]; a target is x | mask | gy | a state_dict name
CASES = {
    "cbam": [("mask", lambda: MaskCBAM(8, r=4, spatial_k=3), True, True,
              [("x_nan", "x", NAN), ("x_pinf", "x", INF), ("x_ninf", "x", -INF), ("mask_nan", "mask", NAN), ("mask_pinf", "mask", INF),
               ("mask_ninf", "mask", -INF), ("gy_nan", "gy", NAN), ("gy_pinf", "gy", INF), ("param_nan", "cam_mlp.0.weight", NAN)]),
             ("nomask", lambda: MaskCBAM(8, r=4, spatial_k=3), False, True, [("x_nan", "x", NAN), ("x_pinf", "x", INF), ("gy_nan", "gy", NAN)]),
             ("raw", lambda: MaskCBAM(8, r=4, spatial_k=3, use_sigmoid_mask=False), True, True,
              [("mask_nan", "mask", NAN), ("mask_pinf", "mask", INF), ("mask_ninf", "mask", -INF)])],
    "eca": [("mask", lambda: MaskECA(8), True, True,
             [("x_nan", "x", NAN), ("x_ninf", "x", -INF), ("mask_nan", "mask", NAN), ("mask_pinf", "mask", INF), ("mask_ninf", "mask", -INF),
              ("gy_pinf", "gy", INF), ("param_nan", "conv1d.weight", NAN)]),
            ("nomask", lambda: MaskECA(8), False, True, [("x_pinf", "x", INF), ("gy_nan", "gy", NAN)]),
            ("raw", lambda: MaskECA(8, use_sigmoid_mask=False), True, True, [("mask_pinf", "mask", INF), ("mask_ninf", "mask", -INF)])],
    "spade": [("in", lambda: MaskSPADE(16, hidden=16, norm_type="in"), True, True,
               [("x_nan", "x", NAN), ("x_pinf", "x", INF), ("mask_nan", "mask", NAN), ("mask_pinf", "mask", INF), ("mask_ninf", "mask", -INF),
                ("gy_nan", "gy", NAN), ("param_nan", "conv_gamma.weight", NAN)]),
              ("bn", lambda: MaskSPADE(16, hidden=16, norm_type="bn"), True, True,
               [("x_nan", "x", NAN), ("mask_nan", "mask", NAN), ("gy_pinf", "gy", INF)]),
              ("raw", lambda: MaskSPADE(16, hidden=16, use_sigmoid_mask=False), True, True, [("mask_pinf", "mask", INF), ("mask_nan", "mask", NAN)])],
    "head": [("train", lambda: MGAMaskHead(8, 4), False, True,
              [("x_nan", "x", NAN), ("x_ninf", "x", -INF), ("gy_nan", "gy", NAN), ("gy_pinf", "gy", INF), ("param_nan", "proj.0.weight", NAN)]),
             ("eval", lambda: MGAMaskHead(8, 4), False, False,
              [("x_nan", "x", NAN), ("x_pinf", "x", INF), ("gy_nan", "gy", NAN), ("param_nan", "proj.0.weight", NAN)])],
}


def build(make, seed):
    """A "trained-like" module: every parameter perturbed, the batch-norm statistics too (as oracle/gen_golden_head.py does)."""
    torch.manual_seed(seed)
    m = make()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g))
        for name, b in m.named_buffers():
            if name.endswith("running_mean"):
                b.add_(0.2 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.mul_(0.5 + torch.rand(b.shape, generator=g))
    return m


def middle(shape, b=None):
    return tuple(([b] if b is not None else []) + [n // 2 for n in (shape[1:] if b is not None else shape)])


def run(m, x, mask, gy):
    xl = x.clone().requires_grad_(True)
    ml = None if mask is None else mask.clone().requires_grad_(True)
    m.zero_grad()
    y = m(xl if ml is None else [xl, ml])
    y.backward(gy)
    out = {"y": y.detach(), "gx": xl.grad}
    if ml is not None:
        out["gmask"] = ml.grad
    out.update({"g." + k: p.grad for k, p in m.named_parameters()})
    out.update({"after." + k: v.detach().clone() for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))})
    return out


def savez_fixed(path, arrays):
    """np.savez_compressed with the archive's time stamps fixed: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(2020, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    os.makedirs(OUT, exist_ok=True)
    for fi, (family, cases) in enumerate(CASES.items()):
        arrays, meta = {}, {}
        for ci, (name, make, has_mask, training, poisons) in enumerate(cases):
            seed = 100 * fi + 10 * ci
            m0 = build(make, seed).train(training)
            state0 = {k: v.detach().clone() for k, v in m0.state_dict().items()}
            C = 16 if family == "spade" else 8
            g = torch.Generator().manual_seed(seed + 2)
            x = torch.randn(B, C, H, W, generator=g)
            mask = torch.randn(B, 1, H, W, generator=g) if has_mask else None
            if mask is not None and name == "raw":
                mask = torch.rand(B, 1, H, W, generator=g)
            gy = torch.randn(B, 1 if family == "head" else C, H, W, generator=g)
            arrays[f"{name}.x"], arrays[f"{name}.gy"] = x.numpy(), gy.numpy()
            if mask is not None:
                arrays[f"{name}.mask"] = mask.numpy()
            for k, v in state0.items():
                arrays[f"{name}.param.{k}"] = v.numpy()
            cfg = {}
            if family in ("cbam", "eca"):
                cfg = dict(use_sigmoid_mask=name != "raw", tiny_thr=1e-4, eps=1e-6)
            elif family == "spade":
                cfg = dict(norm_type="bn" if name == "bn" else "in", use_sigmoid_mask=name != "raw", eps=float(m0.norm.eps), momentum=0.1)
            else:
                cfg = dict(eps=float(m0.proj[1].eps), momentum=float(m0.proj[1].momentum))
            meta[name] = dict(training=training, has_mask=has_mask, cfg=cfg, poisons=[])
            for pid, target, value in [("clean", None, None)] + poisons:
                m = build(make, seed).train(training)
                m.load_state_dict(state0)
                t = dict(x=x.clone(), mask=None if mask is None else mask.clone(), gy=gy.clone())
                index = None
                if target in ("x", "mask", "gy"):
                    index = middle(t[target].shape, B // 2)
                    t[target][index] = value
                elif target is not None:
                    p = dict(m.named_parameters())[target]
                    index = middle(p.shape)
                    with torch.no_grad():
                        p[index] = value
                out = run(m, t["x"], t["mask"], t["gy"])
                for k, v in out.items():
                    fin = torch.isfinite(v)
                    arrays[f"{name}.{pid}.finite.{k}"] = fin.numpy()
                    arrays[f"{name}.{pid}.value.{k}"] = torch.where(fin, v, torch.zeros_like(v)).numpy()
                meta[name]["poisons"].append(dict(id=pid, target=target, index=index, value=None if value is None else repr(value)))
                print(f"{family:5s} {name:6s} {pid:10s} " + " ".join(f"{k}:{int((~torch.isfinite(v)).sum())}/{v.numel()}" for k, v in out.items()))
        arrays["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
        savez_fixed(os.path.join(OUT, f"nonfinite_{family}.npz"), arrays)


if __name__ == "__main__":
    sys.exit(main())
