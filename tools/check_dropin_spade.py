"""Drop-in proof for MaskSPADE against the reference's REAL model factory, recorded like oracle/check_dropin.py records MaskCBAM's.

    PYTHONDONTWRITEBYTECODE=1 YOLO_CONFIG_DIR=<a scratch directory> python tools/check_dropin_spade.py --reference <reference checkout>

Build machine only (the reference never travels).  Builds the reference's ``MGAModel`` from ``configs/models/yolov8_spade.yaml`` (scale n)
un-patched at seed 0, calls ``mga_yolo_amd.install(strict=True)`` and builds it again through the reference's own ``parse_model``; records
the classes of the mask-guided layers, the attributes parse_model attaches, state_dict key / value equality at the same seed, strict
cross-loading, eval- and train-mode CPU forward equality, deepcopy, and that ``uninstall()`` restores the reference.  Data only is
written: ``tests/golden/spade_dropin_report.json`` (asserted by tests/test_spade_dropin_fixture.py).
"""
import argparse
import copy
import importlib.metadata as md
import json
import os
import shutil
import sys
import tempfile
from unittest.mock import MagicMock

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "spade_dropin_report.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ref_root = ap.parse_args().reference
    cv2 = MagicMock(name="cv2")                            # absent from the build image; nothing of it runs on this path
    cv2.__version__, cv2.__spec__ = "4.10.0", None
    sys.modules["cv2"] = cv2
    real = md.version
    md.version = lambda n: "0.25.0" if n == "torchvision" else real(n)
    sys.path.insert(0, ref_root)
    sys.path.insert(0, ROOT)
    import torch
    torch.set_num_threads(4)
    import mga_yolo  # noqa: F401
    from mga_yolo.model.model import MGAModel
    from mga_yolo.nn.modules.masked_spade import MaskSPADE as RefSPADE
    import mga_yolo_amd

    tmp = tempfile.mkdtemp(prefix="dropin_spade_")
    try:
        yaml = os.path.join(tmp, "yolov8n_spade.yaml")     # yaml_model_load takes the scale from the file name
        shutil.copy(os.path.join(ref_root, "configs", "models", "yolov8_spade.yaml"), yaml)

        def build():
            torch.manual_seed(0)
            return MGAModel(yaml, nc=1, verbose=False)

        def flat(o):
            if isinstance(o, torch.Tensor):
                return [o.detach()]
            if isinstance(o, dict):
                return [t for k in sorted(o) for t in flat(o[k])]
            if isinstance(o, (list, tuple)):
                return [t for v in o for t in flat(v)]
            return []

        def rel(x, y):
            return float((x.double() - y.double()).abs().max() / y.double().abs().max().clamp_min(1e-30))

        img = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(11))
        ref = build()
        idx = [i for i, L in enumerate(ref.model) if isinstance(L, RefSPADE)]
        sd_ref = {k: v.clone() for k, v in ref.state_dict().items()}
        ref.eval()
        with torch.no_grad():
            e_ref = flat(ref(img))
        ref.train()
        t_ref = flat(ref(img))
        patched = mga_yolo_amd.install(strict=True)
        new = build()
        R = {"torch": torch.__version__, "yaml": "configs/models/yolov8_spade.yaml", "scale": "n", "patched_modules": patched,
             "spade_layers": idx, "layers": {}}
        for i in idx:
            L = new.model[i]
            R["layers"][str(i)] = dict(cls=f"{type(L).__module__}.{type(L).__name__}", i=L.i, f=L.f, type=L.type, np=int(L.np),
                                       ref_np=int(ref.model[i].np), cfg=dict(vars(L.cfg)) if not hasattr(L.cfg, "__dataclass_fields__") else
                                       {k: getattr(L.cfg, k) for k in L.cfg.__dataclass_fields__},
                                       scale_name=L.scale_name, state={k: list(v.shape) for k, v in L.state_dict().items()})
        R["blocks_are_ours"] = all(type(new.model[i]) is mga_yolo_amd.MaskSPADE for i in idx)
        sd_new = new.state_dict()
        R["state_keys_equal"] = list(sd_ref) == list(sd_new)
        R["state_values_equal_same_seed"] = all(torch.equal(sd_ref[k], sd_new[k]) for k in sd_ref)
        new.load_state_dict(sd_ref, strict=True)
        ref.load_state_dict(new.state_dict(), strict=True)
        R["cross_load_strict"] = True
        new.eval()
        with torch.no_grad():
            e_new = flat(new(img))
        new.train()
        t_new = flat(new(img))
        R["eval_forward_rel_diff"] = max(rel(a, b) for a, b in zip(e_new, e_ref))
        R["train_forward_rel_diff"] = max(rel(a, b) for a, b in zip(t_new, t_ref))
        from mga_yolo.nn.modules.masked_spade import MaskSPADE as Late
        R["late_import_is_ours"] = Late is mga_yolo_amd.MaskSPADE
        R["deepcopy_ok"] = all(type(copy.deepcopy(new).model[i]) is mga_yolo_amd.MaskSPADE for i in idx)
        mga_yolo_amd.uninstall()
        from mga_yolo.nn.modules.masked_spade import MaskSPADE as Back
        R["uninstall_restores"] = Back is RefSPADE and all(type(build().model[i]) is RefSPADE for i in idx)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(OUT, "w") as f:
        json.dump(R, f, indent=1, sort_keys=True)
    print(json.dumps({k: v for k, v in R.items() if k != "layers"}))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
