"""Write tests/golden/image_*.npz from the REFERENCE's own DetectionTrainer.preprocess_batch and DetectionValidator.preprocess (data only --
no reference text is copied), and tests/golden/image_ratios.json.

    python tools/gen_golden_image.py --reference <checkout of the reference project>

Run on the build machine, where the reference is available; it never travels with this repository.  The reference is imported with the
recipe of tools/gen_golden_nms.py.  Its two methods are called unbound on a stand-in that carries what they read: device, stride,
args.multi_scale, args.imgsz, args.half.

  image_<case>.npz        for every no-resize case of tests/image_cases.py: src (the bytes), seed, ref_f32 (the trainer's fp32 output) and
                          ref_f16 (the validator's output under args.half)
  image_ms<seed>.npz      multi_scale at imgsz 64, stride 32 on the (2,3,40,56) source after random.seed(seed), seeds 0, 1 and 5: src, seed,
                          size (what the reference resized to), ref_f32
  image_sizes.npz         seeds 0 .. 31 for each source shape of image_cases.SIZES_HW: only the output shapes the reference picked
  image_ratios.json       the worst |torch's own fp32 host result - oracle| / terms over the resize cases: K of the tests is twice that

Every record is checked against the oracle before it is written: equal bits without a resize, within 2 x the worst ratio with one."""
import argparse
import json
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden_nms import import_reference  # noqa: E402


def stand_in(multi_scale=False, half=False, imgsz=64, stride=32):
    return SimpleNamespace(device=torch.device("cpu"), stride=stride, args=SimpleNamespace(multi_scale=multi_scale, imgsz=imgsz, half=half))


def labels():
    return dict(batch_idx=torch.zeros(1), cls=torch.zeros(1, 1), bboxes=torch.zeros(1, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    import_reference(args.reference)
    from ultralytics.models.yolo.detect.train import DetectionTrainer
    from ultralytics.models.yolo.detect.val import DetectionValidator
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ROOT)
    import image_cases as IC
    import image_oracle as IO

    ratios = IO.torch_ratio(IC.RESIZE)
    assert ratios["nonzero_at_zero_terms"] == 0 and ratios["zero_terms"] > 0
    with open(IC.RATIOS, "w") as f:
        json.dump(ratios, f, indent=1)
        f.write("\n")
    K = 2.0 * ratios["forward"]
    print(f"image_ratios.json: worst ratio {ratios['forward']:.4f} over {len(IC.RESIZE)} cases, {ratios['elements']} elements, "
          f"{ratios['zero_terms']} with zero terms")

    for c in IC.PLAIN:
        src = IC.plain_source(c)
        f32 = DetectionTrainer.preprocess_batch(stand_in(), {"img": src.clone()})["img"]
        f16 = DetectionValidator.preprocess(stand_in(half=True), dict(labels(), img=src.clone()))["img"]
        v32 = DetectionValidator.preprocess(stand_in(), dict(labels(), img=src.clone()))["img"]
        assert f32.dtype == torch.float32 and f16.dtype == torch.float16 and torch.equal(v32, f32)
        want, _ = IO.image(src)
        assert torch.equal(f32, IO.rounded(want, torch.float32)) and torch.equal(f16, IO.rounded(want, torch.float16)), c.name
        np.savez_compressed(IC.path(c.name), src=src.numpy(), seed=IC.SEED, ref_f32=f32.numpy(), ref_f16=f16.numpy())
        print(f"{c.name}: {os.path.getsize(IC.path(c.name)) / 1024:.0f} KB")

    M = IC.MULTI_SCALE
    src = IC.source(M["shape"])
    for seed, size in M["seeds"].items():
        random.seed(seed)
        out = DetectionTrainer.preprocess_batch(stand_in(multi_scale=True, imgsz=M["imgsz"], stride=M["stride"]), {"img": src.clone()})["img"]
        assert tuple(out.shape[2:]) == size, (seed, tuple(out.shape), size)
        r, z, nz, bad = IO.ratio(out, *IO.image(src, size))
        assert r <= K and nz == 0 and bad == 0 and z > 0, (seed, r, z, nz, bad)
        np.savez_compressed(IC.path(f"ms{seed}"), src=src.numpy(), seed=seed, size=np.array(size), ref_f32=out.numpy())
        print(f"ms{seed}: {size}, ratio {r:.3f}, {z} zero-terms elements, {os.path.getsize(IC.path(f'ms{seed}')) / 1024:.0f} KB")

    picked = {}
    for hw in IC.SIZES_HW:
        img = torch.zeros(1, 3, *hw, dtype=torch.uint8)
        rows = []
        for seed in range(IC.SIZES_SEEDS):
            random.seed(seed)
            out = DetectionTrainer.preprocess_batch(stand_in(multi_scale=True, imgsz=M["imgsz"], stride=M["stride"]), {"img": img.clone()})["img"]
            rows.append(tuple(out.shape[2:]))
        picked[f"hw_{hw[0]}x{hw[1]}"] = np.array(rows, dtype=np.int64)
        print(f"sizes for {hw}: {sorted(set(rows))}")
    np.savez_compressed(IC.path("sizes"), imgsz=M["imgsz"], stride=M["stride"], **picked)


if __name__ == "__main__":
    main()
