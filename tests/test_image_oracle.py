"""The image batch without a GPU: the oracle (tests/image_oracle.py) against what the reference's own preprocess methods returned
(tests/golden/image_*.npz, written by tools/gen_golden_image.py), multi_scale_size against the reference's recorded picks, image_batch on
host tensors, and install(preprocess=True) on stand-ins for the reference's modules."""
import random
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_cases as IC
import image_oracle as IO
from mga_yolo_amd import image as IM
from mga_yolo_amd import image_batch, multi_scale_size

K = IO.load_k()
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _load(name):
    return np.load(IC.path(name), allow_pickle=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_rule_on_all_256_bytes():
    v = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)
    want, terms = IO.image(v)
    assert not terms.any()
    for dt in DTYPES:
        assert torch.equal(IO.rounded(want, dt), v.to(dt) / 255), dt                     # the quotient, bit for bit, in the three types
    product = v.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    assert int((product != v.float() / 255).sum()) == 126                                # why the division stays a division


@pytest.mark.parametrize("c", IC.PLAIN, ids=[c.name for c in IC.PLAIN])
def test_no_resize_equals_the_reference_bit_for_bit(c):
    z = _load(c.name)
    src = torch.from_numpy(z["src"])
    assert torch.equal(src, IC.plain_source(c)) and int(z["seed"]) == IC.SEED and tuple(src.shape) == c.shape
    want, terms = IO.image(src)
    assert not terms.any()
    assert torch.equal(IO.rounded(want, torch.float32), torch.from_numpy(z["ref_f32"]))
    assert torch.equal(IO.rounded(want, torch.float16), torch.from_numpy(z["ref_f16"]))


@pytest.mark.parametrize("seed", sorted(IC.MULTI_SCALE["seeds"]))
def test_multi_scale_reference_output_is_within_the_oracle_s_bars(seed):
    z = _load(f"ms{seed}")
    src = torch.from_numpy(z["src"])
    size = tuple(int(s) for s in z["size"])
    assert torch.equal(src, IC.source(IC.MULTI_SCALE["shape"])) and size == IC.MULTI_SCALE["seeds"][seed] and int(z["seed"]) == seed
    ref = torch.from_numpy(z["ref_f32"])
    assert tuple(ref.shape) == IC.MULTI_SCALE["shape"][:2] + size
    r, zero, nonzero, bad = IO.ratio(ref, *IO.image(src, size))
    print(f"seed {seed} -> {size}: ratio {r:.4f} (K = {K:.4f}), {zero} zero-terms elements")
    assert r <= K and bad == 0
    assert zero > 0 and nonzero == 0                                                     # the black quarter: exactly 0.0 there


def test_recorded_ratio_is_torch_s_own():
    import json
    with open(IC.RATIOS) as f:
        rec = json.load(f)
    assert sorted(rec["per_case"]) == sorted(c.name for c in IC.RESIZE)
    assert rec["nonzero_at_zero_terms"] == 0 and rec["zero_terms"] > 0 and 0.5 < rec["forward"] < 4
    c = IC.RESIZE_BY_NAME["down_odd"]
    assert IO.torch_ratio([c])["forward"] <= rec["forward"] + 1e-9                        # one case, run again here


def test_multi_scale_size_against_the_recorded_picks():
    z = _load("sizes")
    imgsz, stride = int(z["imgsz"]), int(z["stride"])
    for hw in IC.SIZES_HW:
        rows = z[f"hw_{hw[0]}x{hw[1]}"]
        assert rows.shape == (IC.SIZES_SEEDS, 2)
        for seed in range(IC.SIZES_SEEDS):
            random.seed(seed)
            got = multi_scale_size(imgsz, stride, hw)
            after = random.getstate()
            random.seed(seed)
            random.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride))
            assert after == random.getstate(), seed                                       # exactly one draw per call
            assert (got or hw) == tuple(int(v) for v in rows[seed]), (hw, seed)
            rng = random.Random(seed)                                                     # a generator of the caller's gives the same pick
            assert multi_scale_size(imgsz, stride, hw, rng=rng) == got
    same = [s for s in range(IC.SIZES_SEEDS) if tuple(z["hw_48x64"][s]) == (48, 64)]
    assert same
    random.seed(same[0])
    assert multi_scale_size(imgsz, stride, (48, 64)) is None                              # sf == 1: the reference does not resize


# ---------------------------------------------------------------------------------------------------------------------------
# image_batch on host tensors
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", IC.PLAIN, ids=[c.name for c in IC.PLAIN])
def test_host_image_batch_no_resize(c):
    src = IC.plain_source(c)
    B, Cc, H, W = c.shape
    for dt in DTYPES:
        for cl in (False, True):
            for layout in ("nchw", "nhwc"):
                for rev in (False, True):
                    v = src.permute(0, 2, 3, 1).contiguous() if layout == "nhwc" else src
                    want = IO.rounded(IO.image(v, None, layout, rev)[0], dt)
                    got = image_batch(v, dtype=dt, channels_last=cl, src_layout=layout, reverse_channels=rev)
                    assert got.dtype == dt and tuple(got.shape) == c.shape and torch.equal(got, want), (dt, cl, layout, rev)
                    assert got.is_contiguous(memory_format=torch.channels_last if cl else torch.contiguous_format)
                    assert not got.requires_grad


def test_host_image_batch_resize_out_and_size_forms():
    c = IC.RESIZE_BY_NAME["down_odd"]
    src = IC.resize_source(c)
    want, terms = IO.image(src, c.out_hw)
    got = image_batch(src, size=c.out_hw)
    r, zero, nonzero, bad = IO.ratio(got, want, terms)
    assert r <= K and zero > 0 and nonzero == 0 and bad == 0 and tuple(got.shape) == (c.B, c.C) + c.out_hw
    for dt in (torch.float16, torch.bfloat16):
        r, _, nonzero, bad = IO.within(image_batch(src, size=c.out_hw, dtype=dt), want, terms, K, dt)
        assert r <= K and nonzero == 0 and bad == 0
    assert tuple(image_batch(src, size=24).shape) == (c.B, c.C, 24, 24)
    assert torch.equal(image_batch(src, size=c.in_hw), image_batch(src))                  # the source's own size: no resize
    out = torch.full((c.B, c.C) + c.out_hw, 7.0).contiguous(memory_format=torch.channels_last)
    res = image_batch(src, size=c.out_hw, channels_last=True, out=out)
    assert res is out and torch.equal(out, got)
    flat = torch.full((c.B * c.C * c.in_hw[0] * c.in_hw[1] + 1,), 7.0)
    view = flat[1:].view((c.B, c.C) + c.in_hw)
    assert image_batch(src, out=view) is view and torch.equal(view, src.float() / 255) and float(flat[0]) == 7.0


def test_host_image_batch_names_every_fault():
    src = torch.zeros(2, 3, 4, 5, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        image_batch(src.float())
    with pytest.raises(TypeError, match="torch.Tensor"):
        image_batch(src.numpy())
    with pytest.raises(TypeError, match="dtype"):
        image_batch(src, dtype=torch.float64)
    with pytest.raises(ValueError, match="4 dimensions"):
        image_batch(src[0])
    with pytest.raises(ValueError, match="not contiguous"):
        image_batch(src.permute(0, 1, 3, 2))
    with pytest.raises(ValueError, match="channels"):
        image_batch(torch.zeros(1, 5, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channels"):
        image_batch(src, src_layout="nhwc")                                               # read as (B,H,W,C): 5 channels
    with pytest.raises(ValueError, match="src_layout"):
        image_batch(src, src_layout="chw")
    with pytest.raises(ValueError, match="size"):
        image_batch(src, size=(0, 4))
    with pytest.raises(ValueError, match="empty"):
        image_batch(torch.zeros(0, 3, 4, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="2\\^31"):
        image_batch(src, size=(1 << 15, 1 << 14))
    with pytest.raises(ValueError, match="shape"):
        image_batch(src, out=torch.zeros(2, 3, 4, 6))
    with pytest.raises(TypeError, match="float16"):
        image_batch(src, out=torch.zeros(2, 3, 4, 5, dtype=torch.float16))
    with pytest.raises(ValueError, match="channels_last"):
        image_batch(src, channels_last=True, out=torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match="contiguous_format"):
        image_batch(src, out=torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
    with pytest.raises(TypeError, match="out must be"):
        image_batch(src, out=[1])


def test_plan_needs_a_device():
    with pytest.raises(ValueError, match="device"):
        IM.ImagePlan.create(2, 3, 4, 5, device="cpu")
    assert sorted(IM.__all__) == sorted(["image_batch", "multi_scale_size", "ImagePlan", "preprocess_batch", "preprocess"])


# ---------------------------------------------------------------------------------------------------------------------------
# install(preprocess=True)
# ---------------------------------------------------------------------------------------------------------------------------
_TRAIN = ("ultralytics.models.yolo.detect.train", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.train")
_VAL = ("ultralytics.models.yolo.detect.val", "mga_yolo.external.ultralytics.ultralytics.models.yolo.detect.val")


@pytest.fixture
def stub_modules():
    """Stand-ins that carry the names of the module objects the reference makes of detect/train.py and detect/val.py; whatever held those
    names before is put back afterwards"""
    before = {}
    for n in _TRAIN + _VAL:
        parts = n.split(".")
        for i in range(1, len(parts) + 1):
            p = ".".join(parts[:i])
            if p not in before:
                before[p] = sys.modules.get(p)
            if i == len(parts) or p not in sys.modules:
                sys.modules[p] = types.ModuleType(p)
    for n in _TRAIN:
        class DetectionTrainer:
            def preprocess_batch(self, batch):
                return "reference"
        sys.modules[n].DetectionTrainer = DetectionTrainer
    for n in _VAL:
        class DetectionValidator:
            def preprocess(self, batch):
                return "reference"
        sys.modules[n].DetectionValidator = DetectionValidator
    yield [sys.modules[n].DetectionTrainer for n in _TRAIN], [sys.modules[n].DetectionValidator for n in _VAL]
    for p, old in before.items():
        if old is None:
            sys.modules.pop(p, None)
        else:
            sys.modules[p] = old


def _self(multi_scale=False, half=False):
    return dict(device=torch.device("cpu"), stride=IC.MULTI_SCALE["stride"],
                args=SimpleNamespace(multi_scale=multi_scale, imgsz=IC.MULTI_SCALE["imgsz"], half=half))


def _labels():
    return dict(batch_idx=torch.zeros(3), cls=torch.zeros(3, 1), bboxes=torch.zeros(3, 4))


def test_install_preprocess_is_opt_in_matches_the_reference_and_uninstall_restores(stub_modules):
    import mga_yolo_amd
    trainers, validators = stub_modules
    originals = [c.__dict__["preprocess_batch"] for c in trainers] + [c.__dict__["preprocess"] for c in validators]

    def bound():
        return [c.__dict__["preprocess_batch"] for c in trainers] + [c.__dict__["preprocess"] for c in validators]
    try:
        mga_yolo_amd.install()
        mga_yolo_amd.install(nms=True, match=True, ap=True)
        assert [c.__dict__["preprocess_batch"] for c in trainers] == originals[:2] and [c.__dict__["preprocess"] for c in validators] == originals[2:]
        mga_yolo_amd.uninstall()
        patched = mga_yolo_amd.install(preprocess=True)
        assert set(_TRAIN + _VAL) <= set(patched)
        assert bound() == [IM.preprocess_batch] * 2 + [IM.preprocess] * 2
        mga_yolo_amd.install(preprocess=True)                                             # a second call rebinds nothing

        for base in trainers:                                                             # MGATrainer's place: through super()
            Sub = type("Sub", (base,), dict(_self(), preprocess_batch=lambda self, batch: super(Sub, self).preprocess_batch(batch)))
            for c in IC.PLAIN:
                z = _load(c.name)
                got = Sub().preprocess_batch({"img": torch.from_numpy(z["src"])})["img"]
                assert torch.equal(got, torch.from_numpy(z["ref_f32"])), c.name
            assert Sub().preprocess_batch({"img": torch.zeros(1, 3, 4, 4)}) == "reference"  # a float img: the method it replaced
            Multi = type("Multi", (base,), _self(multi_scale=True))
            for seed in IC.MULTI_SCALE["seeds"]:
                z = _load(f"ms{seed}")
                random.seed(seed)
                got = Multi().preprocess_batch({"img": torch.from_numpy(z["src"])})["img"]
                # on host bytes the replacement runs torch's own composition at the size the reference drew: this torch's bits of it, and
                # inside the oracle's bars as the recorded output is
                size = tuple(int(s) for s in z["size"])
                assert tuple(got.shape[2:]) == size == tuple(z["ref_f32"].shape[2:])
                assert torch.equal(got, IO.torch_host(torch.from_numpy(z["src"]), size)), seed
                r, _, nonzero, bad = IO.ratio(got, *IO.image(torch.from_numpy(z["src"]), size))
                assert r <= K and nonzero == 0 and bad == 0, (seed, r)
        for base in validators:
            for half, key in ((True, "ref_f16"), (False, "ref_f32")):
                Val = type("Val", (base,), dict(_self(half=half), preprocess=lambda self, batch: super(Val, self).preprocess(batch)))
                for c in IC.PLAIN:
                    z = _load(c.name)
                    lab = _labels()
                    got = Val().preprocess(dict(lab, img=torch.from_numpy(z["src"])))
                    assert torch.equal(got["img"], torch.from_numpy(z[key])), (c.name, key)
                    assert all(got[k] is lab[k] for k in lab)                              # moved to the device they are on: themselves
                assert Val().preprocess(dict(_labels(), img=torch.zeros(1, 3, 4, 4, dtype=torch.float16))) == "reference"
    finally:
        mga_yolo_amd.uninstall()
    assert bound() == originals


def test_install_keeps_its_earlier_keywords():
    import inspect
    import mga_yolo_amd
    p = inspect.signature(mga_yolo_amd.install).parameters
    assert list(p) == ["strict", "nms", "match", "confusion", "ap", "preprocess"] and all(v.default is False for v in p.values())
