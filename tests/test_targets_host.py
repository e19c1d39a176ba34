"""mask_pyramid on CPU tensors (the torch composition of functional.py) against the reference's own results (tests/golden/targets_*.npz,
tools/gen_golden_targets.py), and the argument rules of SlicePlan.create(target_source=...), which are checked on the shapes alone before
anything touches a device.  Every comparison is torch.equal: both methods are integer counts scaled by a power of two."""
import pytest
import torch

import targets_cases as T


@pytest.mark.parametrize("shape", T.SHAPES, ids=T.shape_id)
def test_cpu_path_is_bit_equal_to_every_golden(shape):
    from mga_yolo_amd import mask_pyramid
    meta, z = T.load(shape)
    assert tuple(meta["shape"]) == shape and tuple(meta["patterns"]) == T.PATTERNS
    strides = tuple(meta["strides"])
    assert set(T.MODEL_STRIDES) <= set(strides)
    B, H, W = shape
    n = 0
    for p in T.PATTERNS:
        mask = z[f"mask.{p}"]
        assert mask.shape == shape and mask.dtype == (torch.float32 if p == "f32vals" else torch.uint8)
        for method in T.METHODS:
            # one call per stride list the library knows two paths for, and every stored stride on its own
            for sl in [T.MODEL_STRIDES] + [(s,) for s in strides]:
                got = mask_pyramid(mask, sl, method)
                assert isinstance(got, list) and len(got) == len(sl)
                for s, g in zip(sl, got):
                    want = z[f"{method}.{p}.{s}"]
                    assert g.dtype == torch.float32 and g.shape == want.shape == (B, 1, -(-H // s), -(-W // s))
                    assert torch.equal(g, want), (p, method, s)
                    n += 1
            # and the second oracle agrees with the stored results: the two are interchangeable on the device
            for s, c in zip(strides, T.compose(mask, strides, method)):
                assert torch.equal(c, z[f"{method}.{p}.{s}"]), (p, method, s)
    assert n == len(T.PATTERNS) * 2 * (3 + len(strides))


def test_the_goldens_are_not_trivial():
    _, z = T.load((2, 100, 76))
    avg, mx = z["avgpool.dense.8"], z["maxpool.sparse.8"]
    assert 0.3 < float(avg[..., :12, :9].mean()) < 0.7 and len(avg.unique()) > 10          # interior cells: about half
    assert float(avg[:, :, -1, :].max()) <= 0.5 and float(avg[:, :, :, -1].max()) <= 0.5    # 100 = 12*8 + 4, 76 = 9*8 + 4: padded cells
    assert 0 < float(mx.mean()) < 1 and set(mx.unique().tolist()) == {0.0, 1.0}
    corner = z["avgpool.corner.32"]
    assert corner.shape == (2, 1, 4, 3) and float(corner[0, 0, 3, 2]) == 1.0 / 1024 and float(corner.sum()) == 2.0 / 1024
    assert torch.equal(z["avgpool.f32vals.8"], T.compose((z["mask.f32vals"] > 0).to(torch.uint8), (8,), "avgpool")[0])
    assert float(z["avgpool.one.32"][0, 0, 0, 0]) == 1.0 and float(z["avgpool.one.32"][0, 0, 3, 2]) == (4 * 12) / 1024.0


def test_input_forms_agree_and_out_is_written_in_place():
    from mga_yolo_amd import mask_pyramid
    _, z = T.load((3, 33, 95))
    m3 = z["mask.dense"]
    base = mask_pyramid(m3)
    for form in (m3.unsqueeze(1), m3.float(), m3.float().unsqueeze(1), (m3 * 255), m3.bool(), m3.bool().unsqueeze(1), m3.unsqueeze(1)[:, :, :, :].transpose(0, 1).transpose(0, 1)):
        for a, b in zip(mask_pyramid(form), base):
            assert torch.equal(a, b)
    out = [torch.full(b.shape, -1.0) for b in base]
    ptrs = [o.data_ptr() for o in out]
    ret = mask_pyramid(m3, out=out)
    assert [r.data_ptr() for r in ret] == ptrs and all(torch.equal(r, b) for r, b in zip(ret, base))
    with pytest.raises(ValueError):
        mask_pyramid(m3, out=out[:2])
    with pytest.raises(ValueError):
        mask_pyramid(m3, out=[out[0], out[1], torch.zeros(3, 1, 2, 4)])


def test_bridge_on_cpu_is_the_closing_and_changes_the_result():
    from mga_yolo_amd import mask_pyramid
    m = T.diagonal_mask((2, 100, 76))
    plain, closed = mask_pyramid(m, method="maxpool"), mask_pyramid(m, method="maxpool", bridge=True)
    for c, w in zip(closed, T.compose(m, T.MODEL_STRIDES, "maxpool", bridge=True)):
        assert torch.equal(c, w)
    assert not torch.equal(closed[0], plain[0]) and bool((closed[0] >= plain[0]).all())       # a closing only adds


@pytest.mark.parametrize("kw", [dict(strides=()), dict(strides=(8, 16, 32, 64, 64)), dict(strides=(3,)), dict(strides=(1,)), dict(strides=(128,)),
                                dict(strides=(16, 8)), dict(strides=(8, 8)), dict(method="area"), dict(method="nearest"),
                                dict(method="avgpool", bridge=True)], ids=str)
def test_argument_errors(kw):
    from mga_yolo_amd import mask_pyramid
    with pytest.raises(ValueError):
        mask_pyramid(torch.zeros(1, 16, 16, dtype=torch.uint8), **kw)


def test_wrong_tensors_raise():
    from mga_yolo_amd import mask_pyramid
    for bad in (torch.zeros(16, 16, dtype=torch.uint8), torch.zeros(1, 2, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int64),
                torch.zeros(1, 16, 16, dtype=torch.float16)):
        with pytest.raises(TypeError):
            mask_pyramid(bad)


SHAPES3 = [(4, 16, 16, 16), (4, 32, 8, 8), (4, 64, 4, 4)]


def test_target_strides_are_derived_from_the_sizes():
    from mga_yolo_amd.slice import target_strides
    assert target_strides(SHAPES3, (128, 128)) == (8, 16, 32)
    assert target_strides([(2, 16, 13, 10), (2, 16, 7, 5), (2, 16, 4, 3)], (100, 76)) == (8, 16, 32)        # padded sizes: ceil
    assert target_strides([(1, 8, 68, 68), (1, 8, 34, 34), (1, 8, 17, 17)], (544, 544)) == (8, 16, 32)
    assert target_strides([(1, 8, 32, 24), (1, 8, 2, 2)], (64, 48)) == (2, 32)
    assert target_strides([(1, 8, 1, 1)], (7, 5)) == (8,)                                                    # several fit: the smallest


def _create(shapes=SHAPES3, **kw):
    from mga_yolo_amd import SlicePlan
    return SlicePlan.create(shapes, [8] * len(shapes), [()] * len(shapes), [None] * len(shapes), [{}] * len(shapes), device="cpu", **kw)


@pytest.mark.parametrize("shapes,kw", [
    (SHAPES3, dict(target_source=(128, 96))),                                                  # W asks for 6 / 12 / 24
    ([(4, 16, 16, 8)], dict(target_source=(128, 128))),                                        # H asks for 8, W for 16
    ([(4, 16, 24, 24)], dict(target_source=(128, 128))),                                       # 128 / 24 is no integer
    ([(4, 16, 128, 128)], dict(target_source=(128, 128))),                                     # stride 1
    ([(4, 16, 1, 1)], dict(target_source=(128, 128))),                                         # stride 128
    ([(4, 32, 8, 8), (4, 16, 16, 16)], dict(target_source=(128, 128))),                        # strides 16, 8: descending
    (SHAPES3, dict(target_source=(128, 128), target_hw=[(16, 16), (8, 8), (4, 4)])),           # target_hw is derived
    (SHAPES3, dict(target_source=(128, 128), target_method="area")),
    (SHAPES3, dict(target_source=(128, 128), target_method="avgpool", target_bridge=True)),
    (SHAPES3, dict(target_source=(0, 128))),
    (SHAPES3, dict(target_method="maxpool")), (SHAPES3, dict(target_bridge=True)),             # nothing to apply them to
], ids=lambda v: str(v) if isinstance(v, dict) else "")
def test_slice_plan_target_argument_errors(shapes, kw):
    """raised from the arguments alone: the library is not loaded and no tensor is made (the parameters passed here are placeholders)"""
    with pytest.raises(ValueError):
        _create(shapes, **kw)


def test_unknown_keyword_is_still_a_type_error():
    with pytest.raises(TypeError):
        _create(target_sauce=(128, 128))
