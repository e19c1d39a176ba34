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


# ---- the edge fixtures and the helpers the device tests lean on (tests/targets_cases.py; tests/test_gpu_targets_edges.py)
@pytest.mark.parametrize("shape", T.EDGE_SHAPES, ids=T.shape_id)
def test_cpu_path_and_compose_are_bit_equal_to_every_edge_golden(shape):
    from mga_yolo_amd import mask_pyramid
    meta, z = T.load(shape)
    assert tuple(meta["shape"]) == shape and tuple(meta["patterns"]) == T.EDGE_PATTERNS and tuple(meta["strides"]) == T.ALL_STRIDES
    B, H, W = shape
    n = 0
    for p in T.EDGE_PATTERNS:
        mask = z[f"mask.{p}"]
        assert mask.shape == shape and mask.dtype == (torch.float32 if p in T.F32_PATTERNS else torch.uint8)
        for method in T.METHODS:
            for sl in [T.MODEL_STRIDES, (2, 4, 8, 16)] + [(s,) for s in T.ALL_STRIDES]:
                got = mask_pyramid(mask, sl, method)
                for s, g, c in zip(sl, got, T.compose(mask, sl, method)):
                    want = z[f"{method}.{p}.{s}"]
                    assert g.dtype == torch.float32 and g.shape == want.shape == (B, 1, -(-H // s), -(-W // s))
                    assert torch.equal(g, want), (p, method, s)
                    assert torch.equal(c, want), (p, method, s)
                    n += 1
    assert n == len(T.EDGE_PATTERNS) * 2 * (3 + 4 + 6)


def test_the_edge_patterns_hold_what_they_are_for():
    tiny = float(torch.finfo(torch.float32).tiny)
    for shape in T.EDGE_SHAPES:
        B, H, W = shape
        _, z = T.load(shape)
        # u8all: every byte value; each key byte at each position of an aligned 8-byte word, once among 0x00 and once among 0xff
        u8 = z["mask.u8all"]
        assert W % 8 == 0 and len(u8.unique()) == 256
        words = {tuple(w) for w in u8.reshape(-1, 8).tolist()}
        for k in T.KEY_BYTES:
            for j in range(8):
                for other in (0x00, 0xFF):
                    assert tuple(k if i == j else other for i in range(8)) in words, (shape, k, j, other)
        # f32special: all twelve values, and a plain > 0 on the host flushes none of them
        f = z["mask.f32special"]
        fg = f > 0
        bits = f.view(torch.int32)
        assert len(bits.unique()) == 12 and bool(torch.isnan(f).any())                # twelve bit patterns: +0.0 and -0.0 are two
        assert sorted(f[fg].unique().tolist()) == sorted(torch.tensor([1e-45, 1e-38, tiny, 0.3, 1.0, float("inf")]).tolist())
        assert sorted(f[~fg & ~torch.isnan(f)].unique().tolist()) == sorted(torch.tensor([float("-inf"), -tiny, -1e-45, 0.0]).tolist())
        assert int(((f > 0) & (f < tiny)).sum()) > 0                                  # subnormals, and they are foreground
        assert torch.equal(z["maxpool.f32special.2"], T.compose(fg.to(torch.uint8), (2,), "maxpool")[0])
        # ramp: the 8-counts are the formula, cut where a cell leaves the image (rows only: W % 8 == 0)
        cy, cx = torch.meshgrid(torch.arange(-(-H // 8)), torch.arange(W // 8), indexing="ij")
        want = torch.minimum((cy * 9 + cx * 5) % 65, 8 * (H - 8 * cy).clamp(max=8))
        assert torch.equal(z["avgpool.ramp.8"] * 64, want.float().expand(B, 1, -1, -1))
        quad = want[: 2 * (want.shape[0] // 2), : 2 * (want.shape[1] // 2)].unfold(0, 2, 2).unfold(1, 2, 2).reshape(-1, 4)
        assert all(len(set(q)) == 4 for q in quad.tolist()[:4])                      # the first quads: four different counts
        # lastrow: nothing but the last row and column
        m = z["mask.lastrow"]
        assert int(m.sum()) == B * (H + W - 1) and bool(m[:, H - 1, :].all()) and bool(m[:, :, W - 1].all())


def _seam_levels():
    """every (shape, stride) the device tests close: the levels of (2, 70, 136), one 1 x 1 level and one 1 x 17 level"""
    return [((2, 70, 136), s) for s in (2, 4, 8, 16, 32)] + [((1, 7, 5), 8), ((2, 5, 133), 8)]


def test_seam_masks_closed_forms_agree_with_the_loops_and_the_composition():
    names = set()
    for shape, s in _seam_levels():
        for name, mask, closed, seam in T.seam_masks(shape, s):
            names.add(name)
            unclosed = T.compose(mask, (s,), "maxpool")[0]
            assert torch.equal(T.close3_loops(unclosed), closed), (shape, s, name)
            assert torch.equal(T.compose(mask, (s,), "maxpool", bridge=True)[0], closed), (shape, s, name)
            assert int(mask.sum()) == int(unclosed.sum())                                  # one pixel per chosen cell
            if seam is not None:                                                           # a filled gap: the closing changed the seam cell itself
                assert float(unclosed[0, 0, seam[0], seam[1]]) == 0.0 and float(closed[0, 0, seam[0], seam[1]]) == 1.0, (shape, s, name)
            elif name[0] in "hvd":                                                         # a gap of three, a diagonal: the seam cell stays empty
                k, oh, ow = int(name[1:3]), closed.shape[2], closed.shape[3]
                cell = {"h": (oh // 2, k), "v": (k, ow // 2), "d": (k, k)}[name[0]]
                assert float(closed[0, 0, cell[0], cell[1]]) == 0.0, (shape, s, name)
            elif name == "corners" and min(closed.shape[2:]) >= 5:
                assert torch.equal(unclosed, closed), (shape, s, name)                     # each stays single: three cells or more between two
    # the 35 x 68 level has every case; gaps of one and two are filled, a gap of three is not
    want = {f"{d}{s}gap{g}" for d in "hv" for s in (16, 32) for g in (1, 2, 3)} | {"d16", "q16", "d32", "q32", "corners", "ones", "hole"}
    assert names == want and {c[0] for c in T.seam_masks((2, 70, 136), 2)} == want
    assert [c[0] for c in T.seam_masks((1, 7, 5), 8)] == ["corners", "ones"]


def test_close3_loops_agrees_with_the_composition_and_the_cpu_path_on_random_masks():
    from mga_yolo_amd import mask_pyramid
    for shape in T.EDGE_SHAPES:
        m = T.random_mask(shape)
        strides = (2, 4, 8, 16)
        unclosed = T.compose(m, strides, "maxpool")
        closed = T.compose(m, strides, "maxpool", bridge=True)
        for u, c, g in zip(unclosed, closed, mask_pyramid(m, strides, "maxpool", bridge=True)):
            assert torch.equal(T.close3_loops(u), c) and torch.equal(g, c)
        assert not torch.equal(unclosed[0], closed[0])
