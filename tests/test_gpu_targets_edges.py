"""mask_pyramid on device tensors at the edges its first tests leave out (tests/test_gpu_targets.py): a ragged bottom row under the wide loads,
every byte value, fp32 specials, a last workgroup with one live wave, destinations that are 4-byte aligned and no more, and the closing across
the seams of its 16 x 16 tiles.  Every result is written into tests/targets_cases.guarded_outs -- NaN where the call has to write, NaN
sentinels around it -- so a cell the kernel skips and a cell it writes outside its level both show; every comparison is torch.equal against
the reference's stored result (tests/golden/targets_*.npz) and against the torch composition."""
import pytest
import torch

import targets_cases as T

pytestmark = pytest.mark.gpu

CELL_LISTS = ((2, 4, 8, 16), (4, 64))                              # k_tgt_cells
STRIDE_LISTS = (T.MODEL_STRIDES, (8,), (8, 16)) + CELL_LISTS       # k_tgt_pool with three, one and two levels first


def _run(src, strides, method, bridge=False):
    """mask_pyramid into guarded destinations -> the levels on the host, after the sentinels were checked"""
    from mga_yolo_amd import mask_pyramid
    from mga_yolo_amd.functional import target_pyramid_shapes
    B, H, W = src.shape[0], src.shape[-2], src.shape[-1]
    outs, check = T.guarded_outs(target_pyramid_shapes(B, H, W, strides), src.device)
    ret = mask_pyramid(src, strides, method, bridge, out=outs)
    assert all(r is o for r, o in zip(ret, outs))
    check()
    return [o.cpu() for o in outs]


def _both_types(stored):
    """a uint8 pattern also as fp32 (the same values), an fp32 pattern also as its uint8 binarisation"""
    return [stored, stored.float()] if stored.dtype == torch.uint8 else [stored, (stored > 0).to(torch.uint8)]


@pytest.mark.parametrize("shape", T.EDGE_SHAPES, ids=T.shape_id)
def test_every_edge_pattern_method_type_and_stride_list_equals_the_reference(built_lib, shape):
    _, z = T.load(shape)
    n = 0
    for p in T.EDGE_PATTERNS:
        stored = z[f"mask.{p}"]
        want_c = {(m, sl): T.compose(stored, sl, m) for m in T.METHODS for sl in STRIDE_LISTS}
        for src in _both_types(stored):
            d = src.cuda()
            for method in T.METHODS:
                for sl in STRIDE_LISTS:
                    for s, g, c in zip(sl, _run(d, sl, method), want_c[method, sl]):
                        assert torch.equal(g, z[f"{method}.{p}.{s}"]), (p, src.dtype, method, sl, s)
                        assert torch.equal(g, c), (p, src.dtype, method, sl, s)
                        n += 1
    assert n == len(T.EDGE_PATTERNS) * 2 * 2 * (3 + 1 + 2 + 4 + 2)


@pytest.mark.parametrize("align", [16, 0], ids=["wide", "element"])
@pytest.mark.parametrize("shape", T.EDGE_SHAPES, ids=T.shape_id)
def test_a_source_with_foreground_all_around_it(built_lib, shape, align):
    """the last sample's ragged bottom cells lie against foreground that is not the mask's: rows read past a sample would count"""
    _, z = T.load(shape)
    n = 0
    for p in ("dense", "lastrow", "u8all"):
        for src in _both_types(z[f"mask.{p}"]):
            view = T.guarded_src(src, "cuda", align)
            assert torch.equal(view.cpu(), src)
            for method in T.METHODS:
                for sl in (T.MODEL_STRIDES, (2, 4, 8, 16)):
                    for s, g in zip(sl, _run(view, sl, method)):
                        assert torch.equal(g, z[f"{method}.{p}.{s}"]), (p, src.dtype, method, s)
                        n += 1
    assert n == 3 * 2 * 2 * 7


@pytest.mark.parametrize("shape", T.SHAPES, ids=T.shape_id)
def test_the_first_goldens_into_guarded_destinations(built_lib, shape):
    _, z = T.load(shape)
    for p in ("dense", "corner"):
        stored = z[f"mask.{p}"]
        for src in _both_types(stored):
            for method in T.METHODS:
                got = _run(src.cuda(), T.MODEL_STRIDES, method)
                for s, g, c in zip(T.MODEL_STRIDES, got, T.compose(stored, T.MODEL_STRIDES, method)):
                    assert torch.equal(g, z[f"{method}.{p}.{s}"]) and torch.equal(g, c), (p, src.dtype, method, s)


def _close(src, strides):
    """One closing call built by hand: NaN in every destination, around them and in the whole scratch, run twice from that state -> the
    levels on the host.  A cell of scratch the pooling skips, or that the closing reads past a level, is a NaN in the result."""
    from mga_yolo_amd.functional import TargetPyramidCall, target_pyramid_shapes
    B, H, W = src.shape
    outs, check = T.guarded_outs(target_pyramid_shapes(B, H, W, strides), src.device)
    call = TargetPyramidCall(src, outs, strides, "maxpool", True)
    assert call.launches == 2 and call.scratch.numel() >= 4 * sum(o.numel() for o in outs)
    runs = []
    for _ in range(2):
        call.scratch.fill_(0xFF)                                   # 0xffffffff: a NaN
        for o in outs:
            o.fill_(float("nan"))
        call.run()
        check()
        runs.append([o.cpu() for o in outs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    return runs[0]


@pytest.mark.parametrize("strides", [(2, 4, 8, 16), (8, 16, 32)], ids=str)
def test_the_closing_across_its_tile_seams(built_lib, strides):
    """(2, 70, 136): levels of 35 x 68, 18 x 34, 9 x 17, 5 x 9 and 3 x 5 cells; four levels reach TgtCloseArgs.start[4]"""
    shape = (2, 70, 136)
    n = 0
    for s in strides:
        for name, mask, closed, _ in T.seam_masks(shape, s):
            want = T.compose(mask, strides, "maxpool", bridge=True)
            assert torch.equal(want[strides.index(s)], closed)
            for src in (mask, mask.float()):
                got = _close(src.cuda(), strides)
                assert torch.equal(got[strides.index(s)], closed), (s, name, src.dtype)
                for g, w in zip(got, want):
                    assert torch.equal(g, w), (s, name, src.dtype)
                n += 1
    # 35 x 68: 12 gaps, 4 diagonals; 18 x 34: 5 + 2 gaps, 2 diagonals; the smaller levels have no seam with a cell on either side; 3 more each
    assert n == 2 * {(2, 4, 8, 16): 19 + 12 + 3 + 3, (8, 16, 32): 3 + 3 + 3}[strides]


@pytest.mark.parametrize("shape", [(2, 70, 136), (1, 7, 5), (2, 5, 133)], ids=T.shape_id)
def test_the_closing_of_full_empty_random_and_one_cell_high_levels(built_lib, shape):
    """(1, 7, 5): every level is 1 x 1; (2, 5, 133): 1 x 17 at stride 8, a second tile of one column.  An all-ones level stays all ones:
    what lies outside a level is ignored by the erosion."""
    masks = dict(one=torch.ones(shape, dtype=torch.uint8), zero=torch.zeros(shape, dtype=torch.uint8), random=T.random_mask(shape))
    for strides in [(2, 4, 8, 16), (8, 16, 32), (8,)]:
        for name, mask in masks.items():
            want = T.compose(mask, strides, "maxpool", bridge=True)
            if name in ("one", "zero"):
                assert all(bool((w == (name == "one")).all()) for w in want)
            for src in (mask, mask.float()):
                for g, w in zip(_close(src.cuda(), strides), want):
                    assert torch.equal(g, w), (strides, name, src.dtype)
    if shape == (2, 70, 136):
        m = masks["random"]
        assert not torch.equal(T.compose(m, (2,), "maxpool")[0], T.compose(m, (2,), "maxpool", bridge=True)[0])
    for s in (8,):
        for name, mask, closed, _ in T.seam_masks(shape, s):
            assert torch.equal(_close(mask.cuda(), (s,))[0], closed), (s, name)


def test_input_forms_on_the_device(built_lib):
    shape = (3, 61, 128)
    B, H, W = shape
    _, z = T.load(shape)
    m = z["mask.dense"]
    d = m.cuda()
    wider = torch.full((B, H + 3, W + 24), 1, dtype=torch.uint8, device="cuda")              # foreground around the crop
    wider[:, 2:2 + H, 8:8 + W] = d
    crop = wider[:, 2:2 + H, 8:8 + W]
    fwider = wider.float()
    fcrop = fwider[:, 2:2 + H, 8:8 + W]
    assert not crop.is_contiguous() and not fcrop.is_contiguous()
    forms = dict(bool=d.bool(), bool4=d.bool().unsqueeze(1), u8_4=d.unsqueeze(1), f32_4=d.float().unsqueeze(1), crop=crop, fcrop=fcrop,
                 crop4=crop.unsqueeze(1), times255=d * 255, transposed=d.transpose(1, 2).contiguous().transpose(1, 2))
    assert forms["times255"].dtype == torch.uint8 and int(forms["times255"].max()) == 255 and not forms["transposed"].is_contiguous()
    for method in T.METHODS:
        for sl in (T.MODEL_STRIDES, (2, 4, 8, 16)):
            base = _run(d, sl, method)
            for s, b in zip(sl, base):
                assert torch.equal(b, z[f"{method}.dense.{s}"])
            for name, form in forms.items():
                for a, b in zip(_run(form, sl, method), base):
                    assert torch.equal(a, b), (name, method, sl)
