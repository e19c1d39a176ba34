"""mask_pyramid on device tensors (include/mgatargets.h: k_tgt_pool, k_tgt_cells, k_tgt_close3) against the reference's stored results and
the torch composition (tests/targets_cases.py).  Every comparison is torch.equal: the kernels count integers.

Shapes (tests/golden/targets_*.npz): one cell; smaller than a cell; exactly one 64 x 64 wave tile; partial tiles on both axes; padding at
every stride with W % 8 == 4 (the uint8 element-load path, the fp32 16-byte path with a half cell); odd W (element loads for both types);
the 544 x 544 letterbox size (81 wave tiles)."""
import pytest
import torch

import targets_cases as T

pytestmark = pytest.mark.gpu


def _dev(t):
    return t.cuda()


@pytest.mark.parametrize("shape", T.SHAPES, ids=T.shape_id)
def test_every_pattern_method_and_source_type_equals_the_reference(built_lib, shape):
    from mga_yolo_amd import mask_pyramid
    meta, z = T.load(shape)
    n = 0
    for p in T.PATTERNS:
        stored = z[f"mask.{p}"]
        # uint8 patterns also run as fp32 (the same values), the fp32 pattern also as its uint8 binarisation
        sources = [stored, stored.float()] if stored.dtype == torch.uint8 else [stored, (stored > 0).to(torch.uint8)]
        for src in sources:
            d = _dev(src)
            for method in T.METHODS:
                got = mask_pyramid(d, T.MODEL_STRIDES, method)
                want_c = T.compose(src, T.MODEL_STRIDES, method)
                for s, g, c in zip(T.MODEL_STRIDES, got, want_c):
                    assert g.is_cuda and g.dtype == torch.float32 and g.shape == c.shape
                    g = g.cpu()
                    assert torch.equal(g, z[f"{method}.{p}.{s}"]), (p, src.dtype, method, s)
                    assert torch.equal(g, c), (p, src.dtype, method, s)
                    n += 1
    assert n == len(T.PATTERNS) * 2 * 2 * 3


@pytest.mark.parametrize("shape", [(2, 64, 64), (2, 100, 76), (3, 33, 95)], ids=T.shape_id)
def test_offset_view_takes_the_element_loads_and_agrees(built_lib, shape):
    from mga_yolo_amd import mask_pyramid
    _, z = T.load(shape)
    B, H, W = shape
    n = B * H * W
    for p in ("dense", "u8vals"):
        m = z[f"mask.{p}"]
        aligned = _dev(m)
        assert aligned.data_ptr() % 16 == 0
        buf = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda")          # foreground all around: a read outside the view would count
        view = buf[3:3 + n].view(B, H, W)
        view.copy_(aligned)
        assert view.data_ptr() % 8 == 3 and view.is_contiguous()
        fbuf = torch.full((n + 8,), 7.0, device="cuda")
        fview = fbuf[1:1 + n].view(B, H, W)                                       # fp32: 4-byte aligned only
        fview.copy_(aligned)
        assert fview.data_ptr() % 16 == 4
        for method in T.METHODS:
            base = mask_pyramid(aligned, T.MODEL_STRIDES, method)
            for other in (view, fview):
                for a, b in zip(mask_pyramid(other, T.MODEL_STRIDES, method), base):
                    assert torch.equal(a, b), (p, method, other.dtype)
            for b, s in zip(base, T.MODEL_STRIDES):
                assert torch.equal(b.cpu(), z[f"{method}.{p}.{s}"])


@pytest.mark.parametrize("strides", [(8,), (8, 16), (4, 8, 16), (2, 64), (16, 32), (2, 4, 8, 16)], ids=str)
def test_other_stride_lists(built_lib, strides):
    """prefixes of the chain (k_tgt_pool with fewer levels) and lists outside it (k_tgt_cells: one thread per destination cell)"""
    from mga_yolo_amd import mask_pyramid
    for shape in [(2, 100, 76), (3, 33, 95), (1, 7, 5), (2, 72, 136)]:
        _, z = T.load(shape)
        for p in ("dense", "corner", "f32vals"):
            src = z[f"mask.{p}"]
            for method in T.METHODS:
                got = mask_pyramid(_dev(src), strides, method)
                assert len(got) == len(strides)
                for s, g in zip(strides, got):
                    assert torch.equal(g.cpu(), z[f"{method}.{p}.{s}"]), (shape, p, method, s)


def test_out_buffers_are_written_in_place(built_lib):
    from mga_yolo_amd import mask_pyramid
    _, z = T.load((2, 72, 136))
    src = _dev(z["mask.sparse"])
    out = [torch.full((2, 1, -(-72 // s), -(-136 // s)), -1.0, device="cuda") for s in T.MODEL_STRIDES]
    ptrs = [o.data_ptr() for o in out]
    ret = mask_pyramid(src, out=out)
    assert [r.data_ptr() for r in ret] == ptrs and all(r is o for r, o in zip(ret, out))
    for o, s in zip(out, T.MODEL_STRIDES):
        assert torch.equal(o.cpu(), z[f"avgpool.sparse.{s}"])
    # (B,1,H,W) and (B,H,W) sources agree; a second call overwrites the same buffers
    mask_pyramid(_dev(z["mask.dense"]).unsqueeze(1), method="maxpool", out=out)
    for o, s in zip(out, T.MODEL_STRIDES):
        assert torch.equal(o.cpu(), z[f"maxpool.dense.{s}"])
    with pytest.raises(ValueError):
        mask_pyramid(src, out=[o.cpu() for o in out])


@pytest.mark.parametrize("shape", [(2, 100, 76), (2, 64, 64)], ids=T.shape_id)
def test_bridge_is_the_closing_of_every_level(built_lib, shape):
    from mga_yolo_amd import mask_pyramid
    m = T.diagonal_mask(shape)
    d = _dev(m)
    plain = mask_pyramid(d, method="maxpool")
    for src in (d, d.float()):
        closed = mask_pyramid(src, method="maxpool", bridge=True)
        for c, w in zip(closed, T.compose(m, T.MODEL_STRIDES, "maxpool", bridge=True)):
            assert torch.equal(c.cpu(), w)
        assert not torch.equal(closed[0], plain[0])                      # the closing filled something in
    for pl, w in zip(plain, T.compose(m, T.MODEL_STRIDES, "maxpool")):
        assert torch.equal(pl.cpu(), w)
    # more than one 16 x 16 closing tile per level, through the other pooling kernel: stride 2 of 100 x 76 is 50 x 38 cells
    dense = (torch.rand(shape, generator=torch.Generator().manual_seed(3)) < 0.08).to(torch.uint8)
    got = mask_pyramid(_dev(dense), (2, 4), "maxpool", bridge=True)
    want = T.compose(dense, (2, 4), "maxpool", bridge=True)
    unclosed = T.compose(dense, (2, 4), "maxpool")
    for g, w, u in zip(got, want, unclosed):
        assert torch.equal(g.cpu(), w) and not torch.equal(w, u)
