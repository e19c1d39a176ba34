"""Every C-ABI level struct is filled in ONE place, mga_yolo_amd/_binding.py.  These tests build each level from host tensors (data_ptr()
works on them, nothing is launched) and compare EVERY field with what was passed: pointers against data_ptr(), None against 0, shapes,
the dtype code, the flags and the nested parameter struct's scalars.  B, C, H, W, hidden and k are all different, so a swapped pair of
arguments cannot cancel.  A field the test does not name fails it (`_check`): a new field must be added here too."""
import ctypes as C

import pytest
import torch

B, CH, H, W, HID, K = 2, 16, 3, 5, 4, 7
HT, WT = 11, 13
f32 = torch.float32


def _t(*shape, dtype=f32):
    return torch.zeros(*shape, dtype=dtype)


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check(struct, want: dict):
    """Every field of `struct` is in `want` and equals it (c_void_p reads back None for NULL; floats are compared as c_float)."""
    names = [n for n, _ in struct._fields_]
    assert sorted(names) == sorted(want), sorted(set(names) ^ set(want))
    for n, ctype in struct._fields_:
        got = getattr(struct, n)
        if issubclass(ctype, C.Structure):                     # the nested parameter struct: checked field by field by the caller
            continue
        if ctype is C.c_void_p:
            got = got or 0
        elif ctype is C.c_float:
            assert got == C.c_float(want[n]).value, n
            continue
        assert got == want[n], (n, got, want[n])


def _distinct(*tensors):
    ptrs = [t.data_ptr() for t in tensors if t is not None]
    assert len(set(ptrs)) == len(ptrs) and 0 not in ptrs


@pytest.fixture(scope="module")
def bind(built_lib):
    from mga_yolo_amd import _binding, _lib
    return _binding, _lib


@pytest.mark.parametrize("dtype,code", [(torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2)])
def test_one_dtype_table(bind, dtype, code):
    bd, _lib = bind
    from mga_yolo_amd import functional, segloss
    assert bd.DTYPES[dtype] == code and len(bd.DTYPES) == 3
    assert functional._DTYPES is bd.DTYPES and segloss.DTYPES is bd.DTYPES


@pytest.mark.parametrize("with_mask", [True, False])
def test_cbam_levels(bind, with_mask):
    bd, _lib = bind
    from mga_yolo_amd import BlockConfig
    cfg = BlockConfig(hidden=HID, k=K, use_sigmoid_mask=False, tiny_thr=3e-4, eps=2e-6)
    x, y, gy, gx = (_t(B, CH, H, W, dtype=torch.float16) for _ in range(4))
    mask, gmask = (_t(B, 1, H, W), _t(B, 1, H, W)) if with_mask else (None, None)
    params = [_t(HID, CH), _t(HID), _t(CH, HID), _t(CH), _t(1, 3, K, K), _t(1).reshape(())]
    pg = [torch.zeros_like(p) for p in params]
    ctx, scratch, ws = _t(96, dtype=torch.uint8), _t(160, dtype=torch.uint8), _t(224, dtype=torch.uint8)
    _distinct(x, y, gy, gx, mask, gmask, ctx, scratch, ws, *params, *pg)
    P = dict(zip(("w1", "b1", "w2", "b2", "wsa", "beta"), map(_ptr, params)), hidden=HID, k=K, use_sigmoid_mask=0, tiny_thr=3e-4, eps=2e-6)
    dims = dict(B=B, C=CH, H=H, W=W, dtype=_lib.F16)

    L = _lib.FwdLevel()
    flags = _lib.LAYOUT_NHWC | _lib.FWD_SAVE_PROJ
    bd.fill_cbam_fwd(L, x, mask, y, ctx, params, cfg, flags, ws)
    _check(L.p, P)
    _check(L, dict(x=_ptr(x), mask=_ptr(mask), y=_ptr(y), ctx=_ptr(ctx), ctx_bytes=96, p=L.p, flags=flags, ws=_ptr(ws), ws_bytes=224, **dims))
    bd.fill_cbam_fwd(L, x, mask, y, ctx, params, cfg)                  # refilling a used level: the defaults clear what the first call set
    assert (L.flags, L.ws, L.ws_bytes) == (0, None, 0)

    Lb = _lib.BwdLevel()
    bd.fill_cbam_bwd(Lb, x, mask, gy, ctx, scratch, gx, gmask, pg, params, cfg, _lib.BWD_HAVE_PROJ)
    _check(Lb.p, P)
    _check(Lb, dict(x=_ptr(x), mask=_ptr(mask), gy=_ptr(gy), ctx=_ptr(ctx), scratch=_ptr(scratch), ctx_bytes=96, scratch_bytes=160,
                    gx=_ptr(gx), gmask=_ptr(gmask), p=Lb.p, flags=_lib.BWD_HAVE_PROJ, **dims,
                    **dict(zip(("gw1", "gb1", "gw2", "gb2", "gwsa", "gbeta"), map(_ptr, pg)))))


@pytest.mark.parametrize("with_mask", [True, False])
def test_eca_levels(bind, with_mask):
    bd, _lib = bind
    from mga_yolo_amd import EcaConfig
    cfg = EcaConfig(k=K, use_sigmoid_mask=True, tiny_thr=3e-4, eps=2e-6)
    x, y, gy, gx = (_t(B, CH, H, W, dtype=torch.bfloat16) for _ in range(4))
    mask, gmask = (_t(B, 1, H, W), _t(B, 1, H, W)) if with_mask else (None, None)
    w, beta, gw, gb = _t(1, 1, K), _t(1).reshape(()), _t(1, 1, K), _t(1).reshape(())
    ctx, scratch = _t(96, dtype=torch.uint8), _t(160, dtype=torch.uint8)
    _distinct(x, y, gy, gx, mask, gmask, w, beta, gw, gb, ctx, scratch)
    P = dict(w=_ptr(w), beta=_ptr(beta), k=K, use_sigmoid_mask=1, tiny_thr=3e-4, eps=2e-6)
    dims = dict(B=B, C=CH, H=H, W=W, dtype=_lib.BF16, flags=_lib.LAYOUT_NHWC)

    L = _lib.EcaFwdLevel()
    bd.fill_eca_fwd(L, x, mask, y, ctx, w, beta, cfg, _lib.LAYOUT_NHWC)
    _check(L.p, P)
    _check(L, dict(x=_ptr(x), mask=_ptr(mask), y=_ptr(y), ctx=_ptr(ctx), ctx_bytes=96, p=L.p, **dims))

    Lb = _lib.EcaBwdLevel()
    bd.fill_eca_bwd(Lb, x, mask, gy, ctx, scratch, gx, gmask, gw, gb, w, beta, cfg, _lib.LAYOUT_NHWC)
    _check(Lb.p, P)
    _check(Lb, dict(x=_ptr(x), mask=_ptr(mask), gy=_ptr(gy), ctx=_ptr(ctx), scratch=_ptr(scratch), ctx_bytes=96, scratch_bytes=160,
                    gx=_ptr(gx), gmask=_ptr(gmask), gw=_ptr(gw), gbeta=_ptr(gb), p=Lb.p, **dims))
    bd.fill_eca_bwd(Lb, x, mask, gy, ctx, scratch, gx, gmask, gw, gb, w, beta, cfg)
    assert Lb.flags == 0


@pytest.mark.parametrize("with_second", [True, False])
def test_head_levels(bind, with_second):
    bd, _lib = bind
    x, gx = _t(B, CH, H, W), _t(B, CH, H, W)
    logits, gl = _t(B, 1, H, W), _t(B, 1, H, W)
    gl2 = _t(B, 1, H, W) if with_second else None
    params = [_t(HID, CH, 1, 1), _t(HID), _t(HID), _t(1, HID, 3, 3), _t(1)]
    pg = [torch.zeros_like(p) for p in params]
    rm, rv, nbt = _t(HID), _t(HID), torch.zeros((), dtype=torch.int64)
    ctx, scratch = _t(96, dtype=torch.uint8), _t(160, dtype=torch.uint8)
    _distinct(x, gx, logits, gl, gl2, rm, rv, nbt, ctx, scratch, *params, *pg)
    w1, gamma, beta, wh, bh = params
    P = dict(w1=_ptr(w1), bn_weight=_ptr(gamma), bn_bias=_ptr(beta), running_mean=_ptr(rm), running_var=_ptr(rv),
             num_batches_tracked=_ptr(nbt), wh=_ptr(wh), bh=_ptr(bh), hidden=HID, eps=1e-3, momentum=0.03, training=1)
    dims = dict(B=B, C=CH, H=H, W=W, dtype=_lib.F32)

    L = _lib.HeadFwdLevel()
    bd.fill_head_fwd(L, x, logits, ctx, params, (rm, rv, nbt), HID, 1e-3, 0.03, True, _lib.HEAD_LOGITS_F32)
    _check(L.p, P)
    _check(L, dict(x=_ptr(x), logits=_ptr(logits), ctx=_ptr(ctx), ctx_bytes=96, p=L.p, flags=_lib.HEAD_LOGITS_F32, **dims))
    bd.fill_head_fwd(L, x, logits, ctx, params, (rm, rv, None), HID, 1e-3, 0.03, False)
    _check(L.p, dict(P, num_batches_tracked=0, training=0))
    assert L.flags == 0

    Lb = _lib.HeadBwdLevel()
    flags = _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32
    bd.fill_head_bwd(Lb, x, gl, gl2, ctx, scratch, gx, pg, params, (rm, rv, nbt), HID, 1e-3, 0.03, True, flags)
    _check(Lb.p, dict(P, num_batches_tracked=0))               # the backward never counts a batch
    _check(Lb, dict(x=_ptr(x), g_logits=_ptr(gl), g_logits2=_ptr(gl2), ctx=_ptr(ctx), scratch=_ptr(scratch), ctx_bytes=96, scratch_bytes=160,
                    gx=_ptr(gx), p=Lb.p, flags=flags, **dims,
                    **dict(zip(("gw1", "gbn_weight", "gbn_bias", "gwh", "gbh"), map(_ptr, pg)))))
    # functional._head_params is the same function (tests/test_gpu_head_channels_last.py fills its levels by hand with it)
    from mga_yolo_amd import functional
    _check(functional._head_params(w1, gamma, beta, rm, rv, nbt, wh, bh, HID, 1e-3, 0.03, True), P)


@pytest.mark.parametrize("with_grad", [True, False])
def test_seg_level(bind, with_grad):
    bd, _lib = bind
    logits, target = _t(B, 1, H, W, dtype=torch.float16), _t(B, 1, HT, WT)
    g = torch.zeros_like(logits) if with_grad else None
    _distinct(logits, target, g)
    L = _lib.SegLevel()
    bd.fill_seg(L, logits, target, g, 0.75, _lib.SEG_BILINEAR)
    _check(L, dict(logits=_ptr(logits), target=_ptr(target), glogits=_ptr(g), B=B, H=H, W=W, Ht=HT, Wt=WT, dtype=_lib.F16,
                   scale_weight=0.75, resize=_lib.SEG_BILINEAR))


@pytest.mark.parametrize("norm,with_mask", [("in", True), ("bn", True), ("bn", False)])
def test_spade_level_both_directions(bind, norm, with_mask):
    bd, _lib = bind
    from mga_yolo_amd import SpadeConfig
    hid = 32
    cfg = SpadeConfig(hidden=hid, norm_type=norm, use_sigmoid_mask=False, eps=2e-6, momentum=0.03, training=True)
    x, y, gy, gx = (_t(B, CH, H, W, dtype=torch.float16) for _ in range(4))
    mask, gmask = (_t(B, 1, H, W), _t(B, 1, H, W)) if with_mask else (None, None)
    shapes = [(hid, 1, 3, 3), (hid,), (CH, hid, 3, 3), (CH,), (CH, hid, 3, 3), (CH,)]
    params = [_t(*s) for s in shapes] if with_mask else [None] * 6
    pg = [_t(*s) for s in shapes] if with_mask else [None] * 6
    running = (_t(CH), _t(CH), torch.zeros((), dtype=torch.int64))      # handed over for 'in' too, as the Function does: not read then
    ctx, scratch = _t(96, dtype=torch.uint8), _t(160, dtype=torch.uint8)
    _distinct(x, y, gy, gx, mask, gmask, ctx, scratch, *running, *params, *pg)
    bn = norm == "bn"
    names = ("w0", "b0", "wg", "bg", "wb", "bb")
    common = dict(x=_ptr(x), mask=_ptr(mask), ctx=_ptr(ctx), ctx_bytes=96, B=B, C=CH, H=H, W=W, hidden=hid, dtype=_lib.F16,
                  norm_type=_lib.NORM_BN if bn else _lib.NORM_IN, training=1, use_sigmoid_mask=0, eps=2e-6, momentum=0.03, flags=0,
                  running_mean=_ptr(running[0]) if bn else 0, running_var=_ptr(running[1]) if bn else 0,
                  num_batches_tracked=_ptr(running[2]) if bn else 0, **dict(zip(names, map(_ptr, params))))
    none = dict.fromkeys(("y", "gy", "gx", "gmask", "scratch", "scratch_bytes", "save_gamma") + tuple("g" + n for n in names), 0)

    L = _lib.SpadeLevel()
    bd.fill_spade(L, x, mask, params, cfg, running, ctx, gy=gy, gx=gx, gmask=gmask, pgrads=pg, scratch=scratch)
    _check(L, dict(none, **common, gy=_ptr(gy), gx=_ptr(gx), gmask=_ptr(gmask), scratch=_ptr(scratch), scratch_bytes=160,
                   **dict(zip(("g" + n for n in names), map(_ptr, pg)))))
    bd.fill_spade(L, x, mask, params, cfg, running, ctx, y=y, save_gamma=with_mask)        # the same level refilled for a forward
    _check(L, dict(none, **common, y=_ptr(y), save_gamma=int(with_mask)))


def test_size_queries_go_through_one_cached_helper(bind):
    bd, _lib = bind
    lib = _lib.load()
    _lib.reload_env()
    assert _lib._size_cache == {}
    s = (B, CH, H, W, HID)
    NH, HNH = _lib.LAYOUT_NHWC, _lib.HEAD_LAYOUT_NHWC
    want = {
        ("mgacbam_ctx_bytes", *s): _lib.ctx_bytes(*s),
        ("mgacbam_bwd_scratch_bytes_flags", *s, K, 0): _lib.scratch_bytes(*s, K),
        ("mgacbam_bwd_scratch_bytes_flags", *s, K, NH): _lib.scratch_bytes(*s, K, NH | _lib.BWD_HAVE_PROJ),
        ("mgacbam_fwd_ws_bytes", *s, NH): _lib.fwd_ws_bytes(*s, NH | _lib.FWD_SAVE_PROJ),
        ("mgacbam_eca_ctx_bytes_flags", *s[:4], NH): _lib.eca_ctx_bytes(*s[:4], NH),
        ("mgacbam_eca_scratch_bytes_flags", *s[:4], 0): _lib.eca_scratch_bytes(*s[:4]),
        ("mgahead_ctx_bytes_flags", *s, 0): _lib.head_ctx_bytes(*s, _lib.HEAD_LOGITS_F32),
        ("mgahead_bwd_scratch_bytes_flags", *s, HNH): _lib.head_scratch_bytes(*s, HNH | _lib.HEAD_BWD_ACCUM_GX),
        ("mgaspade_ctx_bytes", B, CH, H, W, 32): _lib.spade_ctx_bytes(B, CH, H, W, 32),
        ("mgaspade_scratch_bytes", B, CH, H, W, 32): _lib.spade_scratch_bytes(B, CH, H, W, 32),
    }
    assert _lib.fwd_ws_bytes(*s, 0) == 0                                   # NCHW levels have no forward workspace: nothing is asked
    assert _lib._size_cache == want
    for (symbol, *ints), n in want.items():
        assert n == getattr(lib, symbol)(*ints) > 0
    with pytest.raises(RuntimeError, match="mgacbam_bwd_scratch_bytes_flags: argument error -2"):
        _lib.scratch_bytes(1, 8, 8, 8, 1, 4)                               # even k: 0 from the library is E_SHAPE, and is not cached
    with pytest.raises(RuntimeError, match="mgahead_ctx_bytes_flags: argument error -2"):
        _lib.head_ctx_bytes(1, 8, 2, 501, 8)
    five = (_lib.SegLevel * 5)()
    with pytest.raises(RuntimeError, match="mgaseg_ws_bytes: argument error -2"):
        _lib.seg_ws_bytes(five, 5)
    assert _lib._size_cache == want
    _lib.reload_env()
    assert _lib._size_cache == {}
