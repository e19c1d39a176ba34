"""The eager frame (mga_yolo_amd/functional.py: _forward_tables / _backward_tables) builds the level tables of all four block families from
what each family DECLARES: the names of a level's inputs and of its saved tensors.  These tests drive that table-building half on host
tensors (data_ptr() works on them, nothing is launched) with a three-level call -- level 0's mask requires grad, level 1's does not and is
channels_last, level 2 has no mask; the mask head has no mask and varies `training` and num_batches_tracked=None instead -- and compare
EVERY field of every forward and backward level with the tensors passed (test_binding_fill's `_check`: a field the test does not name fails
it).  A slot declaration and a fill that disagree fail here."""
import pytest
import torch

from test_binding_fill import HID, K, _check, _ptr, _t, bind  # noqa: F401  (bind: that module's fixture)

SHAPES = [(2, 16, 3, 5), (3, 32, 4, 6), (1, 16, 5, 3)]          # B, C, H, W all different within a level
NHWC_LEVEL = 1
SP_HID = 32
f32 = torch.float32


def _feature(shape, dtype, l):
    x = _t(*shape, dtype=dtype)
    return x.contiguous(memory_format=torch.channels_last) if l == NHWC_LEVEL else x


def _masks():
    """level 0: requires grad; level 1: does not; level 2: none"""
    return [_t(SHAPES[0][0], 1, *SHAPES[0][2:]).requires_grad_(True), _t(SHAPES[1][0], 1, *SHAPES[1][2:]), None]


def _a16(v):
    return (v + 15) & ~15


def _run(F, blk, cfgs, flat):
    """Both table builders, as _BlockFn drives them -> everything they return, and per level the tensors by the names the family declares"""
    needs = (False,) * len(F._LEAD) + tuple(isinstance(t, torch.Tensor) and t.requires_grad for t in flat)
    fwd, outs, keep, kept, hold = F._forward_tables(blk, cfgs, flat, want_grad=any(needs), stream=7)
    assert len(keep) == len(cfgs) * blk.n_saved and len(outs) == len(kept) == len(hold) == len(cfgs)
    gys = [torch.zeros_like(y) for y in outs]
    bwd, grads, hold_b = F._backward_tables(blk, kept, keep, gys, needs)
    n_lead = len(F._LEAD)
    assert len(grads) == n_lead + len(flat) and grads[:n_lead] == [None] * n_lead        # cfgs / state first: no gradient
    levels = []
    for l in range(len(cfgs)):
        saved = dict(zip(blk.saved_names, keep[l * blk.n_saved:(l + 1) * blk.n_saved]))
        back = blk.unpack(keep[l * blk.n_saved:(l + 1) * blk.n_saved])                   # the frame's own way back: by the declared names
        assert set(back) == {"mask", *blk.saved} and all(p is q for p, q in zip(blk.pack(back), saved.values()))
        g = dict(zip(blk.input_names, grads[n_lead + l * blk.slots:n_lead + (l + 1) * blk.slots]))
        inp = dict(zip(blk.input_names, flat[l * blk.slots:(l + 1) * blk.slots]))
        assert hold_b[2 * l] is gys[l]                                                   # already in x's layout and element type
        levels.append(dict(inp=inp, saved=saved, g=g, y=outs[l], ws=hold[l], gy=gys[l], scratch=hold_b[2 * l + 1], kept=kept[l]))
    return fwd, bwd, levels


def _dims(x, code, flags):
    B, C, H, W = x.shape
    return dict(B=B, C=C, H=H, W=W, dtype=code, flags=flags)


def _check_block_grads(lv, params, mask, want_gmask, buffers=()):
    """One gradient per input slot: None exactly for the buffers, an absent / unwanted mask and the parameters a mask-less level does not read"""
    g = lv["g"]
    assert g["x"].shape == lv["inp"]["x"].shape and g["x"].dtype == lv["inp"]["x"].dtype
    assert (g["mask"] is not None) == want_gmask
    for n in buffers:
        assert g[n] is None
    for n, p in params.items():
        assert (g[n] is None) == (p is None) and (p is None or (g[n].shape == p.shape and g[n].dtype == f32))


def test_cbam_tables(bind):  # noqa: F811
    bd, _lib = bind
    from mga_yolo_amd import BlockConfig, functional as F
    blk, names = F._CBAM, bd.CBAM.param_names
    cfgs = tuple(BlockConfig(hidden=HID + l, k=K - 2 * l, use_sigmoid_mask=bool(l), tiny_thr=3e-4, eps=2e-6) for l in range(3))
    masks, flat, per = _masks(), [], []
    for l, (shp, cfg) in enumerate(zip(SHAPES, cfgs)):
        C, h, k = shp[1], cfg.hidden, cfg.k
        ps = [_t(h, C), _t(h), _t(C, h), _t(C), _t(1, 3, k, k), _t(1).reshape(())]
        x = _feature(shp, torch.float16, l)
        per.append((x, masks[l], ps))
        flat += [x, masks[l], *ps]
    assert blk.input_names == ("x", "mask", *names) and blk.saved_names == blk.input_names and F.SLOTS == len(blk.input_names)
    fwd, bwd, levels = _run(F, blk, cfgs, flat)
    for l, (lv, (x, mask, ps), cfg) in enumerate(zip(levels, per, cfgs)):
        flags = _lib.LAYOUT_NHWC if l == NHWC_LEVEL else 0
        lease = lv["kept"][4]
        assert [_ptr(t) for t in lv["saved"].values()] == [_ptr(x), _ptr(mask), *map(_ptr, ps)]
        assert lease.key == (None, 7, *x.shape, cfg.hidden, x.dtype, _lib.ENV_EPOCH, cfg.k) + ((flags,) if flags else ())
        assert lease.buf.numel() == _lib.ctx_bytes(*x.shape, cfg.hidden)
        assert (lv["ws"] is not None) == bool(flags) and (not flags or lv["ws"].numel() == _lib.fwd_ws_bytes(*x.shape, cfg.hidden, flags))
        assert lv["y"].shape == x.shape and lv["y"].stride() == x.stride() and lv["g"]["x"].stride() == x.stride()
        P = dict(zip(names, map(_ptr, ps)), hidden=cfg.hidden, k=cfg.k, use_sigmoid_mask=int(cfg.use_sigmoid_mask), tiny_thr=3e-4, eps=2e-6)
        dims = _dims(x, _lib.F16, flags)
        _check(fwd[l].p, P)
        _check(fwd[l], dict(x=_ptr(x), mask=_ptr(mask), y=_ptr(lv["y"]), ctx=_ptr(lease.buf), ctx_bytes=lease.buf.numel(), p=fwd[l].p,
                            ws=_ptr(lv["ws"]), ws_bytes=0 if lv["ws"] is None else lv["ws"].numel(), **dims))
        want_gmask = l == 0
        _check_block_grads(lv, dict(zip(names, ps)), mask, want_gmask)
        assert lv["scratch"].numel() == _lib.scratch_bytes(*x.shape, cfg.hidden, cfg.k, flags)
        _check(bwd[l].p, P)
        _check(bwd[l], dict(x=_ptr(x), mask=_ptr(mask), gy=_ptr(lv["gy"]), ctx=_ptr(lease.buf), scratch=_ptr(lv["scratch"]),
                            ctx_bytes=lease.buf.numel(), scratch_bytes=lv["scratch"].numel(), gx=_ptr(lv["g"]["x"]),
                            gmask=_ptr(lv["g"]["mask"]), p=bwd[l].p, **dims, **{"g" + n: _ptr(lv["g"][n]) for n in names}))
        assert (bwd[l].gmask is not None) == want_gmask
    del fwd, bwd, levels, lease, lv
    F._POOL.clear()                                                  # the host buffers the leases gave back


def test_eca_tables(bind):  # noqa: F811
    bd, _lib = bind
    from mga_yolo_amd import EcaConfig, functional as F
    blk, names = F._ECA, bd.ECA.param_names
    cfgs = tuple(EcaConfig(k=K - 2 * l, use_sigmoid_mask=bool(l), tiny_thr=3e-4, eps=2e-6) for l in range(3))
    masks, flat, per = _masks(), [], []
    for l, (shp, cfg) in enumerate(zip(SHAPES, cfgs)):
        x, ps = _feature(shp, torch.bfloat16, l), [_t(1, 1, cfg.k), _t(1).reshape(())]
        per.append((x, masks[l], ps))
        flat += [x, masks[l], *ps]
    assert blk.input_names == ("x", "mask", *names) and blk.saved_names == ("x", "mask", "ctx", *names)
    fwd, bwd, levels = _run(F, blk, cfgs, flat)
    for l, (lv, (x, mask, ps), cfg) in enumerate(zip(levels, per, cfgs)):
        flags = _lib.LAYOUT_NHWC if l == NHWC_LEVEL else 0
        ctx = lv["saved"]["ctx"]
        assert [_ptr(lv["saved"][n]) for n in ("x", "mask", *names)] == [_ptr(x), _ptr(mask), *map(_ptr, ps)]
        assert ctx.numel() == _lib.eca_ctx_bytes(*x.shape, flags) and lv["ws"] is None and lv["kept"][4] is None
        assert lv["y"].stride() == x.stride() and lv["g"]["x"].stride() == x.stride()
        P = dict(w=_ptr(ps[0]), beta=_ptr(ps[1]), k=cfg.k, use_sigmoid_mask=int(cfg.use_sigmoid_mask), tiny_thr=3e-4, eps=2e-6)
        dims = _dims(x, _lib.BF16, flags)
        _check(fwd[l].p, P)
        _check(fwd[l], dict(x=_ptr(x), mask=_ptr(mask), y=_ptr(lv["y"]), ctx=_ptr(ctx), ctx_bytes=ctx.numel(), p=fwd[l].p, **dims))
        want_gmask = l == 0
        _check_block_grads(lv, dict(zip(names, ps)), mask, want_gmask)
        assert lv["scratch"].numel() == _lib.eca_scratch_bytes(*x.shape, flags)
        _check(bwd[l].p, P)
        _check(bwd[l], dict(x=_ptr(x), mask=_ptr(mask), gy=_ptr(lv["gy"]), ctx=_ptr(ctx), scratch=_ptr(lv["scratch"]), ctx_bytes=ctx.numel(),
                            scratch_bytes=lv["scratch"].numel(), gx=_ptr(lv["g"]["x"]), gmask=_ptr(lv["g"]["mask"]),
                            gw=_ptr(lv["g"][names[0]]), gbeta=_ptr(lv["g"][names[1]]), p=bwd[l].p, **dims))
        assert (bwd[l].gmask is not None) == want_gmask


def test_head_tables(bind):  # noqa: F811
    bd, _lib = bind
    from mga_yolo_amd import functional as F
    blk, names = F._HEAD, bd.HEAD.param_names
    state, flat, per = [], [], []
    for l, shp in enumerate(SHAPES):
        C, hid = shp[1], HID + l
        ps = [_t(hid, C, 1, 1), _t(hid), _t(hid), _t(1, hid, 3, 3), _t(1)]
        rm, rv, nbt = _t(hid), _t(hid), (torch.zeros((), dtype=torch.int64) if l == 0 else None)
        st = (rm, rv, nbt, 1e-3 * (l + 1), 0.03 * (l + 1), l != 1)                     # training, eval, training without a batch counter
        x = _feature(shp, f32, l)
        state.append(st); per.append((x, ps, st, hid)); flat += [x, *ps]
    assert blk.input_names == ("x", *names) and blk.saved_names == ("x", "ctx", *names, "running_mean", "running_var")
    fwd, bwd, levels = _run(F, blk, tuple(state), flat)
    for l, (lv, (x, ps, (rm, rv, nbt, eps, mom, training), hid)) in enumerate(zip(levels, per)):
        flags = _lib.HEAD_LAYOUT_NHWC if l == NHWC_LEVEL else 0
        ctx = lv["saved"]["ctx"]
        assert [_ptr(lv["saved"][n]) for n in ("x", *names, "running_mean", "running_var")] == [_ptr(x), *map(_ptr, ps), _ptr(rm), _ptr(rv)]
        assert ctx.numel() == _lib.head_ctx_bytes(*x.shape, hid, flags) and lv["ws"] is None
        Bx, _, Hx, Wx = x.shape
        assert lv["y"].shape == (Bx, 1, Hx, Wx) and lv["y"].dtype == x.dtype and lv["y"].is_contiguous() and lv["g"]["x"].stride() == x.stride()
        P = dict(w1=_ptr(ps[0]), bn_weight=_ptr(ps[1]), bn_bias=_ptr(ps[2]), running_mean=_ptr(rm), running_var=_ptr(rv),
                 num_batches_tracked=_ptr(nbt), wh=_ptr(ps[3]), bh=_ptr(ps[4]), hidden=hid, eps=eps, momentum=mom, training=int(training))
        dims = _dims(x, _lib.F32, flags)
        _check(fwd[l].p, P)
        _check(fwd[l], dict(x=_ptr(x), logits=_ptr(lv["y"]), ctx=_ptr(ctx), ctx_bytes=ctx.numel(), p=fwd[l].p, **dims))
        for n, p in zip(names, ps):                                                       # every input of the head takes a gradient
            assert lv["g"][n].shape == p.shape and lv["g"][n].dtype == f32
        assert lv["g"]["x"].shape == x.shape and lv["scratch"].numel() == _lib.head_scratch_bytes(*x.shape, hid, flags)
        _check(bwd[l].p, dict(P, num_batches_tracked=0))                                  # the backward never counts a batch
        _check(bwd[l], dict(x=_ptr(x), g_logits=_ptr(lv["gy"]), g_logits2=0, ctx=_ptr(ctx), scratch=_ptr(lv["scratch"]), ctx_bytes=ctx.numel(),
                            scratch_bytes=lv["scratch"].numel(), gx=_ptr(lv["g"]["x"]), p=bwd[l].p, **dims,
                            **dict(zip(("gw1", "gbn_weight", "gbn_bias", "gwh", "gbh"), (_ptr(lv["g"][n]) for n in names)))))


@pytest.mark.parametrize("norm", ["in", "bn"])
def test_spade_tables(bind, norm):  # noqa: F811
    bd, _lib = bind
    from mga_yolo_amd import SpadeConfig, functional as F
    blk, names = F._SPADE, bd.SPADE.param_names
    buffers = ("running_mean", "running_var", "num_batches_tracked")
    cfgs = tuple(SpadeConfig(hidden=SP_HID, norm_type=norm, use_sigmoid_mask=bool(l), eps=2e-6 * (l + 1), momentum=0.03, training=l != 1)
                 for l in range(3))
    masks, flat, per = _masks(), [], []
    for l, shp in enumerate(SHAPES):
        C = shp[1]
        ps = [_t(*s) for s in [(SP_HID, 1, 3, 3), (SP_HID,), (C, SP_HID, 3, 3), (C,), (C, SP_HID, 3, 3), (C,)]]
        run = (_t(C), _t(C), torch.zeros((), dtype=torch.int64))       # handed over for 'in' too, as mask_spade does: not read then
        x = _feature(shp, torch.float16, l)
        per.append((x, masks[l], ps, run))
        flat += [x, masks[l], *ps, *run]
    assert blk.input_names == ("x", "mask", *names, *buffers) and blk.saved_names == ("x", "mask", "ctx", *names)
    fwd, bwd, levels = _run(F, blk, cfgs, flat)
    bn, short = norm == "bn", ("w0", "b0", "wg", "bg", "wb", "bb")
    for l, (lv, (x, mask, ps, run), cfg) in enumerate(zip(levels, per, cfgs)):
        flags = _lib.SPADE_LAYOUT_NHWC if l == NHWC_LEVEL else 0
        read = ps if mask is not None else [None] * len(ps)                               # a level without a mask reads no parameter
        ctx = lv["saved"]["ctx"]
        assert [_ptr(lv["saved"][n]) for n in ("x", "mask", *names)] == [_ptr(x), _ptr(mask), *map(_ptr, read)]
        # the eager ctx: the full size keeps gamma as fp32; here it is kept in x's element type, and only where a backward will read it
        full = _lib.spade_ctx_bytes(*x.shape, SP_HID)
        assert ctx.numel() == full - _a16(x.numel() * 4) + (_a16(x.numel() * x.element_size()) if mask is not None else 0)
        assert lv["y"].stride() == x.stride() and lv["g"]["x"].stride() == x.stride() and lv["ws"] is None
        common = dict(x=_ptr(x), mask=_ptr(mask), ctx=_ptr(ctx), ctx_bytes=ctx.numel(), hidden=SP_HID, **_dims(x, _lib.F16, flags),
                      norm_type=_lib.NORM_BN if bn else _lib.NORM_IN, training=int(cfg.training), use_sigmoid_mask=int(cfg.use_sigmoid_mask),
                      eps=cfg.eps, momentum=0.03, running_mean=_ptr(run[0]) if bn else 0, running_var=_ptr(run[1]) if bn else 0,
                      num_batches_tracked=_ptr(run[2]) if bn else 0, **dict(zip(short, map(_ptr, read))))
        none = dict.fromkeys(("y", "gy", "gx", "gmask", "scratch", "scratch_bytes", "save_gamma") + tuple("g" + n for n in short), 0)
        _check(fwd[l], dict(none, **common, y=_ptr(lv["y"]), save_gamma=int(mask is not None)))
        want_gmask = l == 0
        _check_block_grads(lv, dict(zip(names, read)), mask, want_gmask, buffers)
        assert lv["scratch"].numel() == _lib.spade_scratch_bytes(*x.shape, SP_HID)
        _check(bwd[l], dict(none, **common, gy=_ptr(lv["gy"]), gx=_ptr(lv["g"]["x"]), gmask=_ptr(lv["g"]["mask"]), scratch=_ptr(lv["scratch"]),
                            scratch_bytes=lv["scratch"].numel(), **{"g" + s: _ptr(lv["g"][n]) for s, n in zip(short, names)}))
        assert (bwd[l].gmask is not None) == want_gmask


def test_spade_keeps_no_gamma_without_a_backward(bind):  # noqa: F811
    """want_grad -> save_gamma: with nothing requiring grad the forward keeps no gamma, and ctx is the smaller for it"""
    bd, _lib = bind
    from mga_yolo_amd import SpadeConfig, functional as F
    shp = SHAPES[0]
    C = shp[1]
    x, mask = _t(*shp), _t(shp[0], 1, *shp[2:])
    ps = [_t(*s) for s in [(SP_HID, 1, 3, 3), (SP_HID,), (C, SP_HID, 3, 3), (C,), (C, SP_HID, 3, 3), (C,)]]
    fwd, _, keep, _, _ = F._forward_tables(F._SPADE, (SpadeConfig(hidden=SP_HID),), [x, mask, *ps, None, None, None], want_grad=False)
    ctx = dict(zip(F._SPADE.saved_names, keep))["ctx"]
    assert fwd[0].save_gamma == 0 and ctx.numel() == _lib.spade_ctx_bytes(*shp, SP_HID) - _a16(x.numel() * 4)
