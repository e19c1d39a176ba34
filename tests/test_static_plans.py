"""The static plans of every block in both feature layouts (mga_yolo_amd/plan.py, slice.py), built on the host: the size queries are host
code and nothing is launched, so bucket layouts, level tables, flags, buffer sizes and refusals are all checked without a GPU.  And the
mask resample's entry points (include/mgaresample.h): every argument error, each returned before a launch (the header against the binding
is tests/test_abi_headers.py's).  PyramidPlan, EcaPyramidPlan and SlicePlan take the new options through ``create`` -- their constructors' argument lists
are pinned by tests/test_gate_abi.py and tests/test_abi_eca_nhwc.py and stay as they are."""
import pytest
import torch

from abi_header import FAKE as P

SHAPES = [(4, 64, 16, 16), (4, 128, 8, 8), (4, 256, 4, 4)]
HIDDEN = [16, 32, 64]
CL = torch.channels_last


def _modules(block, shapes=SHAPES):
    """-> (per-level block parameters, per-level configs, per-level running buffers | None) of freshly built modules"""
    from mga_yolo_amd import MaskCBAM, MaskECA, MaskSPADE
    torch.manual_seed(0)
    if block == "cbam":
        ms = [MaskCBAM(c) for _, c, _, _ in shapes]
        return [m.block_params() for m in ms], [m.block_config() for m in ms], None
    if block == "eca":
        ms = [MaskECA(c) for _, c, _, _ in shapes]
        return [(m.conv1d.weight, m.beta) for m in ms], [m.eca_config() for m in ms], None
    ms = [MaskSPADE(c, hidden=h, norm_type="bn" if l == 1 else "in") for l, ((_, c, _, _), h) in enumerate(zip(shapes, HIDDEN))]
    running = [(m.norm.running_mean, m.norm.running_var, m.norm.num_batches_tracked) if l == 1 else None for l, m in enumerate(ms)]
    return [m.spade_params() for m in ms], [m.spade_config() for m in ms], running


def _head_states(shapes=SHAPES):
    from mga_yolo_amd import MGAMaskHead
    torch.manual_seed(1)
    return [MGAMaskHead(c, h).state_dict() for (_, c, _, _), h in zip(shapes, HIDDEN)]


def _pyramid(block, **kw):
    from mga_yolo_amd import EcaPyramidPlan, PyramidPlan, SpadePyramidPlan
    params, cfgs, running = _modules(block)
    if block == "cbam":
        return PyramidPlan.create(SHAPES, params, cfgs, device="cpu", **kw), params
    if block == "eca":
        return EcaPyramidPlan.create(SHAPES, params, cfgs, device="cpu", **kw), params
    return SpadePyramidPlan(SHAPES, params, cfgs, device="cpu", running=running, **kw), params


def _assert_views(bucket, views, params, start=0):
    """every view aliases `bucket` at the running offset, in the order and shape of `params`; returns the offset after them"""
    off = start
    for lv, ps in zip(views, params):
        assert len(lv) == len(ps)
        for v, p in zip(lv, ps):
            assert v.shape == p.shape and v.dtype == torch.float32
            assert v.data_ptr() == bucket.data_ptr() + 4 * off, off
            off += p.numel()
    return off


# ---------------------------------------------------------------------------------------------------------------- bucket
@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_pyramid_plan_bucket(built_lib, block):
    plan, params = _pyramid(block)
    n = sum(p.numel() for ps in params for p in ps)
    assert plan.grad_bucket.numel() == n and plan.grad_bucket.dtype == torch.float32
    assert _assert_views(plan.grad_bucket, plan.param_grads, params) == n
    assert list(plan.named_param_grads(1).values())[0].data_ptr() == plan.param_grads[1][0].data_ptr()
    assert len(plan.named_param_grads(0)) == len(params[0]) and plan.images() == 4
    assert plan.elements() == sum(b * c * h * w for b, c, h, w in SHAPES)
    # a caller's slice of a larger bucket is used as it is; a wrong size or element type is refused
    big = torch.zeros(n + 7)
    mine, _ = _pyramid(block, grad_bucket=big[3:3 + n])
    assert mine.grad_bucket.data_ptr() == big.data_ptr() + 12 and mine.param_grads[0][0].data_ptr() == big.data_ptr() + 12
    with pytest.raises(AssertionError):
        _pyramid(block, grad_bucket=torch.zeros(n + 1))
    with pytest.raises(AssertionError):
        _pyramid(block, grad_bucket=torch.zeros(n, dtype=torch.float64))


@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_slice_plan_bucket(built_lib, block):
    from mga_yolo_amd import SlicePlan
    from mga_yolo_amd.slice import HEAD_PARAM_NAMES
    params, cfgs, running = _modules(block)
    hs = _head_states()
    plan = SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, block=block, block_running=running, device="cpu")
    n_block = sum(p.numel() for ps in params for p in ps)
    heads = [[sd[k] for k in HEAD_PARAM_NAMES] for sd in hs]
    n_head = sum(p.numel() for ps in heads for p in ps)
    assert plan.grad_bucket.numel() == n_block + n_head + 2                      # [block grads][head grads][log_vars]
    assert plan.block.grad_bucket.data_ptr() == plan.grad_bucket.data_ptr() and plan.block.grad_bucket.numel() == n_block
    off = _assert_views(plan.grad_bucket, plan.block.param_grads, params)
    off = _assert_views(plan.grad_bucket, plan.head_grads, heads, off)
    assert off == n_block + n_head and plan.g_log_vars.data_ptr() == plan.grad_bucket.data_ptr() + 4 * off
    assert (plan.cbam is plan.block) if block == "cbam" else not hasattr(plan, "cbam")
    # the block's dL/dmask buffer is the heads' second dL/dlogits, and the heads write the block's mask input
    for l in range(3):
        assert plan._hb[l].g_logits2 == plan.block.gmask[l].data_ptr() and plan._hf[l].logits == plan.block.mask[l].data_ptr()
        assert plan._seg[l].logits == plan.block.mask[l].data_ptr()


def test_slice_plan_constructor_is_the_cbam_nchw_plan(built_lib):
    """SlicePlan(...) as every caller writes it today builds what create(block="cbam") builds"""
    from mga_yolo_amd import SlicePlan, _lib
    params, cfgs, _ = _modules("cbam")
    plan = SlicePlan(SHAPES, HIDDEN, params, cfgs, _head_states(), device="cpu")
    assert plan.block_name == "cbam" and plan.cbam is plan.block and not plan.channels_last and plan.target_resize == "nearest"
    assert plan._seg[0].resize == _lib.SEG_NEAREST and plan._hf[0].flags == _lib.HEAD_LOGITS_F32 and plan.block._fwd[0].flags == 0
    assert plan.launches() == dict(forward="3 (heads) + 2 (MaskCBAM) + 2 (seg loss + Kendall)",
                                   backward="1 (seg loss + Kendall) + 2 (MaskCBAM) + 5 (heads)")


# ---------------------------------------------------------------------------------------------------------------- one base
@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_pyramid_plans_share_one_base(built_lib, block):
    """one set-up for the three plans: a subclass brings its library calls, and defines none of what the base owns a second time"""
    from mga_yolo_amd import plan as P
    plan, _ = _pyramid(block)
    cls = type(plan)
    assert isinstance(plan, P._BlockPlan) and cls.__mro__[1] is P._BlockPlan and plan.kind == block
    for name in ("x", "mask", "y", "gy", "gx", "gmask", "ctx", "scratch", "params", "param_grads", "cfgs", "shapes", "_fwd", "_bwd"):
        assert len(getattr(plan, name)) == plan.n == 3, name
    assert len(plan.running) == 3 and all(len(run) == 3 for run in plan.running)
    assert [run[0] is not None for run in plan.running] == [False, block == "spade", False]          # the batch-norm level of _modules
    assert len(plan.param_names) == len(plan.grad_names) == len(plan.params[0])
    for name in ("forward", "backward", "launch_counts"):
        assert name in vars(cls), name
    for name in ("capture", "elements", "images", "named_param_grads", "_stream", "_call"):
        assert name not in vars(cls) and callable(getattr(plan, name)), name
    from mga_yolo_amd import SlicePlan
    assert SlicePlan.capture is P._BlockPlan.capture and SlicePlan._call is P._BlockPlan._call and "images" not in vars(SlicePlan)


_HEAD_SEGMENTS = [f"head{l}.{n}" for l in range(3) for n in ("proj.0.weight", "proj.1.weight", "proj.1.bias", "head.weight", "head.bias")]
_HEAD_EMA_SEGMENTS = ["head0.proj.1.running_mean", "head0.proj.1.running_var", "head1.proj.1.running_mean", "head1.proj.1.running_var",
                      "head2.proj.1.running_mean", "head2.proj.1.running_var"]
_BLOCK_SEGMENTS = dict(
    cbam=["block0.cam_mlp.0.weight", "block0.cam_mlp.0.bias", "block0.cam_mlp.2.weight", "block0.cam_mlp.2.bias", "block0.sam_conv.weight", "block0.beta",
          "block1.cam_mlp.0.weight", "block1.cam_mlp.0.bias", "block1.cam_mlp.2.weight", "block1.cam_mlp.2.bias", "block1.sam_conv.weight", "block1.beta",
          "block2.cam_mlp.0.weight", "block2.cam_mlp.0.bias", "block2.cam_mlp.2.weight", "block2.cam_mlp.2.bias", "block2.sam_conv.weight", "block2.beta"],
    eca=["block0.conv1d.weight", "block0.beta", "block1.conv1d.weight", "block1.beta", "block2.conv1d.weight", "block2.beta"],
    spade=["block0.shared.0.weight", "block0.shared.0.bias", "block0.conv_gamma.weight", "block0.conv_gamma.bias", "block0.conv_beta.weight", "block0.conv_beta.bias",
           "block1.shared.0.weight", "block1.shared.0.bias", "block1.conv_gamma.weight", "block1.conv_gamma.bias", "block1.conv_beta.weight", "block1.conv_beta.bias",
           "block2.shared.0.weight", "block2.shared.0.bias", "block2.conv_gamma.weight", "block2.conv_gamma.bias", "block2.conv_beta.weight", "block2.conv_beta.bias"])
_BLOCK_EMA_SEGMENTS = dict(cbam=[], eca=[], spade=["block1.norm.running_mean", "block1.norm.running_var"])       # the batch-norm level of _modules


@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_segment_order(built_lib, block):
    """The names and the order of optim.plan_segments for SHAPES, as recorded before the plans shared a base: optimizer state and checkpoints
    are keyed and laid out by them.  [block, level by level][heads, level by level][mtl_log_vars][the block's averaged buffers][the heads']."""
    from mga_yolo_amd import SlicePlan
    from mga_yolo_amd.optim import plan_segments
    plan, params = _pyramid(block)
    assert [s.name for s in plan_segments(plan)] == _BLOCK_SEGMENTS[block] + _BLOCK_EMA_SEGMENTS[block]
    _, cfgs, running = _modules(block)
    sp = SlicePlan.create(SHAPES, HIDDEN, params, cfgs, _head_states(), block=block, block_running=running, device="cpu")
    assert [s.name for s in plan_segments(sp)] == (_BLOCK_SEGMENTS[block] + _HEAD_SEGMENTS + ["mtl_log_vars"] + _BLOCK_EMA_SEGMENTS[block]
                                                   + _HEAD_EMA_SEGMENTS)
    with pytest.raises(TypeError, match="none of the static plans"):
        plan_segments(object())


# ---------------------------------------------------------------------------------------------------------------- flags and sizes
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_layout_flag_and_buffer_sizes(built_lib, block, channels_last):
    from mga_yolo_amd import _lib
    plan, _ = _pyramid(block, channels_last=channels_last)
    flag = (_lib.SPADE_LAYOUT_NHWC if block == "spade" else _lib.LAYOUT_NHWC) if channels_last else 0
    assert plan.channels_last == channels_last
    for l, (B, Cc, H, W) in enumerate(SHAPES):
        assert plan._fwd[l].flags == flag and plan._bwd[l].flags == flag
        for t in (plan.x[l], plan.y[l], plan.gy[l], plan.gx[l]):
            assert tuple(t.shape) == (B, Cc, H, W) and t.is_contiguous(memory_format=CL if channels_last else torch.contiguous_format)
            assert t.data_ptr() in (plan._fwd[l].x, plan._fwd[l].y, plan._bwd[l].gy, plan._bwd[l].gx)
        for t in (plan.mask[l], plan.gmask[l]):
            assert tuple(t.shape) == (B, 1, H, W) and t.is_contiguous() and t.dtype == torch.float32
        cfg = plan.cfgs[l]
        if block == "cbam":
            want = (_lib.ctx_bytes(B, Cc, H, W, cfg.hidden), _lib.scratch_bytes(B, Cc, H, W, cfg.hidden, cfg.k, flag))
            ws = _lib.fwd_ws_bytes(B, Cc, H, W, cfg.hidden, flag)
            assert (plan._fwd[l].ws_bytes, plan._fwd[l].ws) == ((ws, plan.ws[l].data_ptr()) if channels_last else (0, None))
            assert (plan.ws[l].numel() == ws > 0) if channels_last else plan.ws[l] is None
        elif block == "eca":
            want = (_lib.eca_ctx_bytes(B, Cc, H, W, flag), _lib.eca_scratch_bytes(B, Cc, H, W, flag))
        else:
            want = (_lib.spade_ctx_bytes(B, Cc, H, W, cfg.hidden), _lib.spade_scratch_bytes(B, Cc, H, W, cfg.hidden))
            assert plan._fwd[l].save_gamma == 1 and plan._fwd[l].ctx_bytes == want[0]
        assert (plan.ctx[l].numel(), plan.scratch[l].numel()) == want == (plan._bwd[l].ctx_bytes, plan._bwd[l].scratch_bytes)


@pytest.mark.parametrize("channels_last", [False, True])
def test_slice_plan_head_tables_carry_the_layout(built_lib, channels_last):
    from mga_yolo_amd import SlicePlan, _lib
    params, cfgs, running = _modules("spade")
    plan = SlicePlan.create(SHAPES, HIDDEN, params, cfgs, _head_states(), block="spade", block_running=running, channels_last=channels_last,
                            target_resize="bilinear", device="cpu")
    hfl = _lib.HEAD_LAYOUT_NHWC if channels_last else 0
    for l, (B, Cc, H, W) in enumerate(SHAPES):
        assert plan._hf[l].flags == hfl | _lib.HEAD_LOGITS_F32
        assert plan._hb[l].flags == hfl | _lib.HEAD_BWD_ACCUM_GX | _lib.HEAD_LOGITS_F32
        assert plan.head_ctx[l].numel() == _lib.head_ctx_bytes(B, Cc, H, W, HIDDEN[l], hfl) == plan._hf[l].ctx_bytes
        assert plan.head_scratch[l].numel() == _lib.head_scratch_bytes(B, Cc, H, W, HIDDEN[l], hfl) == plan._hb[l].scratch_bytes
        assert tuple(plan.logits[l].shape) == (B, 1, H, W) and plan.logits[l].is_contiguous()
        assert plan.x[l].is_contiguous(memory_format=CL if channels_last else torch.contiguous_format)
        assert plan._seg[l].resize == _lib.SEG_BILINEAR
        assert plan.block._fwd[l].flags == (_lib.SPADE_LAYOUT_NHWC if channels_last else 0)
    # batch norm's buffers of the middle level are the plan's own copies, the kernels' in-place targets
    rm, rv, nbt = plan.block.running[1]
    assert plan.block._fwd[1].running_mean == rm.data_ptr() and plan.block._fwd[1].num_batches_tracked == nbt.data_ptr()
    assert rm.data_ptr() != running[1][0].data_ptr() and nbt.dtype == torch.int64 and plan.block.running[0] == (None, None, None)


def test_spade_plan_running_defaults_and_mask_sources(built_lib):
    from mga_yolo_amd import SpadePyramidPlan
    params, cfgs, _ = _modules("spade")
    plan = SpadePyramidPlan(SHAPES, params, cfgs, device="cpu", mask_hw=[(10, 6), None, (16, 12)])
    rm, rv, nbt = plan.running[1]
    assert torch.equal(rm, torch.zeros(128)) and torch.equal(rv, torch.ones(128)) and int(nbt) == 0
    assert [None if m is None else tuple(m.shape) for m in plan.mask_src] == [(4, 1, 10, 6), None, (4, 1, 16, 12)]
    assert [None if m is None else tuple(m.shape) for m in plan.gmask_src] == [(4, 1, 10, 6), None, (4, 1, 16, 12)]
    f, b = plan._rs_fwd, plan._rs_bwd
    assert plan._n_rs == plan._n_rs_bwd == 2
    assert (f[0].src, f[0].dst, f[0].B, f[0].in_h, f[0].in_w, f[0].out_h, f[0].out_w) == (plan.mask_src[0].data_ptr(), plan.mask[0].data_ptr(), 4, 10, 6, 16, 16)
    assert (b[1].src, b[1].dst, b[1].B, b[1].in_h, b[1].in_w, b[1].out_h, b[1].out_w) == (plan.gmask[2].data_ptr(), plan.gmask_src[2].data_ptr(), 4, 16, 12, 4, 4)
    nog = SpadePyramidPlan(SHAPES, params, cfgs, device="cpu", mask_hw=[(10, 6), None, None], want_gmask=False)
    assert nog._n_rs == 1 and nog._n_rs_bwd == 0 and nog.gmask_src == [None] * 3 and nog.gmask == [None] * 3


def test_launch_counts(built_lib):
    """What SlicePlan.launches() reports, against the launches csrc/api_eca.hip, api_spade.hip, api_fwd.hip and api_bwd.hip enqueue per group"""
    from mga_yolo_amd import SlicePlan
    hs = _head_states()

    def of(block, cl):
        params, cfgs, running = _modules(block)
        return SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, block=block, channels_last=cl, block_running=running, device="cpu").launches()
    assert of("eca", False) == dict(forward="3 (heads) + 2 (MaskECA) + 2 (seg loss + Kendall)", backward="1 (seg loss + Kendall) + 2 (MaskECA) + 5 (heads)")
    assert of("eca", True) == dict(forward="3 (heads) + 3 (MaskECA) + 2 (seg loss + Kendall)", backward="1 (seg loss + Kendall) + 3 (MaskECA) + 5 (heads)")
    # MaskSPADE: statistics, pack, conv + FiLM; backward reduce, fin, dW, dW fin, dh, dW0 fin, dL/dmask, apply
    assert of("spade", False) == dict(forward="3 (heads) + 3 (MaskSPADE) + 2 (seg loss + Kendall)", backward="1 (seg loss + Kendall) + 8 (MaskSPADE) + 5 (heads)")
    # channels_last with a batch-norm level in training: three more statistics launches
    assert of("spade", True)["forward"] == "3 (heads) + 6 (MaskSPADE) + 2 (seg loss + Kendall)"
    assert of("cbam", True) == dict(forward="3 (heads) + 4 (MaskCBAM) + 2 (seg loss + Kendall)", backward="1 (seg loss + Kendall) + 7 (MaskCBAM) + 5 (heads)")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(built_lib):
    from mga_yolo_amd import GateConfig, PyramidPlan, SlicePlan, SpadeConfig, SpadePyramidPlan
    from mga_yolo_amd.functional import spade_kernel_reason

    def spade(C_=64, **cfg):
        cfg = SpadeConfig(**{"hidden": 16, **cfg})
        h = cfg.hidden
        ps = [torch.zeros(h, 1, 3, 3), torch.zeros(h), torch.zeros(C_, h, 3, 3), torch.zeros(C_), torch.zeros(C_, h, 3, 3), torch.zeros(C_)]
        why = spade_kernel_reason(torch.empty(2, C_, 8, 8, device="meta"), torch.empty(2, 1, 8, 8, device="meta"), cfg)
        with pytest.raises(ValueError) as e:
            SpadePyramidPlan([(2, C_, 8, 8)], [ps], [cfg], device="cpu")
        assert why is not None and why in str(e.value)                        # the text of functional.spade_kernel_reason
    spade(hidden=24)
    spade(C_=40)
    spade(mask_channels=2)
    spade(hidden=80)
    hs = _head_states()
    params, cfgs, _ = _modules("eca")
    with pytest.raises(ValueError, match="gate"):
        SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, block="eca", gate=[GateConfig("deterministic")] * 3, device="cpu")
    params, cfgs, _ = _modules("cbam")
    with pytest.raises(ValueError, match="use_proj"):
        PyramidPlan.create(SHAPES, params, cfgs, channels_last=True, use_proj=True, device="cpu")
    with pytest.raises(ValueError, match="block"):
        SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, block="se", device="cpu")
    with pytest.raises(ValueError, match="target_resize"):
        SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, target_resize="bicubic", device="cpu")
    with pytest.raises(TypeError):
        SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, layout="nhwc", device="cpu")
    # gate= with MaskCBAM in channels_last is taken: the gate is layout-free
    gated = SlicePlan.create(SHAPES, HIDDEN, params, cfgs, hs, channels_last=True, gate=[GateConfig("deterministic")] * 3, device="cpu")
    assert gated.gated and gated.logits[0].data_ptr() == gated.block.logits[0].data_ptr() and gated.block.channels_last
    assert "+ 1 (gate)" in gated.launches()["forward"]


def test_exports():
    import mga_yolo_amd as M
    for name in ("PyramidPlan", "EcaPyramidPlan", "SpadePyramidPlan", "SlicePlan"):
        assert name in M.__all__ and hasattr(M, name)


# ---------------------------------------------------------------------------------------------------------------- the resample ABI
def test_fill_resample_sets_every_field(built_lib):
    from mga_yolo_amd import _binding, _lib
    small, big = torch.zeros(3, 1, 7, 5), torch.zeros(3, 1, 16, 12)
    L = _lib.ResampleLevel()
    _binding.fill_resample(L, small, big, (7, 5), (16, 12))
    assert {n: getattr(L, n) for n, _ in _lib.ResampleLevel._fields_} == dict(src=small.data_ptr(), dst=big.data_ptr(), B=3, in_h=7, in_w=5, out_h=16, out_w=12)
    _binding.fill_resample(L, big, small, (7, 5), (16, 12))                   # the same level refilled for the backward: the sizes keep their meaning
    assert (L.src, L.dst, L.in_h, L.out_w) == (big.data_ptr(), small.data_ptr(), 7, 12)


def _rs_level(_lib, **over):
    L = _lib.ResampleLevel()
    L.src, L.dst, L.B, L.in_h, L.in_w, L.out_h, L.out_w = P, P + 0x1000, 3, 7, 5, 16, 12
    for k, v in over.items():
        setattr(L, k, v)
    return L


RS_CASES = [("src NULL", dict(src=None), -1), ("dst NULL", dict(dst=None), -1),
            ("B = 0", dict(B=0), -2), ("B < 0", dict(B=-3), -2), ("in_h = 0", dict(in_h=0), -2), ("in_w < 0", dict(in_w=-1), -2),
            ("out_h = 0", dict(out_h=0), -2), ("out_w < 0", dict(out_w=-7), -2), ("out_w too large", dict(out_w=65537), -2),
            ("2^31 elements", dict(B=32768, out_h=256, out_w=256), -2),
            ("src misaligned", dict(src=0x10002), -4), ("dst misaligned", dict(dst=0x11001), -4)]


@pytest.mark.parametrize("what,over,code", RS_CASES, ids=[c[0] for c in RS_CASES])
def test_resample_argument_errors_come_before_any_launch(built_lib, what, over, code):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for name in ("mgaspade_resample_forward", "mgaspade_resample_backward"):
        for second in (False, True):                       # the bad level alone, and second of two: nothing is launched before it is found
            bad = _rs_level(_lib, **over)
            arr = (_lib.ResampleLevel * 2)(_rs_level(_lib), bad) if second else (_lib.ResampleLevel * 1)(bad)
            n = 2 if second else 1
            assert getattr(lib, name)(arr, n, None) == code, what
            msg = lib.mgacbam_last_error().decode()
            assert msg.startswith(name) and f"level {n - 1}" in msg, msg


def test_resample_level_count_and_null_table(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    arr = (_lib.ResampleLevel * 1)(_rs_level(_lib))
    for fn in (lib.mgaspade_resample_forward, lib.mgaspade_resample_backward):
        assert fn(None, 1, None) == _lib.E_NULL
        assert fn(arr, 0, None) == _lib.E_LEVELS and fn(arr, _lib.MAX_LEVELS + 1, None) == _lib.E_LEVELS and fn(arr, -1, None) == _lib.E_LEVELS
        assert lib.mgacbam_last_error()
