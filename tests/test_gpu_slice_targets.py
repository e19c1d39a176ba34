"""SlicePlan.create(target_source=...): the plan builds its segmentation targets from the batch's full-resolution masks as the first launch
of the step.  Plan A owns ``mask_full`` and is given the masks; plan B is the same plan as it has always been built, its ``targets`` filled
with torch's pools of the same masks.  Everything else is equal, the kernels are fixed-order, and the targets are exact -- so after a step
the two plans hold the same bits."""
import pytest
import torch

import targets_cases as T
from plan_replays import block_args, build_modules

pytestmark = pytest.mark.gpu

SHAPES = [(4, 16, 16, 16), (4, 32, 8, 8), (4, 64, 4, 4)]
HIDDEN = [16, 32, 64]


def _plans(block, shapes, hidden, source, method="avgpool", bridge=False, resize="bilinear"):
    from mga_yolo_amd import SlicePlan
    heads, blocks = build_modules(block, shapes, hidden)
    params, cfgs, running = block_args(block, blocks)
    states = [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in heads]
    kw = dict(block=block, block_running=running, target_resize=resize, scale_weights=(1.0, 0.5, 2.0))
    a = SlicePlan.create(shapes, hidden, params, cfgs, states, target_source=source, target_method=method, target_bridge=bridge, **kw)
    hw = [(-(-source[0] // s), -(-source[1] // s)) for s in T.MODEL_STRIDES[:len(shapes)]]
    b = SlicePlan.create(shapes, hidden, params, cfgs, states, target_hw=hw, **kw)
    assert a.target_strides == T.MODEL_STRIDES[:len(shapes)] and [tuple(t.shape[2:]) for t in a.targets] == hw
    assert a.mask_full.shape == (shapes[0][0], *source) and a.mask_full.dtype == torch.uint8 and not hasattr(b, "mask_full")
    return a, b


def _load(plans, shapes, seed):
    g = torch.Generator().manual_seed(seed)
    for l, shp in enumerate(shapes):
        x, gy = torch.randn(shp, generator=g).cuda(), torch.randn(shp, generator=g).cuda()
        for p in plans:
            p.x[l].copy_(x); p.gy[l].copy_(gy)
    det = (torch.rand(3, generator=g) * 2.0 + 0.5).cuda()
    for p in plans:
        p.det_loss.copy_(det); p.log_vars.copy_(torch.tensor([0.3, -0.4]).cuda())


def _fill_masks(a, b, seed, method="avgpool", bridge=False):
    """a fresh mask for plan A; torch's pools of it for plan B.  Foreground is any value > 0: the masks carry 0, 1 and 255."""
    g = torch.Generator().manual_seed(seed)
    shape = tuple(a.mask_full.shape)
    m = (torch.rand(shape, generator=g) < 0.25 + 0.1 * (seed % 4)).to(torch.uint8) * (1 + 254 * (torch.rand(shape, generator=g) < 0.5).to(torch.uint8))
    a.mask_full.copy_(m)
    want = T.compose(m, a.target_strides, method, bridge)
    for t, w in zip(b.targets, want):
        t.copy_(w)
    return want


def _same(a, b, want):
    torch.cuda.synchronize()
    a.check_handoff(); b.check_handoff()
    for l, w in enumerate(want):
        assert torch.equal(a.targets[l].cpu(), w), f"targets[{l}]"
    assert torch.equal(a.total, b.total) and torch.equal(a.seg_out, b.seg_out) and torch.equal(a.grad_bucket, b.grad_bucket)
    assert bool(torch.isfinite(a.total).all()) and float(a.seg_out[0]) > 0 and float(a.grad_bucket.abs().max()) > 0


@pytest.mark.parametrize("block", ["cbam", "eca", "spade"])
def test_step_from_masks_equals_step_from_pooled_targets(built_lib, block):
    a, b = _plans(block, SHAPES, HIDDEN, (128, 128))
    _load((a, b), SHAPES, 11)
    want = _fill_masks(a, b, 0)
    a.step(); b.step()
    _same(a, b, want)
    if block != "cbam":
        return
    # the same over three replays of captured graphs, a fresh mask before each
    ga, gb = a.capture(a.step), b.capture(b.step)
    seen = []
    for t in range(3):
        want = _fill_masks(a, b, 1 + t)
        ga.replay(); gb.replay()
        _same(a, b, want)
        seen.append(a.total.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])        # the replays did read the new masks


def test_padded_sizes(built_lib):
    """100 x 76 masks: 13 x 10, 7 x 5 and 4 x 3 targets, the last row and column of each from zero-padded cells"""
    shapes = [(2, 16, 13, 10), (2, 16, 7, 5), (2, 16, 4, 3)]
    a, b = _plans("cbam", shapes, [8, 8, 8], (100, 76))
    _load((a, b), shapes, 12)
    want = _fill_masks(a, b, 2)
    a.step(); b.step()
    _same(a, b, want)


def test_maxpool_targets_with_the_closing(built_lib):
    a, b = _plans("cbam", SHAPES, HIDDEN, (128, 128), method="maxpool", bridge=True, resize="nearest")
    _load((a, b), SHAPES, 13)
    m = T.diagonal_mask((4, 128, 128))
    a.mask_full.copy_(m)
    want = T.compose(m, T.MODEL_STRIDES, "maxpool", bridge=True)
    assert not torch.equal(want[0], T.compose(m, T.MODEL_STRIDES, "maxpool")[0])
    for t, w in zip(b.targets, want):
        t.copy_(w)
    a.step(); b.step()
    _same(a, b, want)


def test_launches_report_the_added_launch(built_lib):
    from mga_yolo_amd import SlicePlan
    for block in ("cbam", "eca", "spade"):
        a, b = _plans(block, SHAPES, HIDDEN, (128, 128))
        la, lb = a.launches(), b.launches()
        assert la["forward"] == "1 (targets) + " + lb["forward"] and la["backward"] == lb["backward"]
    a, b = _plans("cbam", SHAPES, HIDDEN, (128, 128), method="maxpool", bridge=True)
    assert a.launches()["forward"] == "2 (targets) + " + b.launches()["forward"]
    # a plan created without target_source reports what it always did, through either constructor
    assert b.launches() == dict(forward="3 (heads) + 2 (MaskCBAM) + 2 (seg loss + Kendall)", backward="1 (seg loss + Kendall) + 2 (MaskCBAM) + 5 (heads)")
    heads, blocks = build_modules("cbam", SHAPES, HIDDEN)
    params, cfgs, _ = block_args("cbam", blocks)
    old = SlicePlan(SHAPES, HIDDEN, params, cfgs, [{k: v.detach().clone() for k, v in h.state_dict().items()} for h in heads])
    assert old.launches() == b.launches() and old._tgt is None and not hasattr(old, "mask_full")
