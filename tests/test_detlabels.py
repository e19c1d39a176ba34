"""The one definition of a batch's labels (mga_yolo_amd/detlabels.py) without a GPU: the per-image table of rows against a plain loop, the static
buffers' refusal, and box_iou on pairs computed by hand."""
import math

import pytest
import torch

from mga_yolo_amd import detlabels as L

NAN = float("nan")
# (batch_idx, B): what the table must get right, each on its own and all at once
TABLES = {
    "image without labels": ([0, 2, 2, 0], 3),
    "minus one and B": ([-1, 0, 2, 1, 0], 2),
    "fractional": ([0.5, 1, 0, 1.5, 1], 2),
    "nan": ([NAN, 0, 1, NAN], 2),
    "n = 0": ([], 3),
    "shuffled": ([2, 0, 1, 0, 2, 2, 1, 0, 2], 3),
    "everything": ([3, 1, NAN, -1, 0.5, 1, 3, 4, 1, -0.0, 2.5], 4),
    "nobody's": ([-1, 7, NAN, 0.25], 2),
}


def loop_rows(batch_idx, B):
    """the rule row by row: image b's rows are those with batch_idx == b, b = 0 .. B - 1 -- in range and integral by construction"""
    per = [[r for r, v in enumerate(batch_idx) if v == b] for b in range(B)]
    belongs = [any(r in p for p in per) for r in range(len(batch_idx))]
    return per, belongs


@pytest.mark.parametrize("name", TABLES)
def test_rows_per_image_is_the_plain_loop(name):
    batch_idx, B = TABLES[name]
    per, belongs = loop_rows(batch_idx, B)
    rows, has, got = L.rows_per_image(torch.tensor(batch_idx, dtype=torch.float32), B)
    M = max(len(p) for p in per)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (B, M) and tuple(has.shape) == (B, M)
    assert got.tolist() == belongs
    for b in range(B):
        assert rows[b].tolist() == per[b] + [-1] * (M - len(per[b]))            # flat order, then the padding
        assert has[b].tolist() == [True] * len(per[b]) + [False] * (M - len(per[b]))


def test_size_m_cap_is_the_fullest_image_and_at_least_one():
    assert L.size_m_cap(torch.tensor([2., 0, 1, 0, 2, 2, -1, 3]), 3) == 3
    assert L.size_m_cap(torch.zeros(0), 3) == 1 and L.size_m_cap(torch.tensor([-1., 5]), 2) == 1


def test_label_buffers_refuse_a_row_too_many_and_write_n():
    buf = L.LabelBuffers(3, "cpu")
    assert (buf.batch_idx.shape, buf.cls.shape, buf.bboxes.shape, buf.n.dtype) == ((3,), (3,), (3, 4), torch.int32)
    bi, cl, bx = torch.tensor([1., 0]), torch.tensor([[4.], [5.]]), torch.arange(8.).reshape(2, 4)
    buf.set(bi, cl, bx, "SomePlan")
    assert int(buf.n) == 2 and buf.batch_idx[:2].tolist() == [1, 0] and buf.cls[:2].tolist() == [4, 5] and torch.equal(buf.bboxes[:2], bx)
    with pytest.raises(ValueError, match=r"^SomePlan: 4 label rows, the plan holds 3$"):
        buf.set(torch.zeros(4), torch.zeros(4), torch.zeros(4, 4), "SomePlan")
    assert int(buf.n) == 2                                                       # a refused batch leaves the buffers as they were
    buf.set(torch.zeros(0), torch.zeros(0), torch.zeros(0, 4), "SomePlan")
    assert int(buf.n) == 0


def test_pair_iou_by_hand():
    # label (0, 0, 2, 2) and detection (1, 1, 3, 3): intersection 1, union 4 + 4 - 1 = 7; detection (5, 5, 6, 6) is disjoint
    lb = torch.tensor([[[0., 0, 2, 2]]], dtype=torch.float64)
    db = torch.tensor([[[1., 1, 3, 3], [5, 5, 6, 6]]], dtype=torch.float64)
    iou = L.pair_iou(lb, db)
    assert tuple(iou.shape) == (1, 2, 1)
    assert math.isclose(float(iou[0, 0, 0]), 1 / (7 + 1e-7), rel_tol=1e-15)
    assert float(iou[0, 1, 0]) == 0.0


def test_label_boxes_and_img_wh():
    assert L.img_wh(64) == (64.0, 64.0) and L.img_wh((48, 96)) == (96.0, 48.0)         # (h, w) -> (img_w, img_h)
    box = L.label_boxes(torch.tensor([[0.5, 0.5, 0.25, 0.5]]), 96.0, 48.0)
    assert box.tolist() == [[36.0, 12.0, 60.0, 36.0]]
