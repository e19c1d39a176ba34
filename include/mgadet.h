/* libmgacbam.so -- the detection criterion on the device: task-aligned assignment, CIoU, DFL and BCE on the Detect head's feature maps.
 * A header of its own: include/mgacbam.h (ABI 15) is unchanged by it -- no struct, flag, enum or function of it moves -- and everything
 * here follows its conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream
 * passed in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every argument is
 * checked before the first launch.  MGACBAM_E_ARG comes from include/mgatargets.h. */
#ifndef MGADET_H_
#define MGADET_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference's v8DetectionLoss computes (U = ultralytics: U/utils/loss.py:194-297, U/utils/tal.py:14-329,
 * U/utils/metrics.py:77-141), on the feature maps as the Detect head leaves them: level l is (B, 4 * 16 + nc, H_l, W_l), NCHW
 * contiguous, read in place -- the cat / split / permute / contiguous copies of loss.py:247-252 are never made.
 *   anchors      (i + 0.5, j + 0.5) in grid units, level after level, rows first (tal.py:367-379); A = sum H_l W_l
 *   labels       row r = (batch_idx[r], cls[r], bboxes[r] as normalised xywh), r < n.  The g-th row of an image is its ground truth g
 *                (loss.py:217-232); the box is scaled by (W_0 s_0, H_0 s_0) and becomes xyxy; it is valid iff x1 + y1 + x2 + y2 > 0
 *                (loss.py:263).  n is read from the device word `n` (NULL: n = n_cap), so a captured graph replays with another count.
 *   decode       softmax over each side's 16 bins, expectation, anchor -+ distance, in grid units (loss.py:234-241)
 *   assignment   on detached quantities (tal.py:92-154): an anchor is inside a box iff min(deltas) > 1e-9 in pixels (tal.py:279-299);
 *                overlap = clamp(CIoU(gt, pred), 0), eps = 1e-7, both in pixels; metric = sigmoid(score[label])^0.5 overlap^6;
 *                per valid ground truth the topk anchors inside it by metric; an anchor several ground truths claim goes to the
 *                arg-max over ALL ground truths of the overlap (0 outside the box; the first index wins a tie; tal.py:317-326);
 *                target_score = onehot(label) max_g(metric pos_overlap_g / (pos_metric_g + 1e-9))   (tal.py:121-125)
 *   tss          max(sum of target scores, 1)                                                       (loss.py:280)
 *   cls          sum BCEWithLogits(scores, target_scores) / tss                                     (loss.py:284)
 *   box          sum (1 - CIoU(pred, target)) weight / tss over assigned anchors, in grid units, weight = the anchor's target-score
 *                sum; CIoU's alpha is not differentiated (metrics.py:139-140)                        (loss.py:127-129)
 *   dfl          the target ltrb clamped to [0, 14.99], cross-entropy against its two neighbouring bins, mean over the sides, times
 *                weight, / tss                                                                       (loss.py:95-105, 133-135)
 *   out          gains * (box, cls, dfl) * B; items = gains * (box, cls, dfl)                       (loss.py:293-297)
 *
 * Ties.  torch.topk leaves the order of equal metrics open.  Equal metrics arise at exactly 0 only (CIoU <= 0, or fewer than topk
 * anchors inside a small box).  Here a tie goes to the lowest anchor index among the anchors inside the box, and an anchor outside the
 * box is never selected.  A zero-metric positive that stays with a ground truth that picked it has target score 0, hence weight 0 in
 * every term: the loss and every gradient are the same under either order, while the foreground mask is not -- UNLESS an anchor of
 * metric 0 is picked by two ground truths and thereby handed to a third: a contested anchor goes to the arg-max of the overlap over
 * ALL ground truths, which may be one that did not pick it and overlaps it, and there its weight is positive.  Which zero-metric
 * anchors two boxes both pick depends on the order, and then so do the loss and the gradients (crowded scenes of large boxes: 280
 * boxes of 16 to 60 px in three 256^2 images move the loss by 0.8 % between the two orders).  The rule here -- inside the
 * box first, lowest anchor index -- is deterministic; the reference's top-k runs over all anchors with those outside the box at 0, so
 * its pick among zeros is arbitrary.  Parity with the reference is therefore defined only on inputs where the fixture generator's
 * guards hold (tools/gen_golden_det.py: no near-tie at a top-k cut or a contested arg-max, and both tie orders give the same bits),
 * there on the loss, the gradients and the target scores, and on the foreground mask, the assigned ground truth and its box ONLY
 * where the anchor's weight is > 0.
 *
 * Element types: the features (and their gradients) are fp32, fp16 or bf16; they are read, and everything is accumulated, in fp32
 * (the reference's own half-precision arithmetic under autocast is not reproduced).  Every sum has a fixed order: two runs give the
 * same bits.
 *
 * An image with more than m_cap label rows cannot be assigned: the call then sets *status = 1 and writes NaN to out and items (and the
 * backward NaN to every gradient); otherwise *status = 0.  A class outside 0 .. nc - 1 is clamped into it.
 *
 * Launches: mgadet_forward 4 (k_det_assign, k_det_resolve, k_det_loss, k_det_final), mgadet_backward 1 (k_det_bwd).  The backward
 * reads what its forward left in assign_gt, assign_score and ws, and dL/d(out) from DEVICE memory.
 *
 * Refusals: n_levels outside 1 .. MGADET_MAX_LEVELS: MGACBAM_E_LEVELS; an unknown dtype: MGACBAM_E_DTYPE; B, nc, H, W < 1 or
 * B * A >= 2^31 or n_cap < 0: MGACBAM_E_SHAPE; reg_max != 16, topk outside 1 .. MGADET_MAX_TOPK, m_cap outside 1 .. MGADET_MAX_GT,
 * strides not positive and strictly ascending, reserved != 0: MGACBAM_E_ARG; a NULL buffer: MGACBAM_E_NULL; features not aligned to
 * their element, an fp32 / int32 buffer not 4-byte aligned, ws not 16-byte aligned: MGACBAM_E_ALIGN; ws smaller than mgadet_ws_bytes:
 * MGACBAM_E_SIZE.
 * Not built: reg_max != 16, the rotated and the segmentation criteria.  Channels_last maps, (B, H_l, W_l, 64 + nc) in memory, are read
 * and their gradients written in place by mgamaps_det_forward / mgamaps_det_backward (include/ext/mgamaps.h): this header's own entry
 * points take NCHW maps only.
 * ------------------------------------------------------------------------------------------------ */
#define MGADET_MAX_LEVELS 4
#define MGADET_MAX_TOPK 16
#define MGADET_MAX_GT 256

typedef struct mgadet_desc {
  const void* feats[MGADET_MAX_LEVELS];    /* level l: (B, 64 + nc, H[l], W[l]) of `dtype`                                   */
  void* g_feats[MGADET_MAX_LEVELS];        /* backward: dL/dfeats, same shape and type, every element written; forward: unused */
  int32_t H[MGADET_MAX_LEVELS], W[MGADET_MAX_LEVELS];
  int32_t stride[MGADET_MAX_LEVELS];
  int32_t n_levels, B, nc, reg_max;        /* reg_max: 16                                                                    */
  int32_t dtype;                           /* MGACBAM_F32 | MGACBAM_F16 | MGACBAM_BF16                                       */
  int32_t topk;                            /* 1 .. MGADET_MAX_TOPK (the reference: 10)                                       */
  int32_t n_cap;                           /* rows the label buffers hold                                                    */
  int32_t m_cap;                           /* ground truths an image may have, 1 .. MGADET_MAX_GT                            */
  float gains[3];                          /* box, cls, dfl (the reference: 7.5, 0.5, 1.5)                                   */
  int32_t reserved;                        /* 0                                                                              */
  const float* batch_idx;                  /* (n_cap) fp32; may be NULL when n_cap = 0, as cls and bboxes                    */
  const float* cls;                        /* (n_cap) fp32                                                                   */
  const float* bboxes;                     /* (n_cap, 4) fp32, xywh normalised                                               */
  const int32_t* n;                        /* device word: live rows, clamped to 0 .. n_cap; NULL: n_cap                     */
  int32_t* assign_gt;                      /* (B, A) out: the label row an anchor is assigned to, -1: background             */
  float* assign_score;                     /* (B, A) out: the anchor's target score (at its ground truth's class)            */
  float* out;                              /* (3) out: gains * (box, cls, dfl) * B                                           */
  float* items;                            /* (3) out: gains * (box, cls, dfl)                                               */
  int32_t* status;                         /* (1) out: 1 if an image has more than m_cap rows, else 0                        */
  const float* upstream;                   /* backward: (3) dL/d(out) in device memory; forward: unused                      */
  void* ws;                                /* 16-byte aligned; the backward needs it as its forward left it                  */
  size_t ws_bytes;                         /* capacity of ws (checked: MGACBAM_E_SIZE)                                       */
} mgadet_desc_t;

/* bytes of ws the descriptor's calls need; 0 for a descriptor mgadet_forward would refuse for anything but a buffer (the message then
 * says why) */
size_t mgadet_ws_bytes(const mgadet_desc_t* desc);
int mgadet_forward(const mgadet_desc_t* desc, void* stream);
int mgadet_backward(const mgadet_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGADET_H_ */
