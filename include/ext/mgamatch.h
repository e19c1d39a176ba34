/* libmgacbam.so -- matching detections to labels on the device for the validation metrics: what the reference's validator does with the rows
 * of include/mganms.h, image by image on the host.  A header of its own, in a directory of its own: include/mgacbam.h (ABI 15) and the headers
 * beside it are unchanged by it.  It follows their conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every
 * launch on the stream passed in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every
 * argument is checked before the first launch.  No host read-back: a call can sit in a captured graph behind mganms_run. */
#ifndef MGAMATCH_H_
#define MGAMATCH_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference's validator does per image after the post-process (U = ultralytics: DetectionValidator.update_metrics, _prepare_batch,
 * _process_batch U/models/yolo/detect/val.py:131-271, box_iou U/utils/metrics.py:53-74, match_predictions U/engine/validator.py:249-290):
 *   labels       the image's rows of the batch's flat label list: batch_idx (n_cap), cls (n_cap), bboxes (n_cap, 4) xywh normalised, the
 *                form mgadet_desc_t takes; *n live rows (NULL: n_cap; clamped to 0 .. n_cap).  A row belongs to image b iff batch_idx == b;
 *                rows whose batch_idx is outside 0 .. B - 1 belong to no image.  Row order within an image is the flat order.  The box is
 *                (c -+ s / 2) * size with size = img_w, img_h, one rounding per operation.
 *   detections   dets (B, max_det, 6) = x1, y1, x2, y2, conf, cls and count (B), as mganms_run writes them; a negative count (an image
 *                whose candidate list overflowed) is taken as 0 rows, a count above max_det as max_det.
 *   IoU          inter / (area_l + area_d - inter + 1e-7) in fp32, every operation rounded once, in that order; a pair of different
 *                classes has IoU 0.  With MGAMATCH_SINGLE_CLS every class compares equal (pred["cls"] *= 0, the labels' classes ignored).
 *   the rule     for a detection d let l*(d) be the label with the largest IoU.  tp[d, t] is true iff iou[l*(d), d] >= iouv[t] (in fp32) and
 *                d is the lowest detection index among the detections d' with l*(d') = l*(d) and iou[l*(d'), d'] >= iouv[t].  This is what
 *                the reference's sort / unique / unique sequence computes.  So the lowest-index (highest-confidence) detection owns a
 *                label, not the one with the highest IoU, and a detection whose best label is owned stays false even if another label
 *                above the threshold is free.
 *   ties         equal IoUs of one detection with two labels of its class go to the LOWER label row.  The reference's order there is that
 *                of an unstable sort, so this case is defined here and excluded from reference parity.
 *
 * Per-call outputs: tp (B, max_det, niou) uint8, zeros past the count; best_iou (B, max_det) fp32, iou[l*(d), d], 0 past the count and where
 * there is no label; best_gt (B, max_det) int32, the flat label row l*(d), or -1 where the detection has no label of its class with IoU > 0.
 *
 * Accumulation over a validation run (optional: all of rows_tp, rows_conf, rows_cls, rows_img, tgt_cls, tgt_img, state given, or all NULL).
 * state (4) int32 = {n_rows, n_targets, seen, 0} lives on the device; the caller zeroes it before a run.  A call appends the batch's live
 * detection rows at n_rows, image after image and in detection order -- the offsets are a prefix sum over the counts, not the order of
 * atomics, so the result is the same bits on every run -- as rows_tp (niou bytes a row), rows_conf, rows_cls (0 with MGAMATCH_SINGLE_CLS)
 * and rows_img = seen + b; the label rows that belong to an image at n_targets in flat order, as tgt_cls and tgt_img = seen + batch_idx.
 * Then n_rows and n_targets grow by what was appended and seen by B.
 *
 * status (1): 0 ok.  1: an image has more than m_cap label rows; its tp rows are 0, its best_iou rows NaN, its best_gt rows -1, and nothing
 * is appended for the whole call (state is unchanged).  2: the append would pass rows_cap or tgt_cap; tp is written, nothing is appended and
 * state is unchanged.
 *
 * Launches: 2.  k_match: one workgroup per image; it stages the image's label rows in LDS, every thread strides over the detections and
 * keeps the largest class-matched IoU, and an integer minimum in LDS per (threshold, label) finds the owner.  k_match_append: a
 * workgroup per image and one per 256 label rows; the status word, the prefix over the counts and the copies.  ws carries one word per
 * image and a snapshot of state from the first to the second and needs no initialisation.
 *
 * Refusals: B, max_det < 1, n_cap < 0 or >= 2^29, B * max_det >= 2^31: MGACBAM_E_SHAPE; niou outside 1 .. MGAMATCH_MAX_IOU, iouv not strictly
 * ascending in (0, 1] (NaN included), m_cap outside 1 .. MGADET_MAX_GT (256), an unknown flag, reserved != 0, img_w or img_h not positive
 * and finite, rows_cap or tgt_cap < 1 with the accumulation on: MGACBAM_E_ARG; a NULL dets, count, tp, best_iou, best_gt, status or ws, NULL
 * labels with n_cap > 0, a partial set of the accumulation buffers: MGACBAM_E_NULL; an fp32 / int32 buffer not 4-byte aligned, ws not 16-byte
 * aligned: MGACBAM_E_ALIGN; ws smaller than mgamatch_ws_bytes: MGACBAM_E_SIZE.
 * Behind it: the confusion matrix (include/ext/mgaconfusion.h) and ap_per_class on this accumulation (include/ext/mgaap.h).
 * Not built: the scipy assignment branch of match_predictions, rotated boxes, the mask and pose matrices tp_m / tp_p.
 * ------------------------------------------------------------------------------------------------ */
#define MGAMATCH_MAX_IOU 16
#define MGAMATCH_SINGLE_CLS 1

typedef struct mgamatch_desc {
  const float* dets;                       /* (B, max_det, 6): x1, y1, x2, y2, conf, cls                                            */
  const int32_t* count;                    /* (B): live rows of each image; negative: 0                                             */
  const float* batch_idx;                  /* (n_cap)                                                                               */
  const float* cls;                        /* (n_cap)                                                                               */
  const float* bboxes;                     /* (n_cap, 4): xywh normalised                                                           */
  const int32_t* n;                        /* (1) live label rows on the device, or NULL: n_cap                                     */
  int32_t B, max_det;
  int32_t n_cap;                           /* rows the label buffers hold (0: no labels, the three may be NULL)                     */
  int32_t m_cap;                           /* label rows an image may have, 1 .. MGADET_MAX_GT                                      */
  float img_w, img_h;                      /* what the normalised label boxes are scaled by                                         */
  int32_t niou;                            /* 1 .. MGAMATCH_MAX_IOU                                                                 */
  int32_t flags;                           /* MGAMATCH_SINGLE_CLS                                                                   */
  float iouv[MGAMATCH_MAX_IOU];            /* the first niou: strictly ascending, in (0, 1]                                         */
  int32_t rows_cap, tgt_cap;               /* rows the accumulation buffers hold                                                    */
  uint8_t* tp;                             /* (B, max_det, niou) out                                                                */
  float* best_iou;                         /* (B, max_det) out                                                                      */
  int32_t* best_gt;                        /* (B, max_det) out                                                                      */
  uint8_t* rows_tp;                        /* (rows_cap, niou)                                                                      */
  float* rows_conf;                        /* (rows_cap)                                                                            */
  float* rows_cls;                         /* (rows_cap)                                                                            */
  int32_t* rows_img;                       /* (rows_cap)                                                                            */
  float* tgt_cls;                          /* (tgt_cap)                                                                             */
  int32_t* tgt_img;                        /* (tgt_cap)                                                                             */
  int32_t* state;                          /* (4): n_rows, n_targets, seen, 0                                                       */
  int32_t* status;                         /* (1) out: 0, 1 or 2                                                                    */
  void* ws;                                /* 16-byte aligned                                                                       */
  size_t ws_bytes;                         /* capacity of ws (checked: MGACBAM_E_SIZE)                                              */
  int32_t reserved;                        /* 0                                                                                     */
} mgamatch_desc_t;

/* bytes of ws the descriptor's call needs; 0 for a descriptor mgamatch_run would refuse for anything but a buffer (the message then says
 * why) */
size_t mgamatch_ws_bytes(const mgamatch_desc_t* desc);
int mgamatch_run(const mgamatch_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGAMATCH_H_ */
