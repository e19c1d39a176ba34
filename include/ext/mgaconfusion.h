/* libmgacbam.so -- the validator's confusion matrix on the device: what the reference's ConfusionMatrix.process_batch does with the rows of
 * include/mganms.h and the batch's labels, image by image on the host.  The third stage behind mganms_run and mgamatch_run
 * (include/ext/mgamatch.h), in a header of its own: the headers beside and above it are unchanged by it.  It follows their conventions: plain
 * C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed in, return value 0 / MGACBAM_E_* /
 * hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked before the first launch.  No host
 * read-back: a call can sit in a captured graph behind mgamatch_run. */
#ifndef MGACONFUSION_H_
#define MGACONFUSION_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference does per image when it plots (U = ultralytics: ConfusionMatrix.process_batch U/utils/metrics.py:378-456, box_iou
 * U/utils/metrics.py:53-74), with the labels and detections in the form mgamatch_desc_t takes them:
 *   labels       batch_idx (n_cap), cls (n_cap), bboxes (n_cap, 4) xywh normalised; *n live rows (NULL: n_cap; clamped to 0 .. n_cap).  A
 *                row belongs to image b iff batch_idx == b; the box is (c -+ s / 2) * size with size = img_w, img_h.
 *   detections   dets (B, max_det, 6) = x1, y1, x2, y2, conf, cls and count (B); a negative count is taken as 0 rows, one above max_det
 *                as max_det.
 *   counted      a detection is counted iff conf > conf_thres, in fp32 and strictly; a NaN confidence is not counted.  conf_thres is the
 *                value the reference uses AFTER its own substitution (0.25 for None or 0.001): that belongs to the caller.
 *   IoU          inter / (area_l + area_d - inter + 1e-7) in fp32, every operation rounded once, in that order: the expression of
 *                mgamatch_run, between every label of the image and every counted detection WHATEVER THEIR CLASSES.  A pair qualifies iff
 *                iou > iou_thres, strictly; a NaN IoU does not qualify.
 *   the rule     l*(d): the label with the largest qualifying IoU for d, none if no pair qualifies.  w(l): among the counted detections
 *                with l*(d) = l the one with the largest iou[l, d], none if there is none.  A detection that loses its l* is not tried
 *                against its second-best label.  This is what the reference's sort / unique / sort / unique sequence computes.  Unlike
 *                mgamatch_run's rule it ignores classes, its comparisons are strict, and the highest IoU owns a label, not the lowest
 *                detection index.
 *   counts       the matrix has nc + 1 rows and columns, indexed [predicted, true], index nc meaning background.  A label with a winner
 *                adds 1 to [cls(w(l)), cls(l)]; a label without one adds 1 to [nc, cls(l)]; a counted detection that is nobody's winner
 *                adds 1 to [cls(d), nc].  A class is truncated toward zero, as .int() does; with MGACM_SINGLE_CLS every class is taken as 0.
 *   ties         equal IoUs of one detection with two labels go to the LOWER label row; equal IoUs of two detections claiming one label go
 *                to the LOWER detection index.  The reference's order there is that of an unstable sort, so both cases are defined here
 *                and excluded from reference parity.
 *
 * Per-call outputs: det_out (B, max_det) int32: the class of the label the detection won (0 .. nc - 1), nc for a counted detection that
 * won none (a false positive), -1 for a row that is not counted or lies past the count.  lab_out (n_cap) int32: the class of the label's
 * winner, nc for a label without one (a false negative), -1 for a row behind the n word or of no image.  cm (nc + 1, nc + 1) int32: the
 * call's matrix, every cell stored (no zeroing needed).  acc (nc + 1, nc + 1) int64, or NULL: the run-long matrix, cm is added to it; the
 * caller zeroes it before a run.  One workgroup adds with plain stores, so the result is the same bits on every run.
 *
 * status (1): 0 ok.  1: an image has more than m_cap label rows; its det_out and lab_out rows are -1, the other images' are written.  3: a
 * counted detection or a live label row of an image has a class that is not finite or whose truncation is outside 0 .. nc - 1 (the
 * reference raises or wraps there).  1 takes precedence over 3.  On a non-zero status cm is all zeros and acc is untouched.
 *
 * Launches: 2.  k_cm_match: one workgroup per image; it stages the image's label rows in LDS as k_match does, every thread strides over the
 * counted detections and keeps the largest qualifying IoU, and one 64-bit integer maximum in LDS per label over (IoU bits, lowest
 * detection index) finds the winner, whatever order the claims arrive in.  k_cm_count: one workgroup; the status word, a histogram of the
 * outcomes in (nc + 1)^2 int32 cells of LDS, the stores.  ws carries two words per image from the first to the second and needs no
 * initialisation.  No hand-off between workgroups and no spinning: the second launch's order after the first is the stream's.
 *
 * Refusals: B, max_det < 1, n_cap < 0 or >= 2^29, B * max_det >= 2^31: MGACBAM_E_SHAPE; nc outside 1 .. MGACM_MAX_NC (the cells fit the
 * workgroup's static LDS: 120 * 120 * 4 = 57 600 bytes), m_cap outside 1 .. MGADET_MAX_GT (256), an unknown flag, reserved != 0, img_w or
 * img_h not positive and finite, conf_thres not finite, iou_thres not finite or outside [0, 1): MGACBAM_E_ARG; a NULL dets, count, det_out,
 * cm, status or ws, NULL labels or lab_out with n_cap > 0: MGACBAM_E_NULL; an fp32 / int32 buffer not 4-byte aligned, acc not 8-byte
 * aligned, ws not 16-byte aligned: MGACBAM_E_ALIGN; ws smaller than mgacm_ws_bytes: MGACBAM_E_SIZE.
 * ap_per_class is the stage behind this one (include/ext/mgaap.h).
 * Not built: plot_matches / visualize (the TP / FP / FN index lists), rotated boxes (batch_probiou), the classification
 * task's process_cls_preds, nc above MGACM_MAX_NC.
 * ------------------------------------------------------------------------------------------------ */
#define MGACM_MAX_NC 119
#define MGACM_SINGLE_CLS 1

typedef struct mgacm_desc {
  const float* dets;                       /* (B, max_det, 6): x1, y1, x2, y2, conf, cls                                            */
  const int32_t* count;                    /* (B): live rows of each image; negative: 0                                             */
  const float* batch_idx;                  /* (n_cap)                                                                               */
  const float* cls;                        /* (n_cap)                                                                               */
  const float* bboxes;                     /* (n_cap, 4): xywh normalised                                                           */
  const int32_t* n;                        /* (1) live label rows on the device, or NULL: n_cap                                     */
  int32_t B, max_det;
  int32_t n_cap;                           /* rows the label buffers hold (0: no labels, the three and lab_out may be NULL)         */
  int32_t m_cap;                           /* label rows an image may have, 1 .. MGADET_MAX_GT                                      */
  int32_t nc;                              /* 1 .. MGACM_MAX_NC                                                                     */
  int32_t flags;                           /* MGACM_SINGLE_CLS                                                                      */
  float img_w, img_h;                      /* what the normalised label boxes are scaled by                                         */
  float conf_thres;                        /* finite; counted: conf > conf_thres                                                    */
  float iou_thres;                         /* in [0, 1); a pair qualifies: iou > iou_thres                                          */
  int32_t* det_out;                        /* (B, max_det) out                                                                      */
  int32_t* lab_out;                        /* (n_cap) out                                                                           */
  int32_t* cm;                             /* (nc + 1, nc + 1) out: [predicted, true]                                               */
  int64_t* acc;                            /* (nc + 1, nc + 1) in / out, or NULL: no accumulation                                   */
  int32_t* status;                         /* (1) out: 0, 1 or 3                                                                    */
  void* ws;                                /* 16-byte aligned                                                                       */
  size_t ws_bytes;                         /* capacity of ws (checked: MGACBAM_E_SIZE)                                              */
  int32_t reserved;                        /* 0                                                                                     */
} mgacm_desc_t;

/* bytes of ws the descriptor's call needs; 0 for a descriptor mgacm_run would refuse for anything but a buffer (the message then says
 * why) */
size_t mgacm_ws_bytes(const mgacm_desc_t* desc);
int mgacm_run(const mgacm_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGACONFUSION_H_ */
