/* libmgacbam.so -- the detection post-process on the device: Detect decode, candidate selection and greedy non-maximum suppression, the
 * inference-side twin of include/mgadet.h.  A header of its own: include/mgacbam.h (ABI 15) is unchanged by it, and everything here
 * follows its conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed
 * in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked
 * before the first launch.  No host read-back: the outputs have a fixed size, so a call can sit in a captured graph behind the forward. */
#ifndef MGANMS_H_
#define MGANMS_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference's validator and predictor do after the forward (U = ultralytics: Detect._inference U/nn/modules/head.py:150-185,
 * make_anchors / dist2bbox U/utils/tal.py, non_max_suppression U/utils/ops.py:192-338 with torchvision's nms), per image:
 *   input        EITHER the Detect maps: level l is (B, 64 + nc, H_l, W_l), NCHW contiguous, read in place; anchors (j + 0.5, i + 0.5) in
 *                grid units, level after level, rows first; A = sum H_l W_l; each side's distance is the softmax expectation over its 16
 *                bins; the box is anchor -+ distance, times the level's stride; scores are sigmoid(cls)
 *                OR `pred`: an already decoded (B, 4 + nc, A) tensor, xywh in pixels and probabilities (what _inference returns); the box
 *                is centre -+ size / 2 (ops.xywh2xyxy)
 *   candidates   MGANMS_MULTI_LABEL (effective only when nc > 1): every (anchor, class) with prob > conf_thres.  Otherwise the anchor's
 *                best class if its prob > conf_thres; equal probabilities go to the lowest class index.  The candidate index is
 *                anchor * nc + class: anchor first, then class.  It is used only to break ties.
 *   max_nms      only the max_nms highest-scoring candidates of an image take part (ops.py:318-320); equal scores: lowest index first
 *   suppression  candidates are visited by descending score, equal scores by ascending candidate index; a candidate is kept unless its
 *                IoU with an already KEPT candidate is > iou_thres; IoU = inter / (area_a + area_b - inter), no eps; unless
 *                MGANMS_AGNOSTIC only candidates of the same class suppress each other; the visit stops after max_det keeps
 *   output       the kept rows in visiting order: dets (x1, y1, x2, y2, conf, cls), keep = the row's anchor index (return_idxs)
 *
 * Two departures from the reference, both deliberate:
 *   1. The reference separates classes by adding cls * max_wh (7680) to the coordinates in fp32.  That rounds them (at class 79 the
 *      spacing is 1/16 px) and lets boxes wider than max_wh meet across classes.  Here the classes are compared and the IoU is taken on
 *      the unshifted boxes.
 *   2. Half features are read and everything is computed in fp32; the arithmetic of the reference's .half() validation copy is not
 *      reproduced.
 * Parity with the reference is therefore defined on inputs where the fixture generator's guards hold (tools/gen_golden_nms.py: no
 * probability within 1e-5 relative of conf_thres, no compared pair's IoU within 1e-4 of iou_thres with or without the class offset).
 *
 * cand_cap is the number of candidates an image's list can hold.  An image with more candidates cannot be answered exactly: the call
 * sets *status = 1, the image's count becomes -1, its dets rows NaN and its keep rows -1; the other images are unaffected.
 * cand_cap = A * (nc if MGANMS_MULTI_LABEL and nc > 1 else 1) can never overflow.  Otherwise *status = 0.
 *
 * Launches: 2.  k_nms_cand: one thread per anchor; candidates are appended to the image's list (box 4 x fp32 and a 64-bit key: the
 * score's bits above the inverted candidate index, so the largest key is the next candidate to visit and the order of the appends cannot
 * change a result) with one atomic per wave; it also clears the status word.  k_nms_greedy: one workgroup per image; each round is one
 * sweep that kills what the last kept box suppresses and finds the largest live key; max_nms by a radix select over the keys before the
 * first round; it leaves the image's list counter at 0 for the next call.  ws must be zero-filled ONCE by the caller before its first
 * use (as the hand-off words of include/mgacbam.h are); after that no buffer has to be cleared between calls or replays.
 *
 * Refusals: n_levels outside 0 .. MGANMS_MAX_LEVELS: MGACBAM_E_LEVELS; an unknown dtype: MGACBAM_E_DTYPE; B, nc, H,
 * W, A < 1, A not the levels' sum, A * nc or B * A >= 2^31: MGACBAM_E_SHAPE; both feats and pred, strides not positive and
 * strictly ascending, conf_thres or iou_thres outside [0, 1] (NaN included), max_det < 1, max_nms < 1, cand_cap < 1, an unknown flag,
 * reserved != 0: MGACBAM_E_ARG; a NULL buffer (pred with n_levels = 0 included): MGACBAM_E_NULL; features or pred not aligned to
 * their element, an fp32 / int32 buffer not 4-byte aligned, ws not 16-byte aligned: MGACBAM_E_ALIGN; ws smaller than mganms_ws_bytes:
 * MGACBAM_E_SIZE.
 * Not built: the classes= filter and labels= (autolabelling); rotated boxes, end2end heads and extra mask channels (nc is C - 4);
 * reg_max != 16.  Channels_last maps, (B, H_l, W_l, 64 + nc) in memory, are read in place by mgamaps_nms_run (include/ext/mgamaps.h):
 * this header's own entry point takes NCHW maps only.
 * ------------------------------------------------------------------------------------------------ */
#define MGANMS_MAX_LEVELS 4
#define MGANMS_MULTI_LABEL 1
#define MGANMS_AGNOSTIC 2

typedef struct mganms_desc {
  const void* feats[MGANMS_MAX_LEVELS];    /* level l: (B, 64 + nc, H[l], W[l]) of `dtype`; all NULL with pred                       */
  const void* pred;                        /* (B, 4 + nc, A) of `dtype`, xywh in pixels and probabilities; NULL with feats           */
  int32_t H[MGANMS_MAX_LEVELS], W[MGANMS_MAX_LEVELS];
  int32_t stride[MGANMS_MAX_LEVELS];
  int32_t n_levels;                        /* 1 .. MGANMS_MAX_LEVELS with feats, 0 with pred                                        */
  int32_t A;                               /* anchors per image: with pred its last dimension; with feats 0 or the levels' sum      */
  int32_t B, nc;
  int32_t dtype;                           /* MGACBAM_F32 | MGACBAM_F16 | MGACBAM_BF16                                              */
  int32_t max_det;                         /* rows of an image's output (the reference: 300)                                        */
  int32_t max_nms;                         /* candidates that take part (the reference: 30000)                                      */
  int32_t flags;                           /* MGANMS_MULTI_LABEL | MGANMS_AGNOSTIC                                                  */
  float conf_thres, iou_thres;             /* in [0, 1]                                                                             */
  int32_t cand_cap;                        /* candidates an image's list holds                                                      */
  int32_t reserved;                        /* 0                                                                                     */
  float* dets;                             /* (B, max_det, 6) out: x1, y1, x2, y2, conf, cls; zeros past the image's count          */
  int32_t* count;                          /* (B) out: kept rows, -1 for an image whose list overflowed                             */
  int32_t* keep;                           /* (B, max_det) out: the anchor index of each kept row, -1 past the count                */
  int32_t* status;                         /* (1) out: 1 if an image's list overflowed, else 0                                      */
  void* ws;                                /* 16-byte aligned, zero-filled once before its first use                                */
  size_t ws_bytes;                         /* capacity of ws (checked: MGACBAM_E_SIZE)                                              */
} mganms_desc_t;

/* bytes of ws the descriptor's call needs; 0 for a descriptor mganms_run would refuse for anything but a buffer (the message then says
 * why) */
size_t mganms_ws_bytes(const mganms_desc_t* desc);
int mganms_run(const mganms_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGANMS_H_ */
