/* libmgacbam.so -- a batch of uint8 images prepared on the device in one launch: the division by 255, the conversion to the network's
 * element type, the memory layout, the channel order and the bilinear resize of multi-scale training -- what the reference does with a chain
 * of torch operators over the largest tensor of a step (U = ultralytics: DetectionTrainer.preprocess_batch U/models/yolo/detect/train.py,
 * DetectionValidator.preprocess U/models/yolo/detect/val.py, BasePredictor.preprocess U/engine/predictor.py).  A header of its own: the
 * headers beside and above it are unchanged by it.  It follows their conventions: plain C, caller-owned buffers, nothing allocated, copied
 * or synchronised, the launch on the stream passed in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through
 * mgacbam_last_error().  Every argument is checked before the launch.  No workspace. */
#ifndef MGAIMAGE_H_
#define MGAIMAGE_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The rule.
 *   source       uint8, (B,C,in_h,in_w) contiguous, or with MGAIMG_SRC_NHWC (B,in_h,in_w,C) contiguous.  C is 1 .. 4.  No alignment is asked
 *                of it.  With MGAIMG_REVERSE_C destination channel c reads source channel C - 1 - c (BGR to RGB), in either source layout.
 *   destination  (B,C,out_h,out_w) in dtype (MGACBAM_F32 / F16 / BF16), contiguous, or with MGAIMG_DST_NHWC stored as (B,out_h,out_w,C):
 *                torch's channels_last.  Aligned to its element.
 *   the unit     q(v) = fp32(v) / 255.0f, a correctly rounded fp32 division: v.float() / 255 as torch evaluates it on the host.  Not
 *                p(v) = fp32(v) * (1.0f / 255.0f): that differs from the quotient by one ulp for 126 of the 256 byte values.  Rounded to
 *                fp16 or bf16 the two agree for all 256.
 *   no resize    (out_h, out_w) == (in_h, in_w):  bit for bit v.float() / 255, v.half() / 255 and v.to(bfloat16) / 255 as torch evaluates
 *                them ON THE DEVICE, the composition this call replaces.  There a tensor divided by a host scalar is multiplied by the
 *                scalar's fp32 reciprocal, so out = round_to_dtype(p(v)): in fp16 and bf16 the rounded quotient, in fp32 the product.
 *   resize       F.interpolate(v / 255 in fp32, size=(out_h, out_w), mode="bilinear", align_corners=False), rounded once to dtype.  Per axis
 *                the fp32 coordinate rule of include/mgaresample.h: scale = f32(n_in) / f32(n_out), f = max(scale * (j + 0.5) - 0.5, 0),
 *                i0 = min(int(f), n_in - 1), i1 = i0 + (i0 < n_in - 1), lam = f - i0, no operation contracted.  The four taps are the fp32
 *                quotients q of the four bytes; the blend is fma(1 - ly, top, ly * bot) with top = fma(lx, t01, (1 - lx) * t00) and bot
 *                likewise, the same operations in either destination layout.  Nothing but bytes is read from the source, and no
 *                full-size fp32 image exists at any point.
 *
 * One launch per call.
 *   k_img_convert (no resize).  Every load and store instruction of a wave covers one contiguous range, 4 bytes a lane on the source side and
 *                4 elements a lane (16 or 8 bytes) on the destination side.  Where source and destination order agree (the same layout and no
 *                reversal, or C = 1) the batch is one flat stream.  Otherwise a workgroup copies MGAIMG_TILE_PX pixels of one sample -- C
 *                runs of a planar source, one run of an interleaved one -- into LDS with 4-byte loads and writes them out in destination
 *                order.  The vectors start where the destination is aligned to them; the elements before that, and behind the last whole
 *                vector, go one by one.
 *   k_img_resize One workgroup per tile of up to MGAIMG_TILE_H x MGAIMG_TILE_W destination pixels of one sample, all channels; a tile spans the
 *                full width where out_w <= MGAIMG_TILE_W, so that its rows are one contiguous run in either layout.  The taps and weights of
 *                the tile's rows and columns are formed once, in LDS, and the 256 quotients v / 255 are a table there.  The four bytes of a
 *                pixel are gathered through the cache; the stores are those of k_img_convert.
 *
 * Refusals: a NULL desc, src or dst: MGACBAM_E_NULL; B, in_h, in_w, out_h or out_w below 1, C outside 1 .. MGAIMG_MAX_C, or
 * B * C * max(in_h * in_w, out_h * out_w) at or above 2^31: MGACBAM_E_SHAPE; a dtype outside the three: MGACBAM_E_DTYPE; a flag bit outside
 * the three, or reserved != 0: MGACBAM_E_ARG; dst not aligned to its element: MGACBAM_E_ALIGN.
 * Not built: LetterBox and every cv2 augmentation, antialiasing, other interpolation modes, a resize of the masks (the reference does not
 * resize them either), more than 4 channels, a gradient (the input is bytes).
 * ------------------------------------------------------------------------------------------------ */
#define MGAIMG_SRC_NHWC 1
#define MGAIMG_DST_NHWC 2
#define MGAIMG_REVERSE_C 4
#define MGAIMG_MAX_C 4
#define MGAIMG_TILE_PX 1024
#define MGAIMG_TILE_W 1024
#define MGAIMG_TILE_H 64

typedef struct mgaimg_desc {
  const uint8_t* src;                      /* (B,C,in_h,in_w), or (B,in_h,in_w,C) with MGAIMG_SRC_NHWC                               */
  void* dst;                               /* (B,C,out_h,out_w) in dtype, stored (B,out_h,out_w,C) with MGAIMG_DST_NHWC              */
  int32_t B, C, in_h, in_w, out_h, out_w;
  int32_t dtype;                           /* MGACBAM_F32 / F16 / BF16: the destination's                                            */
  int32_t flags;                           /* MGAIMG_SRC_NHWC | MGAIMG_DST_NHWC | MGAIMG_REVERSE_C                                   */
  int32_t reserved;                        /* 0                                                                                      */
} mgaimg_desc_t;

int mgaimg_run(const mgaimg_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGAIMAGE_H_ */
