/* libmgacbam.so -- the multi-scale segmentation targets (masks_multi) built on the device from the batch's full-resolution masks.  A header of
 * its own: include/mgacbam.h (ABI 15) is unchanged by it -- no struct, flag, enum or function of it moves -- and everything here follows
 * its conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed in, return
 * value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked before the first
 * launch. */
#ifndef MGATARGETS_H_
#define MGATARGETS_H_
#include "mgacbam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference's dataset does per sample on its dataloader workers (mga_yolo/data/dataset.py:94-103, MaskUtils in
 * mga_yolo/utils/mask_utils.py:29-40, 101-110) and collate_fn stacks: one binary mask per image, one target per stride.
 *   - a pixel is foreground iff its value > 0 (both element types);
 *   - the mask is zero-padded on the bottom and right up to a multiple of the stride; level l is (B, 1, ceil(H/s_l), ceil(W/s_l)) fp32;
 *   - MGATGT_AVGPOOL: (foreground pixels of the s x s block) / s^2, the divisor counting the padding   downsample_mask_prob(method="avgpool")
 *   - MGATGT_MAXPOOL: 1.0 if the block holds a foreground pixel, else 0.0                                downsample_mask, MGA_MASK_METHOD=maxpool
 *   Both are counts of at most 4096 pixels scaled by a power of two: exact in fp32, so the result equals the reference's bit for bit.
 *   - MGATGT_CLOSE3 (MAXPOOL only): a 3 x 3 dilation, then a 3 x 3 erosion of every level, neighbours outside the level ignored by both
 *     (MGA_MASK_BRIDGE: cv2.morphologyEx(MORPH_CLOSE) with its default border).  The pooling launch then writes into `scratch` and a
 *     second launch writes dst.
 * Strides: a prefix of (8, 16, 32) reads every source element once -- a lane counts an 8 x 8 cell, the 16- and 32-cells are cross-lane
 * sums -- with 8-byte (uint8, src 8-byte aligned, W % 8 == 0) or 16-byte (fp32, src 16-byte aligned, W % 4 == 0) loads, element loads
 * otherwise: src itself has no alignment requirement beyond its element's.  Any other list must be powers of two in 2..64, strictly
 * ascending; it takes one thread per destination cell.  One launch covers every level either way.
 * B, H, W >= 1 and B*H*W < 2^31 (MGACBAM_E_SHAPE); 1 <= n_levels <= MGATGT_MAX_LEVELS (MGACBAM_E_LEVELS); an unknown src_dtype is
 * MGACBAM_E_DTYPE; an unknown method, flag bit or stride list, and MGATGT_CLOSE3 with MGATGT_AVGPOOL, are MGACBAM_E_ARG; every dst must be
 * 4-byte aligned, an fp32 src as well, scratch 16-byte aligned (MGACBAM_E_ALIGN); scratch is sized by mgatgt_scratch_bytes
 * (MGACBAM_E_SIZE otherwise).
 * ------------------------------------------------------------------------------------------------ */
enum { MGACBAM_E_ARG = -7 };      /* an argument outside what the entry point takes (the codes of include/mgacbam.h end at -6) */
enum { MGATGT_AVGPOOL = 0, MGATGT_MAXPOOL = 1 };          /* mgatgt_desc_t.method    */
enum { MGATGT_SRC_U8 = 0, MGATGT_SRC_F32 = 1 };           /* mgatgt_desc_t.src_dtype */
#define MGATGT_CLOSE3 1                                    /* mgatgt_desc_t.flags     */
#define MGATGT_MAX_LEVELS 4

typedef struct mgatgt_desc {
  const void* src;                       /* (B, H, W) contiguous, uint8 or fp32                                */
  float* dst[MGATGT_MAX_LEVELS];         /* level l: (B, 1, ceil(H/stride[l]), ceil(W/stride[l])) fp32         */
  int32_t stride[MGATGT_MAX_LEVELS];
  int32_t n_levels, B, H, W;
  int32_t src_dtype;                     /* MGATGT_SRC_*                                                       */
  int32_t method;                        /* MGATGT_AVGPOOL | MGATGT_MAXPOOL                                    */
  int32_t flags;                         /* 0 | MGATGT_CLOSE3                                                  */
  int32_t reserved;                      /* 0                                                                  */
  void* scratch;                         /* MGATGT_CLOSE3 only: the unclosed levels; NULL otherwise            */
  size_t scratch_bytes;                  /* capacity of scratch (checked: MGACBAM_E_SIZE)                      */
} mgatgt_desc_t;

/* bytes of scratch the descriptor's call needs: 0 without MGATGT_CLOSE3, else every level's fp32 image, each 16-byte aligned; 0 as well
 * for a descriptor mgatgt_forward would refuse (the message then says why) */
size_t mgatgt_scratch_bytes(const mgatgt_desc_t* desc);
/* k_tgt_pool (or k_tgt_cells for the other stride lists); with MGATGT_CLOSE3 then k_tgt_close3 */
int mgatgt_forward(const mgatgt_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGATARGETS_H_ */
