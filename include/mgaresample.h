/* libmgacbam.so -- bilinear resampling of MaskSPADE's mask for the static plans.  include/mgaspade.h includes this file; the declarations
 * live here so that neither include/mgacbam.h (ABI 15) nor the MaskSPADE level struct and entry points change: the addition is two functions
 * and one struct.  Conventions are the library's: plain C, caller-owned buffers, nothing allocated or synchronised, every launch on the
 * stream passed in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error(). */
#ifndef MGARESAMPLE_H_
#define MGARESAMPLE_H_
#include "mgacbam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * A mask at another resolution (mga_yolo/nn/modules/masked_spade.py:102-110): F.interpolate(mode="bilinear", align_corners=False) of an
 * fp32 (B,1,in_h,in_w) tensor to (B,1,out_h,out_w), with torch's fp32 coordinate rule -- the rule the segmentation loss applies to its
 * bilinear targets -- and its exact adjoint.  One launch covers every level of a call.
 *   forward : dst (B,1,out_h,out_w) = resample(src (B,1,in_h,in_w))
 *   backward: in_h, in_w, out_h, out_w keep the forward's meaning; src is dL/d(forward dst), (B,1,out_h,out_w), and dst receives
 *             dL/d(forward src), (B,1,in_h,in_w).  Gather form, a fixed ascending order, no atomics: two runs give the same bits.
 * Every size is in 1..65536 and each tensor holds fewer than 2^31 elements (MGACBAM_E_SHAPE); pointers are 4-byte aligned
 * (MGACBAM_E_ALIGN); 1 <= n_levels <= MGACBAM_MAX_LEVELS (MGACBAM_E_LEVELS).  Every level is checked before the launch.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mgaspade_resample_level {
  const float* src;          /* read                                                               */
  float* dst;                /* written                                                            */
  int32_t B;
  int32_t in_h, in_w;        /* size of the forward's source                                       */
  int32_t out_h, out_w;      /* size of the forward's destination                                  */
} mgaspade_resample_level_t;
int mgaspade_resample_forward(const mgaspade_resample_level_t* levels, int n_levels, void* stream);
int mgaspade_resample_backward(const mgaspade_resample_level_t* levels, int n_levels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGARESAMPLE_H_ */
