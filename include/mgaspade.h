/* libmgacbam.so -- the MaskSPADE entry points.  A header of its own: include/mgacbam.h (ABI 15) is unchanged by them -- no struct, flag,
 * enum or function of it moves -- and everything here follows its conventions: plain C, caller-owned buffers that travel with their
 * capacities, nothing allocated or synchronised, every launch on the stream passed in, return value 0 / MGACBAM_E_* / hipError_t, the
 * message of a failure through mgacbam_last_error(). */
#ifndef MGASPADE_H_
#define MGASPADE_H_
#include "mgacbam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * MaskSPADE: mga_yolo/nn/modules/masked_spade.py.  y = gamma(s) * norm(x) + beta(s), s = sigmoid(mask) (or the mask itself),
 * h = relu(conv3x3(s)), gamma = conv3x3(h; wg) + bg, beta = conv3x3(h; wb) + bb; norm = instance norm, or batch norm (batch statistics
 * and a running-statistics update when `training`, the running statistics otherwise).  The two hidden -> C convolutions run on the matrix
 * cores (fp32 features: v_mfma_f32_16x16x4_f32; fp16 / bf16: the native 16x16x16 forms, fp32 accumulation) fused with the FiLM apply.
 * One struct serves both directions; a direction ignores the other's pointers.  x / y / gy / gx of `dtype` are NCHW-contiguous, or with
 * MGASPADE_LAYOUT_NHWC in `flags` dense (B,H,W,C) (torch's channels_last); the mask, gmask, the parameters, their gradients and the
 * running statistics are the same memory in both layouts, and so are the sizes of ctx and scratch.  A channels-last level returns, bit
 * for bit, what the same data returns as an NCHW level.  The gamma kept in ctx has the level's layout: a backward must carry the flag
 * its forward carried.  Levels of both layouts may share a call.  The mask is
 * (B,1,H,W) fp32 at the feature's size or NULL (then y = norm(x) and no parameter is read); parameters and their gradients fp32.
 * hidden % 16 == 0, hidden <= 64, C % 16 == 0, C <= 1024 (MGACBAM_E_SHAPE otherwise).  x, y, gy, gx, ctx and scratch must be 16-byte
 * aligned (MGACBAM_E_ALIGN).  save_gamma: the forward keeps gamma (feature dtype) in ctx for the backward, which then needs the ctx of
 * such a forward.  Every argument is checked before the first launch; nothing is allocated or synchronised.
 * ------------------------------------------------------------------------------------------------ */
enum { MGASPADE_NORM_IN = 0, MGASPADE_NORM_BN = 1 };
enum { MGASPADE_LAYOUT_NHWC = 2 };   /* mgaspade_level_t.flags; the value of MGACBAM_LAYOUT_NHWC.  Every other bit: MGACBAM_E_SHAPE */
typedef struct mgaspade_level {
  const void* x;             /* (B,C,H,W) dtype; x, y, gy, gx: (B,H,W,C) with MGASPADE_LAYOUT_NHWC  */
  const float* mask;         /* (B,1,H,W) fp32 or NULL                                             */
  void* y;                   /* forward: (B,C,H,W) dtype                                           */
  const void* gy;            /* backward: dL/dy (B,C,H,W) dtype                                    */
  void* gx;                  /* backward: dL/dx (B,C,H,W) dtype                                    */
  float* gmask;              /* backward: dL/dmask (B,1,H,W) fp32, or NULL (not wanted)            */
  const float* w0;           /* shared.0.weight (hidden,1,3,3)                                     */
  const float* b0;           /* shared.0.bias (hidden)                                             */
  const float* wg;           /* conv_gamma.weight (C,hidden,3,3)                                   */
  const float* bg;           /* conv_gamma.bias (C)                                                */
  const float* wb;           /* conv_beta.weight (C,hidden,3,3)                                    */
  const float* bb;           /* conv_beta.bias (C)                                                 */
  float* running_mean;       /* batch norm: (C), updated by a training forward; else NULL          */
  float* running_var;        /* batch norm: (C)                                                    */
  long long* num_batches_tracked; /* batch norm: int64 scalar or NULL                              */
  float* gw0;                /* backward with a mask: the six parameter gradients, same shapes     */
  float* gb0;
  float* gwg;
  float* gbg;
  float* gwb;
  float* gbb;
  void* ctx;                 /* saved by the forward, read by the backward                         */
  size_t ctx_bytes;          /* capacity of ctx (checked: MGACBAM_E_SIZE)                          */
  void* scratch;             /* backward transients                                                */
  size_t scratch_bytes;      /* capacity of scratch (checked: MGACBAM_E_SIZE)                      */
  int32_t B, C, H, W, hidden;
  int32_t dtype;             /* MGACBAM_F32 / F16 / BF16                                           */
  int32_t norm_type;         /* MGASPADE_NORM_IN / MGASPADE_NORM_BN                                */
  int32_t training;          /* batch norm only: batch statistics + running update                 */
  int32_t use_sigmoid_mask;
  int32_t save_gamma;        /* forward: keep gamma in ctx (a backward will follow)                */
  float eps, momentum;
  int32_t flags;             /* 0 or MGASPADE_LAYOUT_NHWC                                          */
} mgaspade_level_t;
size_t mgaspade_ctx_bytes(int B, int C, int H, int W, int hidden);       /* covers every dtype, with save_gamma; 0 on a bad shape */
size_t mgaspade_scratch_bytes(int B, int C, int H, int W, int hidden);
int mgaspade_forward(const mgaspade_level_t* levels, int n_levels, void* stream);
int mgaspade_backward(const mgaspade_level_t* levels, int n_levels, void* stream);

#ifdef __cplusplus
}
#endif

/* The mask resample of the static plans (a mask given at another resolution): declared in a file of its own, which this header brings in,
 * so that the declarations above stay exactly as they were. */
#include "mgaresample.h"
#endif /* MGASPADE_H_ */
