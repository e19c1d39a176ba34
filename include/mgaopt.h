/* libmgacbam.so -- the optimizer step of the static plans, fused over their flat gradient bucket.  A header of its own: include/mgacbam.h
 * (ABI 15) is unchanged by it -- no struct, flag, enum or function of it moves -- and everything here follows its conventions: plain C,
 * caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed in, return value 0 / MGACBAM_E_* /
 * hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked before the first launch. */
#ifndef MGAOPT_H_
#define MGAOPT_H_
#include "mgacbam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference's trainer does after every backward (U/engine/trainer.py:710-718), over every segment in TWO launches:
 *   1. g = grad * inv_scale; a non-finite grad (tested before the scaling) sets found_inf     GradScaler.unscale_
 *   2. total = sqrt(sum g^2 over every segment + ext_sumsq)                                    clip_grad_norm_(max_norm)
 *   3. coef = min(1, max_norm / (total + 1e-6)); g *= coef
 *   4. check_finite and (found_inf or ext_found_inf): parameters, state and the applied-step count t stay bit for bit (GradScaler.step
 *      skips); the EMA and `updates` advance all the same (trainer.py:717 is unconditional)
 *   5. MGAOPT_SGD   = torch.optim.SGD(nesterov=True):  g += wd p;  buf = m buf + g;  g += m buf;  p -= lr g
 *      MGAOPT_ADAMW = torch.optim.AdamW(betas=(m, beta2), eps):  p *= 1 - lr wd;  exp_avg = lerp(exp_avg, g, 1 - m);
 *                     exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2;  t += 1;  p -= (lr / (1 - m^t)) exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^t) + eps)
 *      with 1 - b^t formed as -expm1(t ln b), which is accurate at small t in fp32
 *   6. updates += 1;  d = ema_decay (1 - exp(-updates / ema_tau));  ema = d ema + (1 - d) p      ModelEMA.update (U/utils/torch_utils.py:759-775)
 * lr, m (momentum / beta1) and wd are per group, in the order of optimizer.param_groups after build_optimizer (trainer.py:915-941):
 * group 0 the biases (no decay), group 1 the weights with decay, group 2 the weights of normalisation modules (no decay).
 *
 * Everything that changes from step to step is read from the device-resident mgaopt_hyper_t, so a captured graph replays without
 * re-capture; the host writes it between replays.  Two runs from the same state give the same bits: sums are formed in a fixed order.
 * ------------------------------------------------------------------------------------------------ */
enum { MGAOPT_SGD = 0, MGAOPT_ADAMW = 1 };
enum { MGAOPT_GROUPS = 3, MGAOPT_MAX_SEGMENTS = 4096, MGAOPT_CHUNK = 1024 };

typedef struct mgaopt_segment {
  float* param;              /* (n) fp32, updated in place; of an EMA-only segment: the buffer that is averaged    */
  float* grad;               /* (n) fp32, or NULL: an EMA-only segment (a floating-point buffer ModelEMA averages) */
  float* state0;             /* (n) SGD: the momentum buffer, AdamW: exp_avg; zero-filled once by the caller       */
  float* state1;             /* (n) AdamW: exp_avg_sq, zero-filled once; NULL for SGD                              */
  float* ema;                /* (n) the average, or NULL: none kept                                                */
  int64_t n;                 /* elements, 1 .. 2^31 - 1                                                            */
  int32_t group;             /* 0 .. MGAOPT_GROUPS - 1                                                             */
  int32_t reserved;          /* 0                                                                                  */
} mgaopt_segment_t;

typedef struct mgaopt_cfg {
  int32_t kind;              /* MGAOPT_SGD | MGAOPT_ADAMW                                                          */
  int32_t check_finite;      /* 1: step 4's skip (a GradScaler run); 0: the step is always applied                 */
  int32_t zero_grad;         /* 1: every grad word is left 0 (grad is the accumulator of mgaopt_accumulate)        */
  int32_t reserved;          /* 0                                                                                  */
  double beta2, eps;         /* AdamW: 0.999, 1e-8                                                                 */
  double max_norm;           /* 10.0 (trainer.py:713)                                                              */
  double ema_decay, ema_tau; /* 0.9999, 2000 (ModelEMA's defaults)                                                 */
} mgaopt_cfg_t;

/* Device memory, 8-byte aligned, written by the host between steps (the doubles of torch's Python side rounded once to fp32):
 * one_minus_momentum = 1 - m and ln_momentum = ln m are formed in double.  updates and t are the library's: zero-filled once.
 * t[updates & 1] is the count of steps applied so far; the other slot is what the next step writes.                              */
typedef struct mgaopt_hyper {
  float lr[MGAOPT_GROUPS], momentum[MGAOPT_GROUPS], one_minus_momentum[MGAOPT_GROUPS], ln_momentum[MGAOPT_GROUPS], weight_decay[MGAOPT_GROUPS];
  float inv_scale;           /* 1 / the loss scale; 1 without a scaler                                             */
  float ext_sumsq;           /* squared norm (after unscaling) of the gradients outside the segments; 0 if none    */
  int32_t ext_found_inf;     /* non-zero: a gradient outside the segments was non-finite                           */
  int32_t updates;           /* EMA updates = calls of mgaopt_step so far                                          */
  int32_t t[2];              /* applied steps, two slots (see above)                                               */
  float grad_norm;           /* out: total, before clipping                                                        */
  float clip_coef;           /* out: coef                                                                          */
  int32_t found_inf;         /* out: 1 if a segment's grad was non-finite (ext_found_inf is not folded in)         */
  int32_t reserved[8];
} mgaopt_hyper_t;

/* The workspace holds the device-resident tables (segments; one (segment, offset, length <= MGAOPT_CHUNK) entry per workgroup) and the
 * per-chunk partials.  mgaopt_ws_bytes: its size, 0 for a segment list mgaopt_step would refuse.  mgaopt_ws_init writes the image of
 * the tables into HOST memory of that size; the caller copies it to the device workspace once (16-byte aligned), and again whenever a
 * pointer or length of the list changes.  mgaopt_step checks the list it is given, not the device copy. */
size_t mgaopt_ws_bytes(const mgaopt_segment_t* segs, int n_segs);
int mgaopt_ws_init(const mgaopt_segment_t* segs, int n_segs, void* host_image, size_t host_bytes);
/* acc[i] += grads[i], i < n: one launch, element-wise (one micro-step of a gradient accumulation) */
int mgaopt_accumulate(float* acc, const float* grads, size_t n, void* stream);
/* the step above: k_opt_norm, k_opt_step */
int mgaopt_step(const mgaopt_segment_t* segs, int n_segs, const mgaopt_cfg_t* cfg, mgaopt_hyper_t* hyper, void* ws, size_t ws_bytes,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGAOPT_H_ */
