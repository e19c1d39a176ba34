/* libmgacbam.so -- ProbMaskGater for a whole pyramid, with the noise drawn on the device.  A header of its own: include/mgacbam.h (ABI 15)
 * is unchanged by it -- no struct, flag, enum or function of it moves -- and everything here follows its conventions: plain C,
 * caller-owned buffers, nothing allocated or synchronised, every launch on the stream passed in, return value 0 / MGACBAM_E_* /
 * hipError_t, the message of a failure through mgacbam_last_error().  Every argument of every level is checked before the first launch. */
#ifndef MGAGATE_H_
#define MGAGATE_H_
#include "mgacbam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The gate of mga_yolo/nn/modules/probmaskgater.py on up to MGACBAM_MAX_LEVELS levels, ONE launch per direction.  Per element
 *   p = max(clamp(p_in, 0, 1), p_min)     (p_min applied when > 0)
 * and then the level's mode:
 *   MGAGATE_DETERMINISTIC     out = p (also what an eval-mode gate returns)          backward: the clamps' pass-through
 *   MGAGATE_GUMBEL            out = m = sigmoid((logit(p) + logistic(u1, u2)) / tau)  backward: dm/dp_in
 *   MGAGATE_HARD_ST           out = (m > threshold), m kept in msoft                  backward: that of m (straight-through)
 *   MGAGATE_BERNOULLI_DETACH  out = (u1 < p)                                          backward: zeros
 * m is mgapmg_forward's arithmetic: given equal uniforms the two give equal bits, and so do the two backwards.
 *
 * The uniforms are Philox4x32-10 words: key = (seed & 0xffffffff, seed >> 32), counter = (i, stream_id, step & 0xffffffff, step >> 32)
 * with i the flat element index inside the level; u1 = (word0 >> 8) * 2^-24, u2 = (word1 >> 8) * 2^-24 (exact in fp32, in [0, 1));
 * words 2 and 3 are discarded.  The stream is this library's own: statistically, not bitwise, what torch's generator gives.
 *
 * state: int64[4] in device memory, {seed, step, arrivals, 0}, 8-byte aligned; the caller sets seed and step and zero-fills the rest
 * once.  A forward in which at least one level's mode draws noise reads seed and step and leaves step + 1 behind (arrivals is its
 * scratch and is 0 again when it ends), so a captured graph replays with fresh noise; a forward of deterministic levels only does
 * not touch the state.  The backward does not read it.  Calls that share a state must be ordered on the device (one stream).
 * ------------------------------------------------------------------------------------------------ */
enum { MGAGATE_DETERMINISTIC = 0, MGAGATE_GUMBEL = 1, MGAGATE_HARD_ST = 2, MGAGATE_BERNOULLI_DETACH = 3 };
typedef struct mgagate_level {
  const float* p;            /* (n) fp32: the gate's input, both directions                          */
  float* out;                /* forward: (n) the gated mask                                          */
  float* msoft;              /* GUMBEL / HARD_ST: (n) the soft sample, written forward, read backward */
  const float* gout;         /* backward: dL/dout (n)                                                */
  float* gp;                 /* backward: dL/dp (n)                                                  */
  uint32_t n;                /* elements, >= 1                                                       */
  int32_t mode;              /* MGAGATE_*                                                            */
  int32_t stream_id;         /* counter word 1: levels of one call take different values             */
  float tau, p_min, threshold; /* tau > 0                                                            */
} mgagate_level_t;
int mgagate_forward(const mgagate_level_t* levels, int n_levels, int64_t* state, void* stream);
int mgagate_backward(const mgagate_level_t* levels, int n_levels, void* stream);
/* Host only, for tests: the same inline Philox the kernels compile, run on the CPU. */
void mgagate_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
void mgagate_uniforms(int64_t seed, int64_t step, int32_t stream_id, uint32_t i, float out[2]);

#ifdef __cplusplus
}
#endif
#endif /* MGAGATE_H_ */
