// The optimizer step of the static plans (include/mgaopt.h): what the reference's trainer runs after every backward,
//   GradScaler.unscale_ -> clip_grad_norm_(10.0) -> GradScaler.step(optimizer) -> ModelEMA.update          U/engine/trainer.py:710-718
// over every parameter tensor of the slice in TWO launches instead of about a hundred.  The host builds a chunk table once: one
// (segment, offset, length <= kOptChunk) entry per workgroup, so one grid covers all segments of all levels.
//   k_opt_norm : per chunk, sum (grad * inv_scale)^2 and a non-finite flag (the value BEFORE the scaling is the one tested, as
//                _amp_foreach_non_finite_check_and_unscale_ does); workgroup 0 advances `updates`
//   k_opt_step : every workgroup sums ALL partials in index order -- a few hundred floats -- so the norm, the clip coefficient and the
//                skip decision are the same bits in every workgroup and in every run; then it updates its own chunk
// No in-launch hand-off, no spin wait, no float atomic, and no workgroup reads a word that another writes in the same launch:
//   - partial / flags: written by k_opt_norm (own entry), read by k_opt_step
//   - updates: advanced by workgroup 0 of k_opt_norm, which nobody else reads there; read by every workgroup of k_opt_step
//   - t (the count of APPLIED steps, known only in k_opt_step): two slots.  With u = updates after the advance, every workgroup reads
//     t[(u & 1) ^ 1] and workgroup 0 alone writes t[u & 1]; the next step's u has the other parity, so it reads what this one wrote
//   - the three outputs: written by workgroup 0 of k_opt_step, read by nobody on the device
// Gradient views into the bucket are only 4-byte aligned (the one after a 1-element beta): every access is a scalar, lanes along the
// elements.  At ~1e5 elements both launches are latency-bound.
#pragma once
#include "../../include/mgaopt.h"
#include "common.cuh"

namespace mgacbam {

constexpr int kOptChunk = 1024;                     // elements per workgroup
constexpr int kOptPerThread = kOptChunk / kBlock;   // 4, kBlock apart: coalesced scalar accesses
static_assert(kOptChunk == MGAOPT_CHUNK && kOptChunk % kBlock == 0, "the chunk table is built for this chunk");

struct OptChunk { int32_t seg; uint32_t off; uint32_t len; int32_t pad; };
struct OptArgs {
  const mgaopt_segment_t* segs;    // device copy of the caller's list
  const OptChunk* chunks;          // one per workgroup
  float* partial; int* flags;      // (n_chunk) each
  mgaopt_hyper_t* H;
  int n_chunk;
  int check_finite, zero_grad;
  float max_norm;
  float beta2, om_beta2, ln_beta2, eps;          // AdamW: beta2, 1 - beta2 and ln beta2 formed in double on the host
  float ema_decay, ema_om_decay, ema_inv_tau;    // ModelEMA: decay, 1 - decay (in double), 1 / tau
};

__device__ __forceinline__ bool opt_nonfinite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(kBlock) void k_opt_norm(const OptArgs A) {
  __shared__ float red[kBlock / kWave];
  const int tid = threadIdx.x;
  const OptChunk c = A.chunks[blockIdx.x];
  const float* __restrict__ g = A.segs[c.seg].grad;            // NULL: an EMA-only segment adds nothing to the norm
  const float inv_scale = A.H->inv_scale;
  float s = 0.f;
  int bad = 0;
  if (g) {
#pragma unroll
    for (int k = 0; k < kOptPerThread; ++k) {
      const uint32_t j = tid + k * kBlock;
      if (j < c.len) {
        const float raw = g[static_cast<size_t>(c.off) + j];
        bad |= opt_nonfinite(raw) ? 1 : 0;
        const float v = raw * inv_scale;
        s += v * v;
      }
    }
  }
  s = block_sum(s, tid, red);                                  // fixed order: DPP inside a wave, the four waves in order
  const int any = __syncthreads_or(bad);
  if (tid == 0) {
    A.partial[blockIdx.x] = s;
    A.flags[blockIdx.x] = any ? 1 : 0;
    if (blockIdx.x == 0) A.H->updates = A.H->updates + 1;      // ModelEMA.update: self.updates += 1, whatever the step does
  }
}

// torch's lerp (ATen/native/Lerp.h): the form that is exact at the nearer end
__device__ __forceinline__ float opt_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w); }

template <int KIND>
__global__ __launch_bounds__(kBlock) void k_opt_step(const OptArgs A) {
  const int tid = threadIdx.x;
  const mgaopt_hyper_t* __restrict__ H = A.H;
  const int u = H->updates;                                    // already advanced
  const int t_old = H->t[(u & 1) ^ 1];
  // clip_grad_norm_: the same sum, in the same order, in every workgroup
  const float* __restrict__ partial = A.partial;
  const int* __restrict__ flags = A.flags;
  float sum = 0.f;
  int found = 0;
  for (int i = 0; i < A.n_chunk; ++i) { sum += partial[i]; found |= flags[i]; }
  const float total = sqrtf(sum + H->ext_sumsq);
  const float c = A.max_norm / (total + 1e-6f);
  const float coef = c > 1.f ? 1.f : c;                        // clamp(max=1.0): a NaN norm stays a NaN coefficient, as in torch
  const bool skip = A.check_finite && (found || H->ext_found_inf != 0);     // GradScaler.step: found_inf skips optimizer.step()
  const int t = t_old + (skip ? 0 : 1);
  if (blockIdx.x == 0 && tid == 0) {
    A.H->t[u & 1] = t;
    A.H->grad_norm = total; A.H->clip_coef = coef; A.H->found_inf = found ? 1 : 0;
  }
  const OptChunk ch = A.chunks[blockIdx.x];
  const mgaopt_segment_t S = A.segs[ch.seg];
  const int grp = S.group;
  const float inv_scale = H->inv_scale, lr = H->lr[grp], mom = H->momentum[grp], wd = H->weight_decay[grp];
  float step_size = 0.f, bc2_sqrt = 1.f, om_mom = 0.f, decay_mul = 1.f;
  if constexpr (KIND == MGAOPT_ADAMW) {
    om_mom = H->one_minus_momentum[grp];
    const float tf = static_cast<float>(t);
    step_size = lr / -expm1f(tf * H->ln_momentum[grp]);        // lr / (1 - beta1^t)
    bc2_sqrt = sqrtf(-expm1f(tf * A.ln_beta2));                // sqrt(1 - beta2^t)
    decay_mul = 1.f - lr * wd;
  }
  // ModelEMA.decay(updates) = decay (1 - exp(-updates / tau)); 1 - d is formed from 1 - decay, not by cancelling against 1
  const float omd = A.ema_om_decay + A.ema_decay * expf(-static_cast<float>(u) * A.ema_inv_tau);
  const float d = 1.f - omd;
#pragma unroll
  for (int k = 0; k < kOptPerThread; ++k) {
    const uint32_t j = tid + k * kBlock;
    if (j >= ch.len) continue;
    const size_t i = static_cast<size_t>(ch.off) + j;
    float p = S.param[i];
    if (S.grad) {
      if (!skip) {
        float g = S.grad[i] * inv_scale;
        g *= coef;
        if constexpr (KIND == MGAOPT_SGD) {                    // torch/optim/sgd.py _single_tensor_sgd, nesterov, dampening 0
          g += wd * p;
          const float buf = mom * S.state0[i] + g;             // (the first step's buf = g: the same from a zero buffer)
          S.state0[i] = buf;
          g += mom * buf;
          p -= lr * g;
        } else {                                               // torch/optim/adamw.py -> adam.py _single_tensor_adam, decoupled decay
          p *= decay_mul;
          const float m = opt_lerp(S.state0[i], g, om_mom);
          const float v = A.beta2 * S.state1[i] + A.om_beta2 * g * g;
          S.state0[i] = m; S.state1[i] = v;
          const float denom = sqrtf(v) / bc2_sqrt + A.eps;
          p -= step_size * (m / denom);
        }
        S.param[i] = p;
      }
      if (A.zero_grad) S.grad[i] = 0.f;                        // optimizer.zero_grad() is unconditional (trainer.py:716)
    }
    if (S.ema) {
      float e = S.ema[i];
      e *= d;
      e += omd * p;
      S.ema[i] = e;
    }
  }
}

// one micro-step of a gradient accumulation: acc += grads, element-wise, so the order of the additions is the order of the calls
__global__ __launch_bounds__(kBlock) void k_opt_acc(float* __restrict__ acc, const float* __restrict__ grads, size_t n) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
    acc[i] += grads[i];
}

}  // namespace mgacbam
