// ProbMaskGater on the device: the stochastic gate the reference applies to the mask before the block when
// MGA_PROB_MODE is set.                                                     mga_yolo/nn/modules/probmaskgater.py:58-98
//   p = max(clamp(p_in, 0, 1), p_min)                                        :77-79
//   gumbel : m = sigmoid((logit(clamp(p, 1e-6, 1-1e-6)) + g) / tau),  g = -log(-log U1) + log(-log U2)      :58-71, 85-87
//   hard_st: forward (m > threshold), backward that of m (straight-through)                                   :89-92
// The two uniform tensors are drawn by the caller with torch's generator exactly as the reference does (:53-56), so the kernel is
// a pure function of (p_in, U1, U2) and parity with the reference is element-wise, not statistical.  One launch instead of ~14.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr float kGateEps = 1e-6f;
struct GaterArgs {
  const float* p; const float* u1; const float* u2;   // inputs
  float* out; float* msoft;                            // forward outputs (msoft: saved for backward)
  const float* gout; float* gp;                        // backward
  size_t n;
  float inv_tau, p_min, threshold;
  int hard;
};

// The gate's arithmetic, element by element: k_pmg_fwd / k_pmg_bwd below and the multi-level kernels of gate_rng.cuh (which draw the
// uniforms themselves) call these same functions, so equal uniforms give equal bits on either path.
// p = max(clamp(p_in, 0, 1), p_min)
__device__ __forceinline__ float gate_clamp(float pin, float p_min) {
  float p = fminf(fmaxf(pin, 0.f), 1.f);
  if (p_min > 0.f) p = fmaxf(p, p_min);
  return p;
}
// the soft sample m of a clamped p and two uniforms
__device__ __forceinline__ float gate_soft(float p, float u1, float u2, float inv_tau) {
  const float a = fminf(fmaxf(u1, kGateEps), 1.f - kGateEps), b = fminf(fmaxf(u2, kGateEps), 1.f - kGateEps);
  const float q = fminf(fmaxf(p, kGateEps), 1.f - kGateEps);
  // logit(q) + g, g = -log(-log a) + log(-log b) (logistic noise), as ONE logarithm of q (-log b) / ((1 - q) (-log a)).  The four
  // terms reach 13.8 each and cancel where m is mid-range: summed in fp32 they carry about 1e-6 of rounding, which 1 / tau = 3.3
  // turns into 1e-6 of m; the quotient carries four relative roundings (3e-7) whatever the terms' size.  1 - q is exact for
  // q >= 0.5 and never below 1e-6; the quotient stays within 1e-14 .. 1e14.
  const float z = logf((q * -logf(b)) / ((1.f - q) * -logf(a))) * inv_tau;
  return 1.f / (1.f + expf(-z));
}
// does dL/dp_in pass the two clamps?  (torch's rule: inside the bounds, the bounds included)
__device__ __forceinline__ bool gate_clamp_pass(float pin, float p_min) {
  bool pass = pin >= 0.f && pin <= 1.f;
  if (p_min > 0.f) pass = pass && fminf(fmaxf(pin, 0.f), 1.f) >= p_min;
  return pass;
}
// dL/dp_in of the soft sample m (both soft modes: hard_st is straight-through)
__device__ __forceinline__ float gate_soft_bwd(float pin, float p_min, float m, float gout, float inv_tau) {
  float p = fminf(fmaxf(pin, 0.f), 1.f);
  bool pass = pin >= 0.f && pin <= 1.f;                                   // clamp(0,1) passes gradient inside, bounds included
  if (p_min > 0.f) { pass = pass && p >= p_min; p = fmaxf(p, p_min); }
  pass = pass && p >= kGateEps && p <= 1.f - kGateEps;                    // the logit's own clamp
  const float dlogit = 1.f / p + 1.f / (1.f - p);
  return pass ? gout * m * (1.f - m) * inv_tau * dlogit : 0.f;
}

// (the two kernels belong to ONE translation unit, api_eca.hip; api_gate.hip takes the functions above alone)
#ifndef MGACBAM_GATE_MATH_ONLY
__global__ __launch_bounds__(kBlock) void k_pmg_fwd(const GaterArgs A) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < A.n; i += static_cast<size_t>(gridDim.x) * kBlock) {
    const float m = gate_soft(gate_clamp(A.p[i], A.p_min), A.u1[i], A.u2[i], A.inv_tau);
    A.msoft[i] = m;
    A.out[i] = A.hard ? (m > A.threshold ? 1.f : 0.f) : m;
  }
}

__global__ __launch_bounds__(kBlock) void k_pmg_bwd(const GaterArgs A) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x; i < A.n; i += static_cast<size_t>(gridDim.x) * kBlock)
    A.gp[i] = gate_soft_bwd(A.p[i], A.p_min, A.msoft[i], A.gout[i], A.inv_tau);
}
#endif

}  // namespace mgacbam
