// ProbMaskGater for the static executors: every level of a pyramid in ONE launch each way, the noise drawn in the kernel.
//   k_gate_levels_fwd: p_in -> max(clamp(p_in, 0, 1), p_min) -> the level's mode (include/mgagate.h); the uniforms of the noisy modes are
//                      Philox4x32-10 words keyed by (seed, step, level stream, element), so the kernel reads one tensor and nothing else
//   k_gate_levels_bwd: dL/dp_in of every mode
// The arithmetic after the draw is gater.cuh's (gate_clamp, gate_soft, gate_soft_bwd): given equal uniforms both paths give equal bits.
// The noise state is device memory, int64 state[4] = {seed, step, arrivals, 0}: a captured graph replays with fresh noise because the
// forward itself advances `step` -- every workgroup reads seed and step when it starts and counts itself in `arrivals` after its last store;
// the one that arrives last (every other workgroup has read the state by then) writes step + 1 and arrivals = 0.  Nothing waits on anything.
#pragma once
#define MGACBAM_GATE_MATH_ONLY   // gater.cuh's inline arithmetic without its two kernels (they live in api_eca.hip)
#include "gater.cuh"

namespace mgacbam {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants).  Host and device compile
// this one function: the known-answer vectors are checked on the CPU (mgagate_philox4x32).
__host__ __device__ inline void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(M0) * c0, p1 = static_cast<uint64_t>(M1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1); c3 = static_cast<uint32_t>(p0); c0 = n0; c2 = n2;
    k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// The two uniforms of element i of a level: key = the seed's halves, counter = (i, stream_id, the step's halves); the top 24 bits of
// words 0 and 1 times 2^-24 -- exact in fp32, in [0, 1).  Words 2 and 3 are not used.
__host__ __device__ inline void gate_uniforms(long long seed, long long step, uint32_t stream_id, uint32_t i, float& u1, float& u2) {
  const uint64_t s = static_cast<uint64_t>(seed), t = static_cast<uint64_t>(step);
  const uint32_t key[2] = {static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32)};
  const uint32_t ctr[4] = {i, stream_id, static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  u1 = static_cast<float>(w[0] >> 8) * 5.9604644775390625e-8f;
  u2 = static_cast<float>(w[1] >> 8) * 5.9604644775390625e-8f;
}

enum GateMode { kGateDeterministic = 0, kGateGumbel = 1, kGateHardSt = 2, kGateBernoulliDetach = 3 };   // MGAGATE_* of include/mgagate.h
__host__ __device__ inline bool gate_mode_noisy(int mode) { return mode != kGateDeterministic; }

struct GateLevelArgs {
  const float* p; float* out; float* msoft;            // forward (msoft: the soft modes only)
  const float* gout; float* gp;                        // backward
  uint32_t n, stream_id;
  int mode;
  float inv_tau, p_min, threshold;
};
// Group<> (args.cuh) with room for every level a call may carry (kGroupMax is the widest launch of the feature kernels, whose argument
// blocks are ten times this size): workgroup ids [start[l], start[l+1]) belong to level l, which they sweep with a grid stride
constexpr int kGateLevelsMax = 8;
struct GateGroup {
  int n;
  int start[kGateLevelsMax + 1];
  GateLevelArgs lv[kGateLevelsMax];
  long long* state;                                    // {seed, step, arrivals, 0}
  int noisy;                                           // a level of the call draws noise: the state is read and step advances
};
__device__ __forceinline__ int gate_find_level(const GateGroup& g, int bid, int& local) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < kGateLevelsMax; ++i)
    if (i < g.n && bid >= g.start[i]) l = i;
  local = bid - g.start[l];
  return l;
}

__global__ __launch_bounds__(kBlock) void k_gate_levels_fwd(const GateGroup G) {
  int local;
  const int l = gate_find_level(G, blockIdx.x, local);
  const GateLevelArgs& A = G.lv[l];
  const size_t stride = static_cast<size_t>(G.start[l + 1] - G.start[l]) * kBlock;
  long long seed = 0, step = 0;
  if (G.noisy) {                                                                      // uniform over the launch
    seed = __hip_atomic_load(G.state + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    step = __hip_atomic_load(G.state + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const int mode = A.mode;
  for (size_t i = static_cast<size_t>(local) * kBlock + threadIdx.x; i < A.n; i += stride) {
    const float p = gate_clamp(A.p[i], A.p_min);
    float o = p;
    if (mode != kGateDeterministic) {
      float u1, u2;
      gate_uniforms(seed, step, A.stream_id, static_cast<uint32_t>(i), u1, u2);
      if (mode == kGateBernoulliDetach) {
        o = u1 < p ? 1.f : 0.f;
      } else {
        const float m = gate_soft(p, u1, u2, A.inv_tau);
        A.msoft[i] = m;
        o = mode == kGateHardSt ? (m > A.threshold ? 1.f : 0.f) : m;
      }
    }
    A.out[i] = o;
  }
  if (G.noisy) {
    __syncthreads();                                                                  // every wave has used its seed and step
    if (threadIdx.x == 0) {
      // RELAXED, agent scope: no payload travels between workgroups here -- the state words are themselves read and written with
      // agent-scope atomics (past the non-coherent caches), every value of them a workgroup uses has arrived before its stores issue,
      // hence before the barrier above and this add, and the adds of one address are performed in one order: when the last one is
      // performed every other workgroup's reads are done.  An acq_rel add is a cache write-back + invalidate in each of the ~1000
      // workgroups and measures 12-17 us of the gated step at config 2.
      const long long before = __hip_atomic_fetch_add(G.state + 2, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (before == static_cast<long long>(gridDim.x) - 1) {                          // the last arrival: nobody reads the state any more
        __hip_atomic_store(G.state + 1, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(G.state + 2, 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_gate_levels_bwd(const GateGroup G) {
  int local;
  const int l = gate_find_level(G, blockIdx.x, local);
  const GateLevelArgs& A = G.lv[l];
  const size_t stride = static_cast<size_t>(G.start[l + 1] - G.start[l]) * kBlock;
  const int mode = A.mode;
  for (size_t i = static_cast<size_t>(local) * kBlock + threadIdx.x; i < A.n; i += stride) {
    float g = 0.f;                                                                    // bernoulli_detach: the sample carries no gradient
    if (mode == kGateDeterministic) {
      g = gate_clamp_pass(A.p[i], A.p_min) ? A.gout[i] : 0.f;
    } else if (mode != kGateBernoulliDetach) {
      g = gate_soft_bwd(A.p[i], A.p_min, A.msoft[i], A.gout[i], A.inv_tau);
    }
    A.gp[i] = g;
  }
}

}  // namespace mgacbam
