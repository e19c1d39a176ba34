// libmgacbam.so, C ABI (include/mgagate.h): ProbMaskGater on a whole pyramid, the noise drawn in the kernel
#include "host.cuh"
#include "../../include/mgagate.h"
#include "gate_rng.cuh"

static_assert(kGateLevelsMax == MGACBAM_MAX_LEVELS, "GateGroup holds every level a call may carry");
static_assert(int(kGateDeterministic) == int(MGAGATE_DETERMINISTIC) && int(kGateGumbel) == int(MGAGATE_GUMBEL) &&
              int(kGateHardSt) == int(MGAGATE_HARD_ST) && int(kGateBernoulliDetach) == int(MGAGATE_BERNOULLI_DETACH),
              "gate_rng.cuh restates the header's modes");

// workgroups of a level: one element per thread up to the cap, a grid stride beyond it
static int gate_blocks(uint32_t n) { return static_cast<int>(std::min<uint64_t>((static_cast<uint64_t>(n) + kBlock - 1) / kBlock, 2048)); }

// everything a level is checked for before the first launch, and its kernel arguments
static int gate_level(const char* what, int l, const mgagate_level_t& L, bool bwd, GateLevelArgs& A) {
  if (L.mode < MGAGATE_DETERMINISTIC || L.mode > MGAGATE_BERNOULLI_DETACH) return fail(MGACBAM_E_SHAPE, "%s: level %d: mode %d", what, l, L.mode);
  const bool soft = L.mode == MGAGATE_GUMBEL || L.mode == MGAGATE_HARD_ST;
  if (!L.p) return fail(MGACBAM_E_NULL, "%s: level %d: p is NULL", what, l);
  if (!bwd && !L.out) return fail(MGACBAM_E_NULL, "%s: level %d: out is NULL", what, l);
  if (bwd && (!L.gout || !L.gp)) return fail(MGACBAM_E_NULL, "%s: level %d: gout / gp is NULL", what, l);
  if (soft && !L.msoft) return fail(MGACBAM_E_NULL, "%s: level %d: the soft modes need msoft", what, l);
  if (L.n < 1) return fail(MGACBAM_E_SHAPE, "%s: level %d: n=0", what, l);
  if (!(L.tau > 0.f)) return fail(MGACBAM_E_SHAPE, "%s: level %d: tau=%g must be > 0", what, l, L.tau);
  if (!aligned_to(L.p, 4) || !aligned_to(L.out, 4) || !aligned_to(L.msoft, 4) || !aligned_to(L.gout, 4) || !aligned_to(L.gp, 4))
    return fail(MGACBAM_E_ALIGN, "%s: level %d: fp32 buffers must be 4-byte aligned", what, l);
  A.p = L.p; A.out = L.out; A.msoft = L.msoft; A.gout = L.gout; A.gp = L.gp;
  A.n = L.n; A.stream_id = static_cast<uint32_t>(L.stream_id); A.mode = L.mode;
  A.inv_tau = 1.f / L.tau; A.p_min = L.p_min; A.threshold = L.threshold;
  return 0;
}
static int gate_group(const char* what, const mgagate_level_t* levels, int n_levels, bool bwd, GateGroup& G, int& grid) {
  if (!levels) return fail(MGACBAM_E_NULL, "%s: levels is NULL", what);
  if (n_levels < 1 || n_levels > MGACBAM_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "%s: n_levels=%d", what, n_levels);
  G.n = n_levels; G.state = nullptr; G.noisy = 0;
  grid = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (int e = gate_level(what, l, levels[l], bwd, G.lv[l])) return e;
    G.noisy = G.noisy || gate_mode_noisy(levels[l].mode);
    G.start[l] = grid;
    grid += gate_blocks(levels[l].n);
  }
  for (int l = n_levels; l <= kGateLevelsMax; ++l) G.start[l] = grid;
  return 0;
}

extern "C" int mgagate_forward(const mgagate_level_t* levels, int n_levels, int64_t* state, void* stream) {
  GateGroup G;
  int grid;
  if (int e = gate_group("mgagate_forward", levels, n_levels, false, G, grid)) return e;
  if (!state) return fail(MGACBAM_E_NULL, "mgagate_forward: state is NULL");
  if (!aligned_to(state, 8)) return fail(MGACBAM_E_ALIGN, "mgagate_forward: state must be 8-byte aligned");
  G.state = reinterpret_cast<long long*>(state);
  if (int e = launch("k_gate_levels_fwd", k_gate_levels_fwd, grid, kBlock, 0, static_cast<hipStream_t>(stream), G)) return e;
  g_err[0] = 0;
  return 0;
}
extern "C" int mgagate_backward(const mgagate_level_t* levels, int n_levels, void* stream) {
  GateGroup G;
  int grid;
  if (int e = gate_group("mgagate_backward", levels, n_levels, true, G, grid)) return e;
  G.noisy = 0;
  if (int e = launch("k_gate_levels_bwd", k_gate_levels_bwd, grid, kBlock, 0, static_cast<hipStream_t>(stream), G)) return e;
  g_err[0] = 0;
  return 0;
}

extern "C" void mgagate_philox4x32(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  const uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
  uint32_t w[4];
  philox4x32_10(c, k, w);
  for (int j = 0; j < 4; ++j) out[j] = w[j];
}
extern "C" void mgagate_uniforms(int64_t seed, int64_t step, int32_t stream_id, uint32_t i, float out[2]) {
  gate_uniforms(seed, step, static_cast<uint32_t>(stream_id), i, out[0], out[1]);
}
