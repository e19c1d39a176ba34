// libmgacbam.so, C ABI (include/mgaopt.h): the fused optimizer step over the static plans' gradient bucket
#include "host.cuh"
#include "opt.cuh"

#include <math.h>

static_assert(sizeof(mgaopt_segment_t) == 56 && sizeof(mgaopt_hyper_t) == 128 && sizeof(OptChunk) == 16, "the device tables' layout");

// The workspace: [segments][chunks][partial][flags], each 16-byte aligned; the first two are the image mgaopt_ws_init writes
struct OptLayout { size_t segs, chunks, partial, flags, total; long long n_chunk; };
static long long opt_chunks_of(int64_t n) { return (n + kOptChunk - 1) / kOptChunk; }

// everything a segment list is checked for; kind < 0: the checks that do not depend on the optimizer (the size query, the table image)
static int opt_check_segments(const char* what, const mgaopt_segment_t* segs, int n_segs, int kind, OptLayout& L) {
  if (!segs) return fail(MGACBAM_E_NULL, "%s: segs is NULL", what);
  if (n_segs < 1 || n_segs > MGAOPT_MAX_SEGMENTS) return fail(MGACBAM_E_LEVELS, "%s: n_segs=%d (1 .. %d)", what, n_segs, int(MGAOPT_MAX_SEGMENTS));
  long long n_chunk = 0;
  for (int s = 0; s < n_segs; ++s) {
    const mgaopt_segment_t& S = segs[s];
    if (!S.param) return fail(MGACBAM_E_NULL, "%s: segment %d: param is NULL", what, s);
    if (S.n < 1 || S.n > 0x7fffffffll) return fail(MGACBAM_E_SHAPE, "%s: segment %d: n=%lld (1 .. 2^31 - 1)", what, s, static_cast<long long>(S.n));
    if (S.group < 0 || S.group >= MGAOPT_GROUPS) return fail(MGACBAM_E_SHAPE, "%s: segment %d: group %d (0 .. %d)", what, s, S.group, MGAOPT_GROUPS - 1);
    if (S.grad && !S.state0) return fail(MGACBAM_E_NULL, "%s: segment %d: state0 is NULL", what, s);
    if (S.grad && kind == MGAOPT_ADAMW && !S.state1) return fail(MGACBAM_E_NULL, "%s: segment %d: AdamW needs state1 (exp_avg_sq)", what, s);
    if (!S.grad && !S.ema) return fail(MGACBAM_E_NULL, "%s: segment %d: neither grad nor ema: nothing to do", what, s);
    if (!aligned_to(S.param, 4) || !aligned_to(S.grad, 4) || !aligned_to(S.state0, 4) || !aligned_to(S.state1, 4) || !aligned_to(S.ema, 4))
      return fail(MGACBAM_E_ALIGN, "%s: segment %d: fp32 buffers must be 4-byte aligned", what, s);
    n_chunk += opt_chunks_of(S.n);
  }
  if (n_chunk > (1ll << 24)) return fail(MGACBAM_E_SHAPE, "%s: %lld chunks of %d elements (at most 2^24)", what, n_chunk, kOptChunk);
  Carver cv;
  L.segs = cv.take(static_cast<size_t>(n_segs) * (sizeof(mgaopt_segment_t) / 4));
  L.chunks = cv.take(static_cast<size_t>(n_chunk) * (sizeof(OptChunk) / 4));
  L.partial = cv.take(static_cast<size_t>(n_chunk));
  L.flags = cv.take(static_cast<size_t>(n_chunk));
  L.total = cv.total;
  L.n_chunk = n_chunk;
  return 0;
}

extern "C" size_t mgaopt_ws_bytes(const mgaopt_segment_t* segs, int n_segs) {
  OptLayout L;
  if (opt_check_segments("mgaopt_ws_bytes", segs, n_segs, -1, L)) return 0;
  g_err[0] = 0;
  return L.total;
}

extern "C" int mgaopt_ws_init(const mgaopt_segment_t* segs, int n_segs, void* host_image, size_t host_bytes) {
  OptLayout L;
  if (int e = opt_check_segments("mgaopt_ws_init", segs, n_segs, -1, L)) return e;
  if (!host_image) return fail(MGACBAM_E_NULL, "mgaopt_ws_init: host_image is NULL");
  if (int e = check_capacity("mgaopt_ws_init", "host_image", L.total, host_bytes)) return e;
  memset(host_image, 0, L.total);
  memcpy(at<char>(host_image, L.segs), segs, static_cast<size_t>(n_segs) * sizeof(mgaopt_segment_t));
  OptChunk* c = at<OptChunk>(host_image, L.chunks);
  for (int s = 0; s < n_segs; ++s)
    for (int64_t off = 0; off < segs[s].n; off += kOptChunk, ++c) {
      c->seg = s; c->off = static_cast<uint32_t>(off);
      c->len = static_cast<uint32_t>(std::min<int64_t>(kOptChunk, segs[s].n - off)); c->pad = 0;
    }
  g_err[0] = 0;
  return 0;
}

extern "C" int mgaopt_accumulate(float* acc, const float* grads, size_t n, void* stream) {
  if (!acc || !grads) return fail(MGACBAM_E_NULL, "mgaopt_accumulate: acc / grads is NULL");
  if (n < 1) return fail(MGACBAM_E_SHAPE, "mgaopt_accumulate: n=0");
  if (!aligned_to(acc, 4) || !aligned_to(grads, 4)) return fail(MGACBAM_E_ALIGN, "mgaopt_accumulate: fp32 buffers must be 4-byte aligned");
  const long long grid = static_cast<long long>(std::min<size_t>((n + kBlock - 1) / kBlock, 2048));
  if (int e = launch("k_opt_acc", k_opt_acc, grid, kBlock, 0, static_cast<hipStream_t>(stream), acc, grads, n)) return e;
  g_err[0] = 0;
  return 0;
}

extern "C" int mgaopt_step(const mgaopt_segment_t* segs, int n_segs, const mgaopt_cfg_t* cfg, mgaopt_hyper_t* hyper, void* ws, size_t ws_bytes,
                           void* stream) {
  const char* what = "mgaopt_step";
  if (!cfg) return fail(MGACBAM_E_NULL, "%s: cfg is NULL", what);
  if (cfg->kind != MGAOPT_SGD && cfg->kind != MGAOPT_ADAMW) return fail(MGACBAM_E_SHAPE, "%s: kind %d", what, cfg->kind);
  OptLayout L;
  if (int e = opt_check_segments(what, segs, n_segs, cfg->kind, L)) return e;
  if (!(cfg->max_norm > 0.0) || !(cfg->eps >= 0.0) || !(cfg->beta2 > 0.0 && cfg->beta2 < 1.0) || !(cfg->ema_tau > 0.0) ||
      !(cfg->ema_decay >= 0.0 && cfg->ema_decay <= 1.0))
    return fail(MGACBAM_E_SHAPE, "%s: max_norm=%g eps=%g beta2=%g ema_decay=%g ema_tau=%g", what, cfg->max_norm, cfg->eps, cfg->beta2,
                cfg->ema_decay, cfg->ema_tau);
  if (!hyper) return fail(MGACBAM_E_NULL, "%s: hyper is NULL", what);
  if (!aligned_to(hyper, 8)) return fail(MGACBAM_E_ALIGN, "%s: hyper must be 8-byte aligned", what);
  if (!ws) return fail(MGACBAM_E_NULL, "%s: ws is NULL", what);
  if (!aligned_to(ws, 16)) return fail(MGACBAM_E_ALIGN, "%s: ws must be 16-byte aligned", what);
  if (int e = check_capacity(what, "ws", L.total, ws_bytes)) return e;
  OptArgs A;
  A.segs = at<mgaopt_segment_t>(ws, L.segs); A.chunks = at<OptChunk>(ws, L.chunks);
  A.partial = at(ws, L.partial); A.flags = at<int>(ws, L.flags);
  A.H = hyper;
  A.n_chunk = static_cast<int>(L.n_chunk);
  A.check_finite = cfg->check_finite != 0; A.zero_grad = cfg->zero_grad != 0;
  A.max_norm = static_cast<float>(cfg->max_norm);
  A.beta2 = static_cast<float>(cfg->beta2); A.om_beta2 = static_cast<float>(1.0 - cfg->beta2); A.ln_beta2 = static_cast<float>(log(cfg->beta2));
  A.eps = static_cast<float>(cfg->eps);
  A.ema_decay = static_cast<float>(cfg->ema_decay); A.ema_om_decay = static_cast<float>(1.0 - cfg->ema_decay);
  A.ema_inv_tau = static_cast<float>(1.0 / cfg->ema_tau);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = launch("k_opt_norm", k_opt_norm, L.n_chunk, kBlock, 0, st, A)) return e;
  auto step = cfg->kind == MGAOPT_SGD ? k_opt_step<MGAOPT_SGD> : k_opt_step<MGAOPT_ADAMW>;
  if (int e = launch("k_opt_step", step, L.n_chunk, kBlock, 0, st, A)) return e;
  g_err[0] = 0;
  return 0;
}
