// Host side shared by every translation unit of libmgacbam.so (api_*.hip): error reporting, launch helper, knobs, ctx / scratch
// layouts, launch geometry and the level-grouping of the grouped launches.  The library is built from several translation units
// (one per kernel family) so that they compile in parallel and an edit rebuilds one family; the state they share (the thread-local
// error string, the knobs) is C++17 inline data: ONE instance per process.
// No allocation, no host<->device copy, no synchronisation anywhere: every entry point only enqueues kernels on the caller's
// stream, so calls are re-entrant and graph-capturable.
#pragma once
#include "../../include/mgacbam.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "args.cuh"
#include "common.cuh"

using namespace mgacbam;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
inline thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
// Every launch goes through hipLaunchKernel, here and nowhere else, and its OWN return value is checked: the process-wide sticky
// error state (which may hold an asynchronous error of the framework's kernels on this thread) is neither read nor cleared.
// The arguments are taken as the kernel's own parameter types (a Group by reference: no copy), so a wrong one does not compile.
template <typename... P>
static int launch(const char* what, void (*kernel)(P...), long long grid, int block, size_t smem, hipStream_t st,
                  const std::common_type_t<P>&... args) {
  void* p[] = {const_cast<void*>(static_cast<const void*>(&args))...};
  const hipError_t e = hipLaunchKernel(reinterpret_cast<const void*>(kernel), dim3(static_cast<unsigned>(grid)), dim3(block), p, smem, st);
  if (e != hipSuccess) return fail(static_cast<int>(e), "%s: %s", what, hipGetErrorString(e));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// layouts
// ------------------------------------------------------------------------------------------------
static int check_shape(int B, int C, int H, int W, int hidden, int k) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || hidden < 1 || hidden > 4096 || C > 65536)
    return fail(MGACBAM_E_SHAPE, "bad shape B=%d C=%d H=%d W=%d hidden=%d", B, C, H, W, hidden);
  if (static_cast<long long>(H) * W > (1ll << 30) || static_cast<long long>(B) * C * H * W > (1ll << 40))
    return fail(MGACBAM_E_SHAPE, "tensor too large B=%d C=%d H=%d W=%d", B, C, H, W);
  if (k < 1 || k > 15 || (k & 1) == 0) return fail(MGACBAM_E_SHAPE, "spatial kernel k=%d must be odd and in 1..15", k);
  return 0;
}

// The hand-off region of the ctx (CtxPtrs::sync), in ints from its start; every word is a generation counter.  nflag flags per sample: one
// per tile of >= kSyncPx pixels, whatever tile size the launch geometry picks.  The merged backward launch (k_bwd_r12) has tile /
// conv-tile flags of its OWN beside its dWsa-tile and sweep flags: every class of counters is bumped exactly once per launch of its
// kind, so the two launch forms can alternate on one ctx without their counters drifting apart.  (_lib.sync_regions mirrors this.)
struct SyncLayout {
  size_t nflag;
  size_t gate;               // [B][nflag] k_gate tile flags
  size_t status;             // 4 status words, [0] = time-out
  size_t ca;                 // [B] per-sample ca flags
  size_t bflag, cflag;       // [B][nflag] k_bwd_reduce1 tile flags, [B][nflag] folded conv-tile flags
  size_t mbflag, mcflag;     // the same two of the merged launch
  size_t wflag, sflag;       // the merged launch's [B][nflag] dWsa-tile flags and [B][C] per-channel sweep flags
  size_t arrive;             // [B][kArriveStride], word 0 of each: k_pool's arrival count of the sample (FwdArgs::pool_mlp), 0 between launches
  size_t len;
};
static SyncLayout sync_layout(int B, int C, size_t HW) {
  SyncLayout S;
  S.nflag = (HW + kSyncPx - 1) / kSyncPx + 1;
  const size_t per = static_cast<size_t>(B) * S.nflag;
  S.gate = 0; S.status = per; S.ca = S.status + 4; S.bflag = S.ca + B;
  S.cflag = S.bflag + per; S.mbflag = S.cflag + per; S.mcflag = S.mbflag + per; S.wflag = S.mcflag + per; S.sflag = S.wflag + per;
  S.arrive = S.sflag + static_cast<size_t>(B) * C;           // appended: every older offset is where it was
  S.len = S.arrive + static_cast<size_t>(B) * kArriveStride;
  return S;
}

// Carves a work buffer into 16-byte aligned fields of 4-byte elements, in the order they are taken (every ctx / scratch layout of the
// library); at<T>: the field at a byte offset of a caller's buffer
struct Carver {
  size_t total = 0;
  size_t take(size_t n_elems) { const size_t off = total; total = align16(total + n_elems * 4); return off; }
};
template <typename T = float>
static T* at(const void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(const_cast<void*>(base)) + off); }

static void ctx_layout(int B, int C, int H, int W, int hidden, mgacbam_ctx_layout_t* L) {
  const size_t HW = static_cast<size_t>(H) * W, BC = static_cast<size_t>(B) * C;
  Carver cv;                                                    // (its size_t offsets become the ABI struct's int64_t)
  L->S = cv.take(B); L->use = cv.take(B); L->den = cv.take(B);
  L->avg = cv.take(BC); L->mx = cv.take(BC); L->mavg = cv.take(BC);
  L->valid = cv.take(BC); L->amax = cv.take(BC);
  L->h_avg = cv.take(static_cast<size_t>(B) * hidden); L->h_mx = cv.take(static_cast<size_t>(B) * hidden);
  L->ca = cv.take(BC);
  L->planes = cv.take(static_cast<size_t>(B) * 3 * HW);
  L->cidx = cv.take(static_cast<size_t>(B) * HW);
  L->sa = cv.take(static_cast<size_t>(B) * HW);
  L->proj = cv.take(hidden <= MGACBAM_PROJ_MAX_HIDDEN ? static_cast<size_t>(B) * hidden * HW : 0);
  const SyncLayout S = sync_layout(B, C, HW);
  L->sync = cv.take(S.len);
  L->status = L->sync + static_cast<int64_t>(4 * S.status);
  L->total = static_cast<int64_t>(cv.total);
}

static CtxPtrs ctx_ptrs(void* p, int B, int C, int H, int W, int hidden) {
  mgacbam_ctx_layout_t L;
  ctx_layout(B, C, H, W, hidden, &L);
  return CtxPtrs{at(p, L.S), at(p, L.use), at(p, L.den), at(p, L.avg), at(p, L.mx), at(p, L.mavg), at<int>(p, L.valid), at<int>(p, L.amax),
                 at(p, L.h_avg), at(p, L.h_mx), at(p, L.ca), at(p, L.planes), at<int>(p, L.cidx), at(p, L.sa), at(p, L.proj), at<int>(p, L.sync)};
}

// ------------------------------------------------------------------------------------------------
// launch geometry
// ------------------------------------------------------------------------------------------------
static int pow2_floor(int v) { int p = 1; while (p * 2 <= v) p *= 2; return p; }
static int pow2_ceil(int v) { int p = 1; while (p < v) p *= 2; return p; }
static int env_int(const char* name, int dflt) {
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}
// Tuning / test knobs come from the environment ONCE (first call) -- not per call: the eager path makes ~50 look-ups per step
// otherwise.  mgacbam_reload_env() re-reads them (tests and tuning sweeps that change the environment in-process).
struct Knobs {
  int bwd_merge;           // MGACBAM_BWD_MERGE (default 1): k_bwd_reduce1 + conv + dWsa tiles + k_bwd_reduce2 as one launch (k_bwd_r12)
  int gate_narrow;         // MGACBAM_GATE_NARROW (default 0): k_gate also for tiles narrower than an image row
  int pool_tx, pool_cpt, chan_tx;   // MGACBAM_POOL_TX / _POOL_CPT / _CHAN_TX: launch-geometry overrides (choose_tune, group_cpt)
  int resident_wgs;        // MGACBAM_RESIDENT_WGS: override of the co-resident workgroup budget the hand-off eligibility is sized from
  int fault;               // MGACBAM_FAULT: fault injection for tests (args.cuh)
  int pool_mlp;            // MGACBAM_POOL_MLP: 0 = k_pool never forms ca, unset = by the rule (pool_forms_ca), 2 = at every level whose shape
                           // the tail takes, however small (tests)
  unsigned spin_limit;     // MGACBAM_SPIN_LIMIT
  long long* trace;        // MGACBAM_TRACE_PTR (-DMGACBAM_TRACE builds, tools/trace_gate.py)
};
static Knobs read_knobs() {
  Knobs k;
  k.bwd_merge = env_int("MGACBAM_BWD_MERGE", 1);
  k.gate_narrow = env_int("MGACBAM_GATE_NARROW", 0);
  k.pool_tx = env_int("MGACBAM_POOL_TX", 0); k.pool_cpt = env_int("MGACBAM_POOL_CPT", 0); k.chan_tx = env_int("MGACBAM_CHAN_TX", 0);
  k.resident_wgs = env_int("MGACBAM_RESIDENT_WGS", 0); k.fault = env_int("MGACBAM_FAULT", 0);
  k.pool_mlp = env_int("MGACBAM_POOL_MLP", 1);
  const int sl = env_int("MGACBAM_SPIN_LIMIT", 0);
  k.spin_limit = sl > 0 ? static_cast<unsigned>(sl) : (1u << 20);
  const char* tp = getenv("MGACBAM_TRACE_PTR");
  k.trace = (tp && *tp) ? reinterpret_cast<long long*>(strtoull(tp, nullptr, 0)) : nullptr;
  return k;
}
inline std::mutex g_knob_mu;
inline Knobs g_knobs;
inline std::atomic<bool> g_knobs_ready{false};
static Knobs knobs() {
  if (!g_knobs_ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lk(g_knob_mu);
    if (!g_knobs_ready.load(std::memory_order_relaxed)) { g_knobs = read_knobs(); g_knobs_ready.store(true, std::memory_order_release); }
  }
  return g_knobs;   // (written once under the lock before the flag; mgacbam_reload_env is documented as not concurrent with calls)
}

// Co-resident workgroups of a kernel on the current device = CUs x blocks per CU (occupancy API, for the chosen instantiation and
// its dynamic LDS).  This is what bounds the in-launch hand-off of k_gate: a tile waits for tiles up to 8*span ids AHEAD, and with
// in-order dispatch the lowest unfinished workgroup's producers are dispatched iff 8*span + 1 workgroups fit on the device together.
static int device_cus() {
  static std::mutex mu;
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  std::lock_guard<std::mutex> lk(mu);
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
    cus[dev] = n > 0 ? n : -1;
  }
  return cus[dev] > 0 ? cus[dev] : 0;
}
template <typename K>
static int resident_workgroups(K kernel, size_t smem) {
  const int forced = knobs().resident_wgs;
  if (forced > 0) return forced;
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> cache;
  const auto key = std::make_pair(reinterpret_cast<const void*>(kernel), smem);
  int per_cu = -1;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) per_cu = it->second;
  }
  if (per_cu < 0) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kBlock, smem) != hipSuccess) n = 0;
    per_cu = n;
    std::lock_guard<std::mutex> lk(mu);
    cache[key] = per_cu;
  }
  return per_cu * device_cus();
}
static bool is_pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// elements per lane per access: 4 (16 B fp32, 8 B fp16/bf16) when the row length allows, else scalar.  8-element (16 B) half
// vectors halve the tile count, which starves the small levels (P5: 128 workgroups; k_chan 19 -> 33 us at YOLOv8n sizes): only
// k_gate reads them (forward_args: gvec)
static int vec_of(int H, int W) { return (static_cast<long long>(H) * W) % 4 == 0 ? 4 : 1; }

// k_gate (x-resident chan+apply): every thread keeps kGateR channels, so TY = ceil(C / kGateR) slices (power of two) and the
// rest of the 256 threads go along H*W.  Eligible when a tile is >= kSyncPx pixels (ctx.sync has one flag per kSyncPx) and >= one
// image row, the tiles a k x k window reaches are few (their workgroups must be co-resident: 8 ids apart per tile, common.cuh)
// and the staged rows fit in LDS; otherwise the three-launch forward runs.
static void gate_geometry(int C, int H, int W, int k, int VEC, Tune& t) {
  t.gate_tx = 0; t.gate_rows = 0; t.gate_span = 0;
  const int gty = pow2_ceil((C + kGateR - 1) / kGateR);
  if (gty > kBlock) return;
  const int gtx = kBlock / gty, TP = gtx * VEC;
  int grows = (TP - 1) / W + 2;
  if (grows > H) grows = H;
  grows += k - 1;
  const int span = ((k / 2) * W + TP - 1) / TP + 1;           // tiles reached on either side
  const size_t lds = (3 * static_cast<size_t>(grows) * (W + k - 1) + TP + 3 * k * k + 3 * C + 64) * sizeof(float);
  // TP < W (wide feature maps at C >= 256: a tile is a fraction of an image row).  Supported -- a tile inside one row stages and waits
  // for only the columns its windows reach (fwd.cuh: `narrow`), parity-tested -- but OPT-IN (MGACBAM_GATE_NARROW=1): at BASELINE
  // configs[3] it measures 224 us against 201 us for k_mlp + k_chan + k_apply.  tools/trace_gate.py fwd cfg4: a 64- / 32-pixel tile
  // needs rows of up to 3 below it, i.e. tiles 7-8 positions AHEAD in dispatch order, and sits 6.8 us (p90 11) waiting for them to be
  // scheduled and to reach their publish point; the TY = 16 / 32 channel slices combine through LDS in 5.2 us; the C = 512 role MLP
  // takes 20 us for the first round; 60 % of the resident workgroups are in the chain at any time and HBM runs at 3 TB/s
  // (whether the 8*span + 1 workgroups a tile's wait spans are co-resident on THIS device is checked at dispatch: forward_group)
  if (TP >= kSyncPx && (TP >= W || knobs().gate_narrow) && lds <= 48 * 1024) { t.gate_tx = gtx; t.gate_rows = grows; t.gate_span = span; }
}

// k_pool forms ca itself -- the last workgroup of a sample to arrive runs the shared MLP (fwd.cuh: pool_body) -- at NCHW levels where
// k_gate's first resident round would otherwise sit on the sample's ca flag: the streamed MLP takes the shape, C*hidden is small enough
// that the forward never splits the MLP off (forward_group: k_mlp), the level can run k_gate, and x of one sample is >= 1 MiB.  The last
// condition keeps the small levels of a pyramid out: a tail costs k_pool ~2.5 us (every level streams to the end of the launch, so the
// tails run behind it), and the tiles of the small levels become resident in k_gate's second round, when ca is long there -- only the
// level of the first round repays it (k_gate -6 us at config 2).  A rule of the LEVEL alone:
// a ctx meets the level in calls of any composition, and the pool and the chan|apply stage calls must agree.  Fault injection keeps the
// role workgroup it silences.
static bool pool_forms_ca(const Geo& g, const Tune& t, bool nhwc, int dtype) {
  const Knobs kn = knobs();
  if (nhwc || kn.fault || kn.pool_mlp == 0) return false;
  if (!mlp_stream_ok(g) || static_cast<long long>(g.C) * g.hidden >= 8192 || t.gate_tx <= 0) return false;
  return kn.pool_mlp == 2 || static_cast<size_t>(g.C) * g.HW * (dtype == MGACBAM_F32 ? 4 : 2) >= (size_t(1) << 20);
}

static Tune choose_tune(int B, int C, int H, int W, int k) {
  const int HW = H * W, VEC = vec_of(H, W), nv = HW / VEC;
  const Knobs kn = knobs();
  Tune t;
  // rows of TX lanes sweep H*W: aim for >= 4 sweeps per lane, then shrink channels/row until the grid fills the chip
  int tx = pow2_floor(nv / 4 > 0 ? nv / 4 : 1);
  if (tx > 256) tx = 256;
  int cpt = 4;
  while (cpt > 1 && static_cast<long long>(B) * ((C + (256 / tx) * cpt - 1) / ((256 / tx) * cpt)) < 1024) cpt /= 2;
  t.pool_tx = tx; t.pool_cpt = cpt;
  // one H*W vector per lane, TY channel slices: TX <= 64 so row reductions are pure wave shuffles
  int ctx = pow2_ceil(nv) < 64 ? pow2_ceil(nv) : 64;
  constexpr int kChanMinTx = 16;
  while (ctx > kChanMinTx && static_cast<long long>(B) * ((nv + ctx - 1) / ctx) < 768) ctx /= 2;
  while (ctx < 64 && (256 / ctx) * 4 > C) ctx *= 2;       // keep >= 4 channels per row
  t.chan_tx = ctx;
  // conv tiles: full rows when W <= 128, otherwise equal column strips; 4 px per thread
  const int ntx = (W + 127) / 128;
  const int tw = (((W + ntx - 1) / ntx) + 3) / 4 * 4;
  t.conv_twq = tw / 4;
  int th = 256 / t.conv_twq;
  if (th > H) th = H;
  if (th > 64) th = 64;
  const int cap = 24 * 256 / (4 * (tw + k - 1)) - (k - 1);  // 4 staged planes (tile + halo) in <= 24 loads per thread
  if (th > cap) th = cap;
  if (th < 1) th = 1;
  t.conv_th = th;
  int wth = 3500 / (4 * (tw + k - 1)) - (k - 1);                // dWsa tiles: 4 staged planes (tile + halo) <= ~14 KB of LDS
  if (wth > H) wth = H;
  if (wth > 64) wth = 64;
  if (wth < 1) wth = 1;
  t.wsa_th = wth;
  // experiment hooks (tests / tuning sweeps); ignored when not a legal value
  int v;
  if (is_pow2_in(v = kn.pool_tx, 1, 256)) t.pool_tx = v;
  if ((v = kn.pool_cpt) == 1 || v == 2 || v == 4) t.pool_cpt = v;
  if (is_pow2_in(v = kn.chan_tx, 1, 64)) t.chan_tx = v;
  // k_apply stages every image row its TX*VEC-pixel tile touches, plus the k-1 halo rows
  int rows = (t.chan_tx * VEC - 1) / W + 2;
  if (rows > H) rows = H;
  t.apply_rows = rows + k - 1;
  gate_geometry(C, H, W, k, VEC, t);
  return t;
}

static int conv_tiles(const Tune& t, int H, int W) {
  const int TW = t.conv_twq * 4;
  return ((W + TW - 1) / TW) * ((H + t.conv_th - 1) / t.conv_th);
}
static int wsa_tiles(const Tune& t, int H, int W) {
  const int TW = t.conv_twq * 4;
  return ((W + TW - 1) / TW) * ((H + t.wsa_th - 1) / t.wsa_th);
}
static int chan_tiles(const Tune& t, int H, int W, int vec) {
  const int nv = H * W / vec;
  return (nv + t.chan_tx - 1) / t.chan_tx;
}

// ------------------------------------------------------------------------------------------------
// channels-last levels (MGACBAM_LAYOUT_NHWC, nhwc.cuh): chunk geometry and work buffers, functions of the level alone
// ------------------------------------------------------------------------------------------------
// elements per lane along C: 16 B when C allows it (fp32: 4, fp16 / bf16: 8), else 4 or scalar
static int nhwc_vec(int C, int dtype) { return (dtype != MGACBAM_F32 && C % 8 == 0) ? 8 : (C % 4 == 0 ? 4 : 1); }
// a level's vector width: along H*W for NCHW levels, along C for NHWC levels
static int level_vec(bool nhwc, int C, int H, int W, int dtype) { return nhwc ? nhwc_vec(C, dtype) : vec_of(H, W); }
static NhwcGeo nhwc_geo(int C, int H, int W, int vec) {
  NhwcGeo n;
  n.ng = (C + vec - 1) / vec;
  n.cs = std::max(4, std::min(pow2_ceil(n.ng), 64));         // >= 4 lanes: a tile is at most 512 pixels (k_apply_nhwc stages its rows)
  n.lcs = 0;
  while ((1 << n.lcs) < n.cs) ++n.lcs;
  n.ch = (kBlock / n.cs) * (vec == 8 ? 4 : 8);                // pixels per thread: nhwc.cuh NhwcNpx
  n.ntile = static_cast<int>((static_cast<long long>(H) * W + n.ch - 1) / n.ch);
  n.rp = (n.ntile + kNhwcMaxChunks - 1) / kNhwcMaxChunks;     // H*W-dependent chunking: at most kNhwcMaxChunks partials per sample
  n.nchunk = (n.ntile + n.rp - 1) / n.rp;
  return n;
}
// workgroups of the NHWC fold kernels (k_pool_fin, k_eca_fin, k_eca_fold): blocks of kNhwcFoldC channels per sample
static int nhwc_fold_blocks(const Geo& g) { return g.B * ((g.C + kNhwcFoldC - 1) / kNhwcFoldC); }
static size_t nhwc_ws_bytes(int B, int C, int H, int W, int vec) {
  return static_cast<size_t>(B) * nhwc_geo(C, H, W, vec).nchunk * (4 * static_cast<size_t>(C) + 4) * sizeof(float);
}

// backward scratch of a level of either layout (vec: level_vec); the two layouts differ in the partials of A_part and pgh
struct ScratchLayout { size_t A_part, gpre, gplanes, gwsa_part, gz, gbq, gh_avg, gh_mx, pgh, proj, total; };
// W1-projection planes of a level with kProjMax < hidden <= kProjWide (bwd.cuh): made by the k_bwd_reduce1 tiles on the matrix cores and
// read by k_bwd_apply within one backward, so they live in the scratch buffer (its LAST region), not in the ctx.  Everything the rule asks
// of the level except what the scratch size cannot know (fp32 features, gmask wanted: backward_args).  The tiles' wave must be the B operand
// of v_mfma_f32_16x16x4_f32 -- 4 channel rows x 16 lanes of 4 pixels: VEC 4, chan_tx 16 -- and x at least 1 MiB: a smaller level is still
// in the cache when k_bwd_apply reads it again, so its planes would save nothing.
static bool wide_proj_shape(int B, int C, int H, int W, int hidden, bool nhwc, int vec, const Tune& t) {
  return !nhwc && hidden > kProjMax && hidden <= kProjWide && vec == 4 && t.chan_tx == 16 &&
         static_cast<size_t>(B) * C * H * W * sizeof(float) >= (size_t(1) << 20);
}
static ScratchLayout scratch_layout(int B, int C, int H, int W, int hidden, int k, bool nhwc, int vec) {
  // the tile counts follow the launch geometry, which follows the knobs (NHWC: only the conv tiling, which does not depend on B, is used)
  const Tune t = choose_tune(B, C, H, W, k);
  const size_t HW = static_cast<size_t>(H) * W, BC = static_cast<size_t>(B) * C;
  const size_t nwsa = static_cast<size_t>(B) * wsa_tiles(t, H, W);
  ScratchLayout L;
  Carver cv;
  // NCHW: tile partials of A and Q live together, (B, nt, 2, C); NHWC: (B, nchunk, 3, C) = A, D, sum x*wgt
  L.A_part = cv.take(nhwc ? 3 * BC * nhwc_geo(C, H, W, vec).nchunk : 2 * BC * chan_tiles(t, H, W, vec));
  L.gpre = cv.take(B * HW); L.gplanes = cv.take(static_cast<size_t>(B) * 3 * HW);
  L.gwsa_part = cv.take(nwsa * 3 * k * k);
  L.gz = cv.take(BC); L.gbq = cv.take(BC);
  L.gh_avg = cv.take(static_cast<size_t>(B) * hidden); L.gh_mx = cv.take(static_cast<size_t>(B) * hidden);
  // channel groups per sample -- NCHW: worst case (1 channel per row of the sweep kernels), NHWC: blocks of kNhwcFoldC
  const size_t cpg = nhwc ? kNhwcFoldC : kBlock / t.pool_tx;
  L.pgh = cv.take(static_cast<size_t>(B) * ((C + cpg - 1) / cpg) * hidden);
  L.proj = cv.take(wide_proj_shape(B, C, H, W, hidden, nhwc, vec, t) ? static_cast<size_t>(B) * hidden * HW : 0);   // (B, hidden, HW)
  L.total = cv.total;
  return L;
}
static ScratchPtrs scratch_ptrs(void* p, const ScratchLayout& L) {
  return ScratchPtrs{at(p, L.A_part), at(p, L.gpre), at(p, L.gplanes), at(p, L.gwsa_part), at(p, L.gz), at(p, L.gbq),
                     at(p, L.gh_avg), at(p, L.gh_mx), at(p, L.pgh), at(p, L.proj)};
}
// the size queries take no element type: the answer covers every one (the NCHW geometry does not depend on it)
static size_t ws_bytes_any(int B, int C, int H, int W, bool nhwc) {
  if (!nhwc) return 0;
  return std::max(nhwc_ws_bytes(B, C, H, W, nhwc_vec(C, MGACBAM_F32)), nhwc_ws_bytes(B, C, H, W, nhwc_vec(C, MGACBAM_F16)));
}
static size_t scratch_bytes_any(int B, int C, int H, int W, int hidden, int k, bool nhwc) {
  return std::max(scratch_layout(B, C, H, W, hidden, k, nhwc, level_vec(nhwc, C, H, W, MGACBAM_F32)).total,
                  scratch_layout(B, C, H, W, hidden, k, nhwc, level_vec(nhwc, C, H, W, MGACBAM_F16)).total);
}

// ABI 14: every work buffer travels with its capacity; the requirement is recomputed under the CURRENT knobs at every call
static int check_capacity(const char* what, const char* buf, size_t want, size_t got) {
  if (got < want)
    return fail(MGACBAM_E_SIZE, "%s: %s holds %zu bytes, this shape needs %zu under the current knobs (query the size again after "
                "mgacbam_reload_env(); a size cached across a knob change or taken for another shape is stale)", what, buf, got, want);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// dispatch helpers
// ------------------------------------------------------------------------------------------------
static size_t elem_size(int dtype) { return dtype == MGACBAM_F32 ? 4 : 2; }
static bool aligned_to(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

static int check_dtype(const char* what, int dtype) {
  if (dtype < MGACBAM_F32 || dtype > MGACBAM_BF16) return fail(MGACBAM_E_DTYPE, "%s: dtype %d", what, dtype);
  return 0;
}

// Kernel selection: a run-time value becomes a compile-time one by calling a generic lambda with a tag -- f(Ty<float>{}),
// f(Int<4>{}), f(std::true_type{}) -- and returning what it returns: nested, the innermost lambda names ONE instantiation
// (`return k_pool<T, v.value, c.value, m.value>;`) and the selection is a typed expression that yields the kernel.  Only the
// combinations a selector can form are instantiated; the LAST listed value is where every other run-time value goes.
template <typename T> struct Ty { using type = T; };
template <int V> using Int = std::integral_constant<int, V>;
// any dtype other than F32 / F16 is bf16_t
template <typename F>
static auto with_elem(int dtype, F f) {
  if (dtype == MGACBAM_F32) return f(Ty<float>{});
  if (dtype == MGACBAM_F16) return f(Ty<__half>{});
  return f(Ty<bf16_t>{});
}
template <int V0, int... Vs, typename F>
static auto with_int(int v, F f) {
  if constexpr (sizeof...(Vs) == 0) {
    return f(Int<V0>{});
  } else {
    if (v == V0) return f(Int<V0>{});
    return with_int<Vs...>(v, f);
  }
}
template <typename F>
static auto with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
// T x VEC (vec_of: 1 or 4): f(Ty<T>, Int<VEC>)
template <typename F>
static auto with_elem_vec(int dtype, int vec, F f) {
  return with_elem(dtype, [&](auto t) { return with_int<4, 1>(vec, [&](auto v) { return f(t, v); }); });
}
// T x VEC of k_gate (FwdSig::gvec) and of the NHWC kernels (nhwc_vec): fp16 / bf16 also 8 (float x 8 is never formed)
template <typename F>
static auto with_elem_vec8(int dtype, int vec, F f) {
  return with_elem(dtype, [&](auto t) {
    if constexpr (sizeof(typename decltype(t)::type) == 2) return with_int<8, 4, 1>(vec, [&](auto v) { return f(t, v); });
    else return with_int<4, 1>(vec, [&](auto v) { return f(t, v); });
  });
}
// channels per thread of the sweep kernels (group_cpt), the conv size of the kernels specialised for 3 / 5 / 7 (0: any k, loops
// not unrolled) and of those that know only 7
template <typename F> static auto with_cpt(int cpt, F f) { return with_int<4, 2, 1>(cpt, f); }
template <typename F> static auto with_k(int k, F f) { return with_int<3, 5, 7, 0>(k, f); }
template <typename F> static auto with_k7(int k, F f) { return with_int<7, 0>(k, f); }
template <typename Tag> using elem_t = typename Tag::type;

static Geo make_geo(int B, int C, int H, int W, const mgacbam_params_t& p) {
  Geo g;
  g.B = B; g.C = C; g.H = H; g.W = W; g.HW = H * W; g.hidden = p.hidden; g.k = p.k;
  g.use_sigmoid = p.use_sigmoid_mask; g.thr = p.tiny_thr; g.eps = p.eps;
  g.proj_h = 0;
  return g;
}
static ParamPtrs make_params(const mgacbam_params_t& p) { return ParamPtrs{p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta}; }
static int check_params(const mgacbam_params_t& p) {
  if (!p.w1 || !p.b1 || !p.w2 || !p.b2 || !p.wsa || !p.beta) return fail(MGACBAM_E_NULL, "NULL parameter pointer");
  return 0;
}

// What a MaskCBAM level of either direction and layout is checked for after its pointers, and the part of its kernel arguments that
// does not depend on direction or layout (Level: mgacbam_fwd_level_t / mgacbam_bwd_level_t, Args: FwdArgs / BwdArgs)
template <typename Level>
static int check_level(const char* what, const Level& L) {
  if (int e = check_params(L.p)) return e;
  if (int e = check_shape(L.B, L.C, L.H, L.W, L.p.hidden, L.p.k)) return e;
  return check_dtype(what, L.dtype);
}
template <typename Level>
static int check_ctx_capacity(const char* what, const Level& L) {
  mgacbam_ctx_layout_t CL;
  ctx_layout(L.B, L.C, L.H, L.W, L.p.hidden, &CL);
  return check_capacity(what, "ctx", static_cast<size_t>(CL.total), L.ctx_bytes);
}
template <typename Level, typename Args>
static void level_setup(const Level& L, Args& A) {
  A.c = ctx_ptrs(const_cast<void*>(static_cast<const void*>(L.ctx)), L.B, L.C, L.H, L.W, L.p.hidden);
  A.p = make_params(L.p);
  A.g = make_geo(L.B, L.C, L.H, L.W, L.p);
  A.t = choose_tune(L.B, L.C, L.H, L.W, L.p.k);
  A.nflag = static_cast<int>(sync_layout(L.B, L.C, static_cast<size_t>(L.H) * L.W).nflag);
  const Knobs kn = knobs();
  A.trace = kn.trace; A.spin_limit = kn.spin_limit;
}

// Levels that share every compile-time property of the kernels (element type, vector width, mask / no mask, conv size, dL/dmask wanted,
// layout) are launched together: one grid per stage, the levels' grids concatenated.  Each family defines the signature it groups by next to
// its level function -- only the fields its kernel selection reads, set by name -- and the frame below asks three things of it:
//   operator==   over every field but weight.  The hand-off counters in ctx.sync count launches per TILE, so which levels share a launch is
//                part of correctness: a field belongs here only if it is a function of the LEVEL alone, never of the call's other levels
//   int weight   not compared: ~ how long a workgroup of the level runs (C x channels per thread of the tile kernels where the family has
//                them, else C); for_each_group launches the levels of a group longest first
//   int nhwc     the level is channels-last: a launch group is single-layout, and its group function picks the layout's kernels

// channels per thread for the row-sweep kernels, uniform over a group: 2 when that still gives the chip >= 6 workgroups
// per CU, else 1 (4 is instantiated and reachable through MGACBAM_POOL_CPT, but measured slower at every benchmark shape:
// k_pool 80 us vs 91 us at config 4, 22 vs 26 us at config 2)
template <typename Args>
static int group_cpt(const Args* lv, int n, int max_cpt = 2) {
  const int forced = knobs().pool_cpt;
  if (forced == 1 || forced == 2 || forced == 4) return forced;
  for (int cpt = max_cpt; cpt > 1; cpt /= 2) {
    long long blocks = 0;
    for (int l = 0; l < n; ++l) {
      const int tx = lv[l].t.pool_tx;
      const int cpb = (kBlock / tx) * cpt;
      blocks += static_cast<long long>(lv[l].g.B) * ((lv[l].g.C + cpb - 1) / cpb);   // real workgroups (padding ids exit at once)
    }
    if (blocks >= 1536) return cpt;
  }
  return 1;
}
// grids are XCD-aligned (common.cuh: xcd_sample_part): ceil(B/8)*8 sample slots x parts
static int xcd_grid(int B, int parts) { return ((B + 7) / 8) * 8 * parts; }
static int pad8(int n) { return (n + 7) & ~7; }
template <typename Args>
static int sweep_blocks(const Args& a, int tx, int cpt) {
  const int cpb = (kBlock / tx) * cpt;
  return xcd_grid(a.g.B, (a.g.C + cpb - 1) / cpb);
}
static size_t convT_smem(const Tune& t, int k) {
  return (((3 * k * k + 3) & ~3) + static_cast<size_t>(t.conv_th + k - 1) * (t.conv_twq * 4 + k - 1)) * sizeof(float);
}
static size_t wsa_smem(const Tune& t, int k) {
  return (4 * static_cast<size_t>(t.wsa_th + k - 1) * (t.conv_twq * 4 + k - 1) + static_cast<size_t>(3 * k * t.wsa_th) * k) * sizeof(float);
}
static size_t params_smem(const Geo& g) { return (3 * static_cast<size_t>(g.B) + 2 * kBlock) * sizeof(float); }
static int params_blocks(const Geo& g) { return g.hidden + (g.C + kBlock - 1) / kBlock + (3 * g.k * g.k + 3) / 4 + 1; }
static size_t chan_smem(const Geo& g, int vec, bool proj) {
  return (3 * static_cast<size_t>(g.C) + 2 * g.hidden + (proj ? static_cast<size_t>(g.C) * kProjMax : 0) + 4 * kBlock * vec) * sizeof(float);
}
static size_t apply_smem(const Geo& g, const Tune& t, int vec) {
  return (((3 * g.k * g.k + 3) & ~3) + 3 * static_cast<size_t>(t.apply_rows) * (g.W + g.k - 1) + t.chan_tx * vec + g.C) * sizeof(float);
}
static size_t gate_smem(const Geo& g, const Tune& t, int vec) {
  const size_t head = (g.C + 3) & ~3;
  const size_t role = 3 * static_cast<size_t>(g.C) + 2 * g.hidden;           // gate_role: the MLP's scratch (staged form: [2C][2h][C])
  const size_t conv = ((3 * g.k * g.k + 3) & ~3) + 3 * static_cast<size_t>(t.gate_rows) * (g.W + g.k - 1) + static_cast<size_t>(t.gate_tx) * vec;
  return std::max(role, head + std::max(conv, static_cast<size_t>(3) * kBlock * vec)) * sizeof(float);
}
static int gate_tiles(const Tune& t, int H, int W, int vec) {
  const int nv = H * W / vec;
  return (nv + t.gate_tx - 1) / t.gate_tx;
}
static size_t bwd_apply_smem(const Geo& g, int vec) { return (5 * static_cast<size_t>(g.C) + 2 * g.hidden + kBlock * vec) * sizeof(float); }
// (proj: the level's tiles also make its W1-projection planes -- 1, the VALU form: W1^T staged after the partials, four planes per combine
//  round; 2, the MFMA form: W1 comes from memory, and three waves' 16 x 64 partials are combined in one round)
static size_t reduce1_smem(const Geo& g, int vec, int proj) {
  if (!proj) return (3 * static_cast<size_t>(g.C) + kBlock * vec) * sizeof(float);
  if (proj == 2) return (((3 * static_cast<size_t>(g.C) + 3) & ~static_cast<size_t>(3)) + 3 * 16 * kWave) * sizeof(float);
  return (((3 * static_cast<size_t>(g.C) + 3) & ~static_cast<size_t>(3)) + static_cast<size_t>(g.C) * kProjMax + 4 * kBlock * vec) * sizeof(float);
}
static size_t pool_mlp_smem(const Geo& g) { return (4 + 2 * static_cast<size_t>(g.C) + 2 * g.hidden) * sizeof(float); }   // k_pool's tail: [last?, 3 pad][2C avg|mx][2h]
static size_t mlp_smem(const Geo& g) { return (3 * static_cast<size_t>(g.C) + 2 * g.hidden) * sizeof(float); }
// (their NHWC siblings: the *NhwcLds layout structs beside the kernels, nhwc.cuh lds_bytes)

// concatenate the levels' grids: workgroup ids [start[l], start[l+1]) of the launch belong to level l; returns the grid
template <typename Args, typename Fn>
static int fill_starts(Group<Args>& G, const Args* lv, int n, Fn blocks_of) {
  int tot = 0;
  for (int l = 0; l < n; ++l) { G.start[l] = tot; tot += blocks_of(lv[l]); }
  G.start[n] = tot;
  return tot;
}
template <typename Args>
static Group<Args> make_group(const Args* lv, int n) {
  Group<Args> G;
  G.n = n;
  for (int l = 0; l < n; ++l) G.lv[l] = lv[l];
  return G;
}
// dynamic LDS of a launch: the largest any level of the group asks for (smem_of: a function of the level, or a plain size)
template <typename Args, typename SmemOf>
static size_t group_smem(const Group<Args>& G, SmemOf smem_of) {
  if constexpr (std::is_convertible_v<SmemOf, size_t>) {
    return smem_of;
  } else {
    size_t smem = 0;
    for (int l = 0; l < G.n; ++l) smem = std::max(smem, static_cast<size_t>(smem_of(G.lv[l])));
    return smem;
  }
}
// One grouped launch: the levels' grids concatenated (G.start), the group's LDS size, kBlock threads.  The launches whose grid is not
// a concatenation per level (k_gate, k_bwd_r12, the mask head's per-pass sub-groups) compute it themselves and call launch().
template <typename Args, typename BlocksOf, typename SmemOf>
static int launch_group(const char* what, void (*kernel)(Group<Args>), Group<Args>& G, BlocksOf blocks_of, SmemOf smem_of, hipStream_t st) {
  const int grid = fill_starts(G, G.lv, G.n, blocks_of);
  return launch(what, kernel, grid, kBlock, group_smem(G, smem_of), st, G);
}

// partition the levels into launch groups (same signature, at most kGroupMax levels) and run `run` on each, in order of first
// appearance; layout 0 / 1: only the NCHW / channels-last levels, -1: all
template <typename Args, typename Sig, typename Run>
static int for_each_group(Args* args, const Sig* sigs, int n, int layout, Run run) {
  bool done[MGACBAM_MAX_LEVELS];
  for (int l = 0; l < n; ++l) done[l] = layout >= 0 && sigs[l].nhwc != layout;
  for (int l = 0; l < n; ++l) {
    if (done[l]) continue;
    int idx[kGroupMax], m = 0;
    for (int j = l; j < n && m < kGroupMax; ++j)
      if (!done[j] && sigs[j] == sigs[l]) { idx[m++] = j; done[j] = true; }
    std::stable_sort(idx, idx + m, [&](int a, int b) { return sigs[a].weight > sigs[b].weight; });
    Args grp[kGroupMax];
    for (int j = 0; j < m; ++j) grp[j] = args[idx[j]];
    if (int e = run(grp, m, sigs[l])) return e;
  }
  return 0;
}

// The frame of every grouped entry point: `level` checks one level and builds its argument block and signature
// (int level(const Level&, Args&, Sig&)); EVERY level is checked before anything is launched; then `run(Args*, n, const Sig&)` gets each
// launch group, in for_each_group's order -- nchw_first: the groups of the NCHW levels, then those of the channels-last ones (MaskCBAM,
// MaskECA), else all in order of first appearance (mask head, MaskSPADE).
template <typename Args, typename Sig, typename Level, typename LevelFn, typename Run>
static int run_levels(const Level* levels, int n_levels, bool nchw_first, LevelFn level, Run run) {
  if (!levels) return fail(MGACBAM_E_NULL, "levels is NULL");
  if (n_levels < 1 || n_levels > MGACBAM_MAX_LEVELS) return fail(MGACBAM_E_LEVELS, "n_levels=%d", n_levels);
  Args args[MGACBAM_MAX_LEVELS];
  Sig sigs[MGACBAM_MAX_LEVELS];
  for (int l = 0; l < n_levels; ++l)
    if (int e = level(levels[l], args[l], sigs[l])) return e;
  for (int layout = nchw_first ? 0 : -1; layout <= (nchw_first ? 1 : -1); ++layout)
    if (int e = for_each_group(args, sigs, n_levels, layout, run)) return e;
  g_err[0] = 0;
  return 0;
}
