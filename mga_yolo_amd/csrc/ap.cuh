// Average precision per class from a validation run's accumulated rows (include/ext/mgaap.h), without a host read-back: the fourth stage
// behind the post-process, the matching and the confusion matrix.  Launches are ordered by the stream only; every step across workgroups
// is reduce / one-workgroup scan / apply, and no floating-point value is ever combined by an atomic, so a run's result is the same bits
// every time.  Every kernel reads n_rows / n_targets from the device state words and the status word k_ap_starts wrote; a tile past the live
// rows exits before it reads anything.
//   k_ap_init      zeroes the control words, the class counters and nt.
//   k_ap_keys      per live row the confidence key (complement of the order-preserving image of the fp32 bits, -0.0 taken as +0.0) and the
//                  class key; a row of no class gets the largest key of class nc - 1, which no finite confidence has, so it sorts behind
//                  every counted row.  Integer atomics count nt and the detections per class (their order cannot change a count), in LDS
//                  first: one global atomic per class and workgroup (one per row is 17 ms at 1.5 M rows of one class).
//   k_ap_starts    one workgroup: the status word, the exclusive prefix of the class counts (a class's first sorted position).
//   k_ap_hist / k_ap_scan / k_ap_scatter    one pass of the stable LSD radix sort, 8 bits a pass.  The table is digit-major,
//                  table[digit * live_tiles + tile], so one flat exclusive scan gives every (digit, tile) its first position.  In the
//                  scatter a wave takes 64 consecutive rows a round; eight ballots (one per digit bit) give a lane the mask of the lanes
//                  with its digit, its rank the population below it; the first lane of a digit writes the wave's count to LDS, and a row's
//                  position is: the digit's rows of earlier rounds + of earlier waves of this round + the rank.
//   k_ap_tp_*      the inclusive scan of one threshold's tp column over the sorted order.
//   k_ap_env_*     precision's running maximum from the right over the same order, segmented by class: an associative combine on
//                  (maximum over the leading class's rows, leading class, trailing class).
//   k_ap_curves    one workgroup per class: binary searches into the class's rows for the 101 AP points, and at threshold 0 for the three
//                  1000-point curves.
#pragma once
#include "common.cuh"

namespace mgacbam {

constexpr int kApTile = 2048;                                  // MGAAP_TILE: rows per workgroup in every tiled step
constexpr int kApPer = kApTile / kBlock;                       // rows per thread
constexpr int kApWaves = kBlock / kWave;
constexpr int kApScanBlock = 1024;                             // threads of the one-workgroup integer scans
constexpr int kApScanPer = 16;                                 // entries per thread and trip
constexpr int kApPoints = 101, kApCurve = 1000;
constexpr int kApMaxNc = 1024;                                 // MGAAP_MAX_NC
static_assert(kApTile == kApPer * kBlock && kApTile == 8 * kApWaves * kWave, "a tile is eight rounds of the workgroup's waves");

struct ApArgs {
  const unsigned char* rows_tp; const float* rows_conf; const float* rows_cls; const float* tgt_cls; const int* state;
  int rows_cap, tgt_cap, niou, nc;
  const double* grid_ap; const double* grid_curve;
  double* ap; double* p_curve; double* r_curve; double* prec_values; int* nt; int* n_det;     // the result block
  int* status;
  int* ctl;                                                    // ws (8): [0] a bad target class was seen, [1] a NaN confidence, [2] the status
  int* starts;                                                 // ws (nc + 1): detections per class, then their exclusive prefix; [nc] = the counted rows
  unsigned* ckey[2]; unsigned* pay[2];                         // ws (rows_cap) each: the ping-pong buffers of the sort
  unsigned* clskey;                                            // ws (rows_cap): a row's class key, by row index
  int* S;                                                      // ws (rows_cap): the scanned tp column
  double* env;                                                 // ws (rows_cap): the envelope column
  int* table;                                                  // ws (256, live tiles): the sort's digit-major histogram table
  int* tpagg;                                                  // ws (tiles): tile sums of the tp column, then their exclusive prefix
  int4* envagg; int4* envcarry;                                // ws (tiles) each: a tile's ApSeg and the ApSeg of everything to its right
};
struct ApPass { int src, shift, by_class; };                   // the buffer the pass reads, the digit's shift, class digit or confidence digit

__device__ __forceinline__ int ap_rows(const ApArgs& A) { return min(max(A.state[0], 0), A.rows_cap); }
__device__ __forceinline__ int ap_targets(const ApArgs& A) { return min(max(A.state[1], 0), A.tgt_cap); }
__device__ __forceinline__ int ap_tiles(int n) { return (n + kApTile - 1) / kApTile; }
// the row index at a sorted position; the sort moves a permutation of 0 .. n - 1, and an index is still held below rows_cap before it is used
__device__ __forceinline__ unsigned ap_row(const ApArgs& A, int buf, int p) { return min(A.pay[buf][p], static_cast<unsigned>(A.rows_cap - 1)); }
// a class as a finite integer in 0 .. nc - 1, or -1
__device__ __forceinline__ int ap_class(float c, int nc) {
  if (!(c >= 0.f && c < static_cast<float>(nc))) return -1;    // a NaN fails both
  const int k = static_cast<int>(c);
  return static_cast<float>(k) == c ? k : -1;
}
__device__ __forceinline__ float ap_conf(float v) { return v == 0.f ? 0.f : v; }   // -0.0 -> +0.0
// ascending in this key = descending in confidence
__device__ __forceinline__ unsigned ap_conf_key(float v) {
  const unsigned u = __float_as_uint(ap_conf(v));
  return ~(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u));
}

// ---- the two index rules, as host functions too (tools/ap_host_check.cpp runs them under the host sanitizers) ---------------------
// the lanes of a wave that hold digit d: live = the ballot of the lanes with a row, have[b] = the ballot of bit b of the lanes' digits
__host__ __device__ __forceinline__ unsigned long long ap_same_digit(unsigned long long live, const unsigned long long (&have)[8], unsigned d) {
  unsigned long long same = live;
#pragma unroll
  for (int b = 0; b < 8; ++b) same &= ((d >> b) & 1u) ? have[b] : ~have[b];
  return same;
}
// a lane's rank among them: the lanes below it
__host__ __device__ __forceinline__ int ap_rank_below(unsigned long long same, int lane) {
  return __builtin_popcountll(same & ((1ull << lane) - 1ull));
}
// a row's position within its tile among the rows of its digit: the digit's rows of the earlier rounds (run), of the earlier waves of this
// round (cnt[w][d], w < wave) and of the lower lanes of its wave
template <typename Cnt>
__host__ __device__ __forceinline__ int ap_tile_rank(int run, const Cnt& cnt, int wave, unsigned d, int rank) {
  int before = run;
  for (int w = 0; w < wave; ++w) before += cnt[w][d];
  return before + rank;
}
// np.interp(x, mrec, mpre) over a class view K (np_ rows; mrec / mpre: index 0 and np_ + 1 are the sentinels); x lies in [0, 1]
template <typename View>
__host__ __device__ __forceinline__ double ap_interp_pr(const View& K, double x) {
  int lo = 0, hi = K.np_ + 2;                                  // mrec(lo) <= x < mrec(hi), hi = one past the end
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (K.mrec(mid) <= x) lo = mid; else hi = mid;
  }
  const double xj = K.mrec(lo), fj = K.mpre(lo);
  if (lo == K.np_ + 1 || xj == x) return fj;
  const double slope = (K.mpre(lo + 1) - fj) / (K.mrec(lo + 1) - xj);
  return slope * (x - xj) + fj;
}
// np.interp(-x, -conf, recall or precision, left = left)
template <bool kRecall, typename View>
__host__ __device__ __forceinline__ double ap_interp_conf(const View& K, double x, double left) {
  const double q = -x;
  const int last = K.np_ - 1;
  auto fp = [&](int j) { return kRecall ? K.recall(j) : K.precision(j); };
  if (q < K.neg_conf(0)) return left;
  if (q > K.neg_conf(last)) return fp(last);
  int lo = 0, hi = K.np_;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (K.neg_conf(mid) <= q) lo = mid; else hi = mid;
  }
  const double xj = K.neg_conf(lo), fj = fp(lo);
  if (lo == last || xj == q) return fj;
  const double slope = (fp(lo + 1) - fj) / (K.neg_conf(lo + 1) - xj);
  return slope * (q - xj) + fj;
}

// ---- workgroup scans ---------------------------------------------------------------------------------------------------------
// exclusive prefix of one int per thread over a workgroup of NT threads (red: NT / 64 + 1 ints of LDS); total: the workgroup's sum
template <int NT>
__device__ __forceinline__ int ap_block_exclusive(int v, int* red, int& total) {
  const int tid = static_cast<int>(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
  int inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o *= 2) {
    const int up = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += up;
  }
  __syncthreads();                                             // red may still be read from the previous call
  if (lane == kWave - 1) red[wave] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < NT / kWave; ++w) { const int s = red[w]; if (w < wave) before += s; all += s; }
  total = all;
  return before + inc - v;
}

// What a run of sorted rows passes to its left neighbour for the running maximum from the right: the maximum of precision over its
// LEADING class's rows, the leading and the trailing class.  ch < 0: no rows.  Classes ascend along the order, so ch == ct means one class.
struct ApSeg { double v; int ch, ct; };
__device__ __forceinline__ ApSeg ap_seg_empty() { return ApSeg{0.0, -1, -1}; }
__device__ __forceinline__ ApSeg ap_seg_join(const ApSeg& L, const ApSeg& R) {     // L lies left of R
  if (L.ch < 0) return R;
  if (R.ch < 0) return L;
  const bool through = L.ch == L.ct && R.ch == L.ch;
  return ApSeg{through ? fmax(L.v, R.v) : L.v, L.ch, R.ct};
}
__device__ __forceinline__ int4 ap_seg_pack(const ApSeg& s) {
  const long long b = __double_as_longlong(s.v);
  return make_int4(static_cast<int>(b & 0xffffffffll), static_cast<int>(b >> 32), s.ch, s.ct);
}
__device__ __forceinline__ ApSeg ap_seg_unpack(const int4& q) {
  const long long b = (static_cast<long long>(q.y) << 32) | static_cast<unsigned>(q.x);
  return ApSeg{__longlong_as_double(b), q.z, q.w};
}
// inclusive suffix join over the workgroup's kBlock threads: thread i gets own_i + own_(i+1) + ... (s: kBlock ApSegs of LDS, left holding them)
__device__ __forceinline__ ApSeg ap_block_suffix(ApSeg own, ApSeg* s) {
  const int tid = static_cast<int>(threadIdx.x);
  __syncthreads();
  s[tid] = own;
  __syncthreads();
  for (int o = 1; o < kBlock; o *= 2) {
    const ApSeg right = tid + o < kBlock ? s[tid + o] : ap_seg_empty();
    __syncthreads();
    own = ap_seg_join(own, right);
    s[tid] = own;
    __syncthreads();
  }
  return own;
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_ap_init(const ApArgs A) {
  const int tid = static_cast<int>(threadIdx.x);
  if (tid < 8) A.ctl[tid] = 0;
  for (int c = tid; c <= A.nc; c += kBlock) A.starts[c] = 0;
  for (int c = tid; c < A.nc; c += kBlock) A.nt[c] = 0;
}

__global__ __launch_bounds__(kBlock) void k_ap_keys(const ApArgs A) {
  __shared__ int s_det[kApMaxNc], s_nt[kApMaxNc];              // the workgroup's counts: one global atomic per class and workgroup, not per row
  const int n = ap_rows(A), m = ap_targets(A), nc = A.nc, tid = static_cast<int>(threadIdx.x);
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;           // (64-bit: a cap may lie just below 2^31)
  const long long i0 = static_cast<long long>(blockIdx.x) * kBlock + tid;
  for (int c = tid; c < nc; c += kBlock) { s_det[c] = 0; s_nt[c] = 0; }
  __syncthreads();
  bool nan_conf = false, bad_target = false;
  for (long long i = i0; i < n; i += stride) {
    const float conf = A.rows_conf[i];
    const int c = ap_class(A.rows_cls[i], nc);
    if (conf != conf) nan_conf = true;
    A.ckey[0][i] = c >= 0 ? ap_conf_key(conf) : 0xffffffffu;
    A.clskey[i] = static_cast<unsigned>(c >= 0 ? c : nc - 1);
    A.pay[0][i] = static_cast<unsigned>(i);
    if (c >= 0) atomicAdd(&s_det[c], 1);
  }
  for (long long j = i0; j < m; j += stride) {
    const int c = ap_class(A.tgt_cls[j], nc);
    if (c >= 0) atomicAdd(&s_nt[c], 1); else bad_target = true;
  }
  if (bad_target) atomicOr(&A.ctl[0], 1);
  if (nan_conf) atomicOr(&A.ctl[1], 1);
  __syncthreads();
  for (int c = tid; c < nc; c += kBlock) {
    if (s_det[c]) atomicAdd(&A.starts[c], s_det[c]);
    if (s_nt[c]) atomicAdd(&A.nt[c], s_nt[c]);
  }
}

__global__ __launch_bounds__(kApScanBlock) void k_ap_starts(const ApArgs A) {
  __shared__ int red[kApScanBlock / kWave + 1];
  const int tid = static_cast<int>(threadIdx.x), nc = A.nc;
  const int st = A.ctl[0] ? 3 : (A.ctl[1] ? 4 : 0);
  const int mine = tid < nc ? A.starts[tid] : 0;              // nc <= MGAAP_MAX_NC = the workgroup's threads
  int total;
  const int before = ap_block_exclusive<kApScanBlock>(mine, red, total);
  if (tid == 0) { A.ctl[2] = st; *A.status = st; A.starts[nc] = total; }
  if (tid < nc) { A.starts[tid] = before; A.n_det[tid] = st ? -1 : mine; if (st) A.nt[tid] = -1; }
}

// ---- one pass of the sort -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ap_digit(const ApArgs& A, const ApPass& P, int p, unsigned& key, unsigned& row) {
  row = ap_row(A, P.src, p);
  key = P.by_class ? 0u : A.ckey[P.src][p];
  return ((P.by_class ? A.clskey[row] : key) >> P.shift) & 255u;
}

__global__ __launch_bounds__(kBlock) void k_ap_hist(const ApArgs A, const ApPass P) {
  __shared__ int h[256];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  h[tid] = 0;
  __syncthreads();
  for (int j = 0; j < kApPer; ++j) {
    const int p = base + j * kBlock + tid;
    unsigned key, row;
    if (p < n) atomicAdd(&h[ap_digit(A, P, p, key, row)], 1);
  }
  __syncthreads();
  A.table[static_cast<size_t>(tid) * ap_tiles(n) + tile] = h[tid];
}

// exclusive scan, in place, of `len` ints by one workgroup, kApScanBlock * kApScanPer entries a trip
__device__ __forceinline__ void ap_scan_ints(int* a, long long len, int* red) {
  const int tid = static_cast<int>(threadIdx.x);
  int carry = 0;
  for (long long e0 = 0; e0 < len; e0 += kApScanBlock * kApScanPer) {
    const long long at0 = e0 + static_cast<long long>(tid) * kApScanPer;
    int v[kApScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kApScanPer; ++k) { v[k] = at0 + k < len ? a[at0 + k] : 0; sum += v[k]; }
    int total;
    int run = carry + ap_block_exclusive<kApScanBlock>(sum, red, total);
#pragma unroll
    for (int k = 0; k < kApScanPer; ++k) { if (at0 + k < len) a[at0 + k] = run; run += v[k]; }
    carry += total;
  }
}

__global__ __launch_bounds__(kApScanBlock) void k_ap_scan(const ApArgs A) {
  __shared__ int red[kApScanBlock / kWave + 1];
  if (A.ctl[2]) return;
  ap_scan_ints(A.table, 256ll * ap_tiles(ap_rows(A)), red);
}

__global__ __launch_bounds__(kBlock) void k_ap_scatter(const ApArgs A, const ApPass P) {
  __shared__ int s_first[256];                                 // the digit's first position for this tile
  __shared__ int s_run[256];                                   // the digit's rows in the tile's earlier rounds
  __shared__ int s_cnt[kApWaves][256];                         // the digit's rows per wave in this round
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
  const int tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  s_first[tid] = A.table[static_cast<size_t>(tid) * ap_tiles(n) + tile];
  s_run[tid] = 0;
#pragma unroll
  for (int w = 0; w < kApWaves; ++w) s_cnt[w][tid] = 0;
  __syncthreads();
  const int dst = P.src ^ 1;
  for (int r = 0; r < kApPer; ++r) {                           // uniform: every lane takes every ballot
    const int p = base + (r * kApWaves + wave) * kWave + lane;
    const bool live = p < n;
    unsigned key = 0, row = 0, d = 0;
    if (live) d = ap_digit(A, P, p, key, row);
    const unsigned long long alive = __builtin_amdgcn_ballot_w64(live);
    unsigned long long have[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) have[b] = __builtin_amdgcn_ballot_w64((d >> b) & 1u);
    const unsigned long long same = ap_same_digit(alive, have, d);
    const int rank = ap_rank_below(same, lane);
    if (live && rank == 0) s_cnt[wave][d] = __popcll(same);
    __syncthreads();
    if (live) {
      const int at_ = s_first[d] + ap_tile_rank(s_run[d], s_cnt, wave, d, rank);
      if (at_ < n) {                                           // always, by the table; a row is never stored past the live rows
        A.pay[dst][at_] = row;
        if (!P.by_class) A.ckey[dst][at_] = key;
      }
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int w = 0; w < kApWaves; ++w) { add += s_cnt[w][tid]; s_cnt[w][tid] = 0; }
    s_run[tid] += add;
    __syncthreads();
  }
}

// ---- one threshold's column --------------------------------------------------------------------------------------------------------
struct ApCol { int pay, t; };                                  // the buffer that holds the sorted payload, the threshold

__global__ __launch_bounds__(kBlock) void k_ap_tp_reduce(const ApArgs A, const ApCol C) {
  __shared__ int red[kApWaves + 1];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  int sum = 0;
  for (int j = 0; j < kApPer; ++j) {
    const int p = base + j * kBlock + tid;
    if (p < n) sum += A.rows_tp[static_cast<size_t>(ap_row(A, C.pay, p)) * A.niou + C.t] != 0;
  }
  int total;
  ap_block_exclusive<kBlock>(sum, red, total);
  if (tid == 0) A.tpagg[tile] = total;
}

__global__ __launch_bounds__(kApScanBlock) void k_ap_tp_scan(const ApArgs A) {
  __shared__ int red[kApScanBlock / kWave + 1];
  if (A.ctl[2]) return;
  ap_scan_ints(A.tpagg, ap_tiles(ap_rows(A)), red);
}

__global__ __launch_bounds__(kBlock) void k_ap_tp_apply(const ApArgs A, const ApCol C) {
  __shared__ int red[kApWaves + 1];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  const int p0 = base + tid * kApPer;                          // a thread's rows are consecutive
  int v[kApPer], sum = 0;
#pragma unroll
  for (int k = 0; k < kApPer; ++k) {
    v[k] = p0 + k < n ? A.rows_tp[static_cast<size_t>(ap_row(A, C.pay, p0 + k)) * A.niou + C.t] != 0 : 0;
    sum += v[k];
  }
  int total;
  int run = A.tpagg[tile] + ap_block_exclusive<kBlock>(sum, red, total);
#pragma unroll
  for (int k = 0; k < kApPer; ++k) { run += v[k]; if (p0 + k < n) A.S[p0 + k] = run; }
}

// a thread's kApPer consecutive sorted rows for the envelope: class (nc past the counted rows) and precision
__device__ __forceinline__ void ap_env_rows(const ApArgs& A, const ApCol& C, int p0, int (&cls)[kApPer], double (&prec)[kApPer]) {
  const int counted = A.starts[A.nc];
#pragma unroll
  for (int k = 0; k < kApPer; ++k) {
    const int p = p0 + k;
    cls[k] = A.nc; prec[k] = 0.0;
    if (p < counted) {
      const int c = static_cast<int>(A.clskey[ap_row(A, C.pay, p)]), first = A.starts[c];
      const int before = first > 0 ? A.S[first - 1] : 0;
      cls[k] = c;
      prec[k] = static_cast<double>(A.S[p] - before) / static_cast<double>(p - first + 1);
    }
  }
}
__device__ __forceinline__ ApSeg ap_env_own(const int (&cls)[kApPer], const double (&prec)[kApPer]) {
  ApSeg own{prec[0], cls[0], cls[kApPer - 1]};
#pragma unroll
  for (int k = 1; k < kApPer; ++k) if (cls[k] == cls[0]) own.v = fmax(own.v, prec[k]);
  return own;
}

__global__ __launch_bounds__(kBlock) void k_ap_env_reduce(const ApArgs A, const ApCol C) {
  __shared__ ApSeg s[kBlock];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  int cls[kApPer]; double prec[kApPer];
  ap_env_rows(A, C, base + tid * kApPer, cls, prec);
  const ApSeg all = ap_block_suffix(ap_env_own(cls, prec), s);
  if (tid == 0) A.envagg[tile] = ap_seg_pack(all);
}

// one workgroup: envcarry[tile] = the join of every tile to its right, kBlock tiles a trip from the right end
__global__ __launch_bounds__(kBlock) void k_ap_env_scan(const ApArgs A) {
  __shared__ ApSeg s[kBlock];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tiles = ap_tiles(ap_rows(A));
  ApSeg carry = ap_seg_empty();                                // uniform over the workgroup
  for (int hi = tiles; hi > 0; hi -= kBlock) {
    const int lo = max(hi - kBlock, 0), tile = lo + tid;
    const ApSeg own = tile < hi ? ap_seg_unpack(A.envagg[tile]) : ap_seg_empty();
    const ApSeg inc = ap_block_suffix(own, s);
    const ApSeg right = tid + 1 < kBlock ? s[tid + 1] : ap_seg_empty();
    if (tile < hi) A.envcarry[tile] = ap_seg_pack(ap_seg_join(right, carry));
    carry = ap_seg_join(s[0], carry);
  }
}

__global__ __launch_bounds__(kBlock) void k_ap_env_apply(const ApArgs A, const ApCol C) {
  __shared__ ApSeg s[kBlock];
  if (A.ctl[2]) return;
  const int tid = static_cast<int>(threadIdx.x), tile = static_cast<int>(blockIdx.x), n = ap_rows(A), base = tile * kApTile;
  if (base >= n) return;
  const int p0 = base + tid * kApPer, counted = A.starts[A.nc];
  int cls[kApPer]; double prec[kApPer];
  ap_env_rows(A, C, p0, cls, prec);
  ap_block_suffix(ap_env_own(cls, prec), s);
  const ApSeg right = ap_seg_join(tid + 1 < kBlock ? s[tid + 1] : ap_seg_empty(), ap_seg_unpack(A.envcarry[tile]));
  double m = right.v;
  int c = right.ch;
#pragma unroll
  for (int k = kApPer - 1; k >= 0; --k) {
    if (cls[k] == c) m = fmax(m, prec[k]); else { m = prec[k]; c = cls[k]; }
    if (p0 + k < counted) A.env[p0 + k] = m;
  }
}

// ---- curves ----------------------------------------------------------------------------------------------------------------------
// The sorted rows of one class as np.interp's arrays.  mrec / mpre: index 0 and np_ + 1 are the sentinels.
struct ApClass {
  const ApArgs& A; int first, np_, before, pay; double den;
  __device__ __forceinline__ double tpc(int j) const { return static_cast<double>(A.S[first + j] - before); }      // row j = 0 .. np_ - 1
  __device__ __forceinline__ double recall(int j) const { return tpc(j) / den; }
  __device__ __forceinline__ double precision(int j) const { return tpc(j) / static_cast<double>(j + 1); }
  __device__ __forceinline__ double mrec(int j) const { return j == 0 ? 0.0 : (j == np_ + 1 ? 1.0 : recall(j - 1)); }
  __device__ __forceinline__ double mpre(int j) const { return j == 0 ? 1.0 : (j == np_ + 1 ? 0.0 : A.env[first + j - 1]); }
  __device__ __forceinline__ double neg_conf(int j) const { return -static_cast<double>(ap_conf(A.rows_conf[ap_row(A, pay, first + j)])); }
};
__global__ __launch_bounds__(kBlock) void k_ap_curves(const ApArgs A, const ApCol C) {
  __shared__ double y[kApPoints];
  const int tid = static_cast<int>(threadIdx.x), c = static_cast<int>(blockIdx.x), t = C.t;
  const size_t row = static_cast<size_t>(c) * kApCurve;
  if (A.ctl[2] || A.nt[c] == 0 || A.starts[c + 1] == A.starts[c]) {      // a status: NaN; a class without labels or detections: zeros
    const double fill = A.ctl[2] ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    if (tid == 0) A.ap[static_cast<size_t>(c) * A.niou + t] = fill;
    if (t == 0)
      for (int k = tid; k < kApCurve; k += kBlock) { A.p_curve[row + k] = fill; A.r_curve[row + k] = fill; A.prec_values[row + k] = fill; }
    return;
  }
  const int first = A.starts[c];
  const ApClass K{A, first, A.starts[c + 1] - first, first > 0 ? A.S[first - 1] : 0, C.pay, static_cast<double>(A.nt[c]) + 1e-16};
  if (tid < kApPoints) y[tid] = ap_interp_pr(K, A.grid_ap[tid]);
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k + 1 < kApPoints; ++k) sum += (A.grid_ap[k + 1] - A.grid_ap[k]) * (y[k + 1] + y[k]) / 2.0;
    A.ap[static_cast<size_t>(c) * A.niou + t] = sum;
  }
  if (t != 0) return;
  for (int k = tid; k < kApCurve; k += kBlock) {
    const double x = A.grid_curve[k];
    A.prec_values[row + k] = ap_interp_pr(K, x);
    A.r_curve[row + k] = ap_interp_conf<true>(K, x, 0.0);
    A.p_curve[row + k] = ap_interp_conf<false>(K, x, 1.0);
  }
}

}  // namespace mgacbam
