// The detection post-process (include/mganms.h): Detect decode, candidates and greedy non-maximum suppression, without a host read-back.
//   k_nms_cand   : one thread per anchor, consecutive lanes on consecutive cells.  From the maps: the class probabilities first, the 64
//                  box channels only for an anchor that has a candidate.  From `pred`: read and convert.  Candidates are appended to the
//                  image's list -- box 4 x fp32 and a 64-bit key -- at a wave prefix behind ONE atomic per wave.  The key is the score's
//                  bits above the inverted candidate index (anchor * nc + class): keys are distinct, the largest is the next candidate
//                  to visit, and the order the hardware appends in cannot change any result.  It also clears the status word.
//                  The maps' layout is a compile-time parameter (detmaps.cuh: MapsLayout): in NHWC an anchor's channels are one row, read with
//                  16-byte loads where the row's own address allows; the class order, the append and the key are the NCHW kernel's.
//   k_nms_greedy : one workgroup per image.  max_nms: a radix select over the keys (eight 8-bit passes) finds the max_nms-th largest,
//                  what lies below it is dead.  Then one sweep per kept row: it kills what the last kept box suppresses and finds the
//                  largest live key (a DPP arg-max per wave, a few words through LDS).  A thread sweeps the same entries in every round,
//                  so a kill is read again only by the thread that wrote it.  Lists of up to kNmsLds entries are swept in LDS, longer
//                  ones in the workspace.  It leaves the image's counter at 0 for the next call.
#pragma once
#include "detmaps.cuh"

namespace mgacbam {

constexpr int kNmsLds = 1024;                  // entries of a list that is swept in LDS (24 bytes each)
typedef unsigned long long nms_key_t;

struct NmsArgs {
  DetMaps maps;                                // the Detect maps (detmaps.cuh; n_levels = 0: B, nc and A alone), or
  const void* pred;                            // (B, 4 + nc, A)
  int bpi;                                     // k_nms_cand's workgroups per image
  float conf, iou;
  int max_det, max_nms, multi, agnostic, cand_cap;
  int* cnt;                                    // (B): candidates appended to the image's list (may exceed cand_cap: the overflow)
  nms_key_t* keys;                             // (B, cand_cap)
  float4* boxes;                               // (B, cand_cap)
  float* dets; int* count; int* keep; int* status;
};

__device__ __forceinline__ nms_key_t nms_key(float score, int cand) {
  return (static_cast<nms_key_t>(__float_as_uint(score)) << 32) | static_cast<unsigned>(~cand);
}
__device__ __forceinline__ int nms_key_cand(nms_key_t k) { return static_cast<int>(~static_cast<unsigned>(k)); }

// the anchor's class values (probabilities from `pred`, logits from the maps) in ascending class order: fn(c, value)
template <typename T, typename F>
__device__ __forceinline__ void nms_classes(const MapsPlanes<T>& cls, int nc, F fn) {
  for (int c = 0; c < nc; ++c) fn(c, cls.at(c));
}
template <typename T, typename F>
__device__ __forceinline__ void nms_classes(const MapsRow<T>& cls, int nc, F fn) { cls.scan(0, nc, fn); }   // the row's own 16-byte pieces

// L: the maps' layout.  NHWC: an anchor's channels are one row, read with 16-byte loads (the class logits of consecutive anchors lie `no` elements
// apart, so the class scan touches every line of the map whatever the threshold); a decoded prediction has no such layout (api_nms.hip refuses it).
template <typename T, MapsLayout L = MapsLayout::kNCHW>
__global__ __launch_bounds__(kBlock) void k_nms_cand(const NmsArgs A) {
  constexpr bool kRows = L == MapsLayout::kNHWC;
  using Reader = typename MapsReaderOf<T, L>::type;
  const int tid = static_cast<int>(threadIdx.x), lane = tid & (kWave - 1);
  const int b = static_cast<int>(blockIdx.x) / A.bpi, a = (static_cast<int>(blockIdx.x) % A.bpi) * kBlock + tid;
  if (blockIdx.x == 0 && tid == 0) *A.status = 0;
  const bool live = a < A.maps.A;
  const int nc = A.maps.nc;
  // where the anchor's class values start and how far apart its channels lie
  Reader cls{}, f{};
  MapsAnchor t{};                                              // from pred: t.hw alone, the anchors
  if (live) {
    if constexpr (kRows) {
      t = maps_anchor(A.maps, a);
      f = maps_feat<T, L>(A.maps, t, b);
      cls = Reader{f.f + 4 * kMapsReg};
    } else {
      if (A.pred) {
        t.hw = static_cast<size_t>(A.maps.A);
        f = Reader{static_cast<const T*>(A.pred) + static_cast<size_t>(b) * (4 + nc) * t.hw + a, t.hw};
        cls = Reader{f.f + 4 * t.hw, t.hw};
      } else {
        t = maps_anchor(A.maps, a);
        f = maps_feat<T>(A.maps, t, b);
        cls = Reader{f.f + 4 * kMapsReg * t.hw, t.hw};
      }
    }
  }
  const bool from_pred = !kRows && A.pred != nullptr;
  // the anchor's candidates: every class over the threshold, or the best one (the lowest index among equal probabilities)
  int m = 0, best_c = 0;
  float best_p = -1.f;
  if (live) {
    nms_classes(cls, nc, [&](int c, float v) {
      const float p = from_pred ? v : sigmoidf_(v);
      if (A.multi) m += p > A.conf ? 1 : 0;
      else if (p > best_p) { best_p = p; best_c = c; }
    });
    if (!A.multi) m = best_p > A.conf ? 1 : 0;
  }
  // the wave's place in the list: a prefix over the lanes' counts and one atomic
  int before, total;
  if (!A.multi) {
    const unsigned long long mask = __ballot(m != 0);
    before = __popcll(mask & ((1ull << lane) - 1ull));
    total = __popcll(mask);
  } else {
    int incl = m;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += o;
    }
    before = incl - m;
    total = __shfl(incl, kWave - 1, kWave);
  }
  int base = 0;
  if (lane == 0 && total > 0) base = atomicAdd(&A.cnt[b], total);
  base = __shfl(base, 0, kWave);
  if (m == 0) return;
  float4 box;
  if (from_pred) {                                             // ops.xywh2xyxy
    const float cx = f.at(0), cy = f.at(1), w2 = f.at(2) * 0.5f, h2 = f.at(3) * 0.5f;
    box = make_float4(cx - w2, cy - h2, cx + w2, cy + h2);
  } else {
    box = make_float4((t.ax - maps_dist(f, 0)) * t.s, (t.ay - maps_dist(f, 1)) * t.s, (t.ax + maps_dist(f, 2)) * t.s, (t.ay + maps_dist(f, 3)) * t.s);
  }
  const size_t row = static_cast<size_t>(b) * A.cand_cap;
  long long at_ = static_cast<long long>(base) + before;
  if (!A.multi) {
    if (at_ < A.cand_cap) { A.keys[row + at_] = nms_key(best_p, a * nc + best_c); A.boxes[row + at_] = box; }
    return;
  }
  nms_classes(cls, nc, [&](int c, float v) {
    const float p = from_pred ? v : sigmoidf_(v);
    if (!(p > A.conf)) return;
    if (at_ < A.cand_cap) { A.keys[row + at_] = nms_key(p, a * nc + c); A.boxes[row + at_] = box; }
    ++at_;
  });
}

// (key, position) arg-max over a wave: the DPP steps of wave_group_argmax on a 64-bit key in two words.  Live keys are distinct; dead
// ones are 0 and lose against any live key.
__device__ __forceinline__ void nms_max_combine(unsigned& hi, unsigned& lo, int& pos, unsigned ohi, unsigned olo, int opos) {
  if (ohi > hi || (ohi == hi && olo > lo)) { hi = ohi; lo = olo; pos = opos; }
}
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ void nms_dpp_max(unsigned& hi, unsigned& lo, int& pos) {
  const int ihi = static_cast<int>(hi), ilo = static_cast<int>(lo);
  const unsigned ohi = static_cast<unsigned>(__builtin_amdgcn_update_dpp(ihi, ihi, CTRL, ROW_MASK, 0xF, false));
  const unsigned olo = static_cast<unsigned>(__builtin_amdgcn_update_dpp(ilo, ilo, CTRL, ROW_MASK, 0xF, false));
  const int opos = __builtin_amdgcn_update_dpp(pos, pos, CTRL, ROW_MASK, 0xF, false);
  nms_max_combine(hi, lo, pos, ohi, olo, opos);
}
__device__ __forceinline__ void nms_wave_max(unsigned& hi, unsigned& lo, int& pos) {
  nms_dpp_max<0xB1>(hi, lo, pos);
  nms_dpp_max<0x4E>(hi, lo, pos);
  nms_dpp_max<0x141>(hi, lo, pos);
  nms_dpp_max<0x140>(hi, lo, pos);
  nms_dpp_max<0x142, 0xA>(hi, lo, pos);
  nms_dpp_max<0x143, 0xC>(hi, lo, pos);
  hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(hi), 63));
  lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(lo), 63));
  pos = __builtin_amdgcn_readlane(pos, 63);
}

// LDS words the rounds and the select share
struct NmsShared {
  unsigned hi[kBlock / kWave], lo[kBlock / kWave];
  int pos[kBlock / kWave];
  int hist[256];
  int sel, want;
};

// ops.py:318-320: what lies below the max_nms-th largest key is dead.  n > max_nms, every key is live and distinct.
template <typename KP>
__device__ __forceinline__ void nms_select(KP keys, int n, int max_nms, int tid, NmsShared& S) {
  nms_key_t prefix = 0;
  int want = max_nms;                                          // the want-th largest of the keys that share the prefix
  for (int shift = 56; shift >= 0; shift -= 8) {
    S.hist[tid] = 0;                                           // kBlock = 256 bins
    __syncthreads();
    const nms_key_t above = shift == 56 ? 0ull : (~0ull << (shift + 8));
    for (int i = tid; i < n; i += kBlock) {
      const nms_key_t k = keys[i];
      if ((k & above) == prefix) atomicAdd(&S.hist[static_cast<int>(k >> shift) & 255], 1);
    }
    __syncthreads();
    int over = 0;
    for (int j = tid + 1; j < 256; ++j) over += S.hist[j];
    if (over < want && want <= over + S.hist[tid]) { S.sel = tid; S.want = want - over; }
    __syncthreads();
    prefix |= static_cast<nms_key_t>(S.sel) << shift;
    want = S.want;
    __syncthreads();
  }
  for (int i = tid; i < n; i += kBlock)
    if (keys[i] < prefix) keys[i] = 0;
}

// The visit: returns the number of kept rows, written to dets and keep as it goes.
template <typename KP, typename BP>
__device__ __forceinline__ int nms_rounds(const NmsArgs& A, int b, int n, KP keys, BP boxes, int tid, NmsShared& S) {
  const int lane = tid & (kWave - 1), wave = tid / kWave, nc = A.maps.nc;
  const bool by_class = !A.agnostic && nc > 1;
  float* dets = A.dets + static_cast<size_t>(b) * A.max_det * 6;
  int* keep = A.keep + static_cast<size_t>(b) * A.max_det;
  int kept = 0, last_c = 0;
  float4 last = make_float4(0.f, 0.f, 0.f, 0.f);
  float last_area = 0.f;
  while (kept < A.max_det) {
    unsigned hi = 0, lo = 0;
    int pos = -1;
    for (int i = tid; i < n; i += kBlock) {
      const nms_key_t k = keys[i];
      if (k == 0) continue;
      if (kept > 0) {                                          // only a KEPT box suppresses: the last one, the earlier ones did in their rounds
        bool same = true;
        if (by_class) same = nms_key_cand(k) % nc == last_c;
        if (same) {
          const float4 q = boxes[i];
          const float iw = fmaxf(fminf(last.z, q.z) - fmaxf(last.x, q.x), 0.f), ih = fmaxf(fminf(last.w, q.w) - fmaxf(last.y, q.y), 0.f);
          const float inter = iw * ih, area = (q.z - q.x) * (q.w - q.y);
          if (inter / (last_area + area - inter) > A.iou) { keys[i] = 0; continue; }
        }
      }
      nms_max_combine(hi, lo, pos, static_cast<unsigned>(k >> 32), static_cast<unsigned>(k), i);
    }
    nms_wave_max(hi, lo, pos);
    if (lane == 0) { S.hi[wave] = hi; S.lo[wave] = lo; S.pos[wave] = pos; }
    __syncthreads();
    hi = S.hi[0]; lo = S.lo[0]; pos = S.pos[0];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) nms_max_combine(hi, lo, pos, S.hi[w], S.lo[w], S.pos[w]);
    __syncthreads();                                           // S is written again in the next round
    if (hi == 0 && lo == 0) break;                             // nothing live (uniform: every thread read the same words)
    const int cand = nms_key_cand((static_cast<nms_key_t>(hi) << 32) | lo);
    last = boxes[pos];
    last_area = (last.z - last.x) * (last.w - last.y);
    last_c = cand % nc;
    if ((pos & (kBlock - 1)) == tid) keys[pos] = 0;            // its owner in the sweep
    if (tid == 0) {
      float* d = dets + kept * 6;
      d[0] = last.x; d[1] = last.y; d[2] = last.z; d[3] = last.w; d[4] = __uint_as_float(hi); d[5] = static_cast<float>(last_c);
      keep[kept] = cand / nc;
    }
    ++kept;
  }
  return kept;
}

__global__ __launch_bounds__(kBlock) void k_nms_greedy(const NmsArgs A) {
  __shared__ nms_key_t s_keys[kNmsLds];
  __shared__ float4 s_boxes[kNmsLds];
  __shared__ NmsShared S;
  __shared__ int s_n;
  const int tid = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
  if (tid == 0) s_n = A.cnt[b];
  __syncthreads();
  const int total = s_n;
  if (tid == 0) A.cnt[b] = 0;                                  // the next call's list starts empty
  float* dets = A.dets + static_cast<size_t>(b) * A.max_det * 6;
  int* keep = A.keep + static_cast<size_t>(b) * A.max_det;
  if (total > A.cand_cap || total < 0) {                       // the list overflowed: this image cannot be answered
    const float nan = __int_as_float(0x7fc00000);
    for (int i = tid; i < A.max_det * 6; i += kBlock) dets[i] = nan;
    for (int i = tid; i < A.max_det; i += kBlock) keep[i] = -1;
    if (tid == 0) { A.count[b] = -1; *A.status = 1; }
    return;
  }
  const int n = total;
  nms_key_t* gkeys = A.keys + static_cast<size_t>(b) * A.cand_cap;
  float4* gboxes = A.boxes + static_cast<size_t>(b) * A.cand_cap;
  int kept;
  if (n <= kNmsLds) {
    for (int i = tid; i < n; i += kBlock) { s_keys[i] = gkeys[i]; s_boxes[i] = gboxes[i]; }
    __syncthreads();
    if (n > A.max_nms) nms_select(s_keys, n, A.max_nms, tid, S);
    kept = nms_rounds(A, b, n, s_keys, s_boxes, tid, S);
  } else {
    if (n > A.max_nms) nms_select(gkeys, n, A.max_nms, tid, S);
    kept = nms_rounds(A, b, n, gkeys, gboxes, tid, S);
  }
  for (int i = kept * 6 + tid; i < A.max_det * 6; i += kBlock) dets[i] = 0.f;
  for (int i = kept + tid; i < A.max_det; i += kBlock) keep[i] = -1;
  if (tid == 0) A.count[b] = kept;
}

}  // namespace mgacbam
