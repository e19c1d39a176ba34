// The validator's confusion matrix (include/ext/mgaconfusion.h), without a host read-back: the third stage behind the post-process and the matching.
//   k_cm_match : one workgroup per image.  The image's label rows are staged in LDS as k_match stages them (labels.cuh: labels_stage -- flat order,
//                prefix sums, no atomics).  Every thread strides over the image's detections; a counted one
//                (conf > conf_thres) keeps the largest IoU above iou_thres over ALL the labels, whatever their classes -- a strict `>` over
//                ascending slots that starts at the threshold, so equal IoUs go to the lower label row and a NaN never wins.  One 64-bit
//                atomicMax in LDS per label on (IoU bits << 32 | ~d) finds w(l): the largest IoU, among equals the lowest detection -- the
//                maximum of a set, whatever order its members arrive in.  det_out carries the slot from the second phase to the last (the
//                same thread writes and reads it), then the outcome.  Workgroup 0 also writes -1 into the lab_out rows of no image.
//   k_cm_count : one workgroup.  It folds the images' overflow and bad-class words into the status word, histograms the outcomes into
//                (nc + 1)^2 LDS cells with LDS integer atomics (integer sums: the order of arrival does not show), stores the per-call
//                matrix with plain stores and adds it to the run-long int64 matrix -- no global atomics, no zeroing launch.
#pragma once
#include "labels.cuh"

namespace mgacbam {

constexpr int kCmMaxNc = 119;                                  // MGACM_MAX_NC: (nc + 1)^2 int32 cells of static LDS, 57 600 bytes
constexpr int kCmCells = (kCmMaxNc + 1) * (kCmMaxNc + 1);

struct CmArgs {
  const float* dets; const int* count;
  LabelBatch labels;
  int B, max_det, m_cap, nc, single_cls;
  float img_w, img_h, conf_thres, iou_thres;
  int* det_out; int* lab_out; int* cm; long long* acc; int* status;
  int* over;                                                   // ws, (B): 1 for an image with more than m_cap label rows
  int* bad;                                                    // ws, (B): 1 for an image with a class outside 0 .. nc - 1 among what it counts
};

// a class as the reference's .int() takes it: truncated toward zero.  false: not finite, or the truncation lies outside 0 .. nc - 1
__device__ __forceinline__ bool cm_class(float c, int nc, int single_cls, int& out) {
  if (single_cls) { out = 0; return true; }
  const bool ok = c > -1.f && c < static_cast<float>(nc);       // a NaN fails both
  out = ok ? static_cast<int>(c) : 0;
  return ok;
}

__global__ __launch_bounds__(kBlock) void k_cm_match(const CmArgs A) {
  __shared__ float4 s_box[kMatchMaxGt];
  __shared__ float s_area[kMatchMaxGt];
  __shared__ int s_cls[kMatchMaxGt];
  __shared__ int s_row[kMatchMaxGt];
  __shared__ unsigned long long s_win[kMatchMaxGt];
  __shared__ int s_wave[kMatchWaves];
  __shared__ int s_bad;
  const int tid = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
  const int n = labels_live(A.labels), cnt = match_live_rows(A, b), nc = A.nc;
  const float fB = static_cast<float>(A.B);
  if (tid == 0) s_bad = 0;
  __syncthreads();
  if (b == 0)                                                  // the rows behind the n word and the rows of no image
    for (int r = tid; r < A.labels.n_cap; r += kBlock)
      if (r >= n || !labels_has_image(A.labels.batch_idx[r], fB)) A.lab_out[r] = -1;
  bool bad = false;
  const int m = labels_stage(A.labels, n, b, tid, s_wave, [&](int slot, int r) {
    int lc;
    if (!cm_class(A.labels.cls[r], A.nc, A.single_cls, lc)) bad = true;
    if (slot < A.m_cap) {
      const float4 q = labels_box_val(A.labels, r, A.img_w, A.img_h);
      s_box[slot] = q; s_area[slot] = match_area(q); s_cls[slot] = lc; s_row[slot] = r;
    } else {
      A.lab_out[r] = -1;                                       // past m_cap: the image cannot be answered
    }
  });
  const bool over = m > A.m_cap;
  const size_t row0 = static_cast<size_t>(b) * A.max_det;
  int* det_out = A.det_out + row0;
  if (over) {
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();                                           // the staged rows
    for (int d = tid; d < A.max_det; d += kBlock) det_out[d] = -1;
    for (int s = tid; s < A.m_cap; s += kBlock) A.lab_out[s_row[s]] = -1;
    __syncthreads();
    if (tid == 0) { A.over[b] = 1; A.bad[b] = s_bad; }
    return;
  }
  for (int s = tid; s < m; s += kBlock) s_win[s] = 0ull;
  __syncthreads();                                             // the staged rows and the winners' words
  // every counted detection's best label above the threshold, and per label the largest such IoU
  // (two detections a thread and trip, kBlock apart, as in k_match: one read of a staged label serves both and 300 rows are one trip)
  for (int d0 = tid; d0 < cnt; d0 += 2 * kBlock) {
    float4 box[2];
    float area[2], best[2] = {A.iou_thres, A.iou_thres};
    int slot[2] = {-1, -1};
    bool on[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool live = d0 + u * kBlock < cnt;
      const float* q = A.dets + (row0 + (live ? d0 + u * kBlock : d0)) * 6;
      box[u] = make_float4(q[0], q[1], q[2], q[3]);
      area[u] = match_area(box[u]);
      on[u] = live && q[4] > A.conf_thres;                     // counted: strict, a NaN confidence is not
      int dc;
      if (on[u] && !cm_class(q[5], nc, A.single_cls, dc)) bad = true;
    }
    if (on[0] || on[1]) {
#pragma unroll 2
      for (int s = 0; s < m; ++s) {
        const float la = s_area[s];
        const float4 lb = s_box[s];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const float iou = match_iou(lb, la, box[u], area[u]);
          if (iou > best[u]) { best[u] = iou; slot[u] = s; }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int d = d0 + u * kBlock;
      if (d >= cnt) continue;
      det_out[d] = on[u] ? (slot[u] >= 0 ? slot[u] : -2) : -1;   // -2: counted, no label
      if (on[u] && slot[u] >= 0)                               // best > iou_thres >= 0: the bits of a positive float order as it does
        atomicMax(&s_win[slot[u]], (static_cast<unsigned long long>(__float_as_uint(best[u])) << 32) | static_cast<unsigned>(~d));
    }
  }
  if (bad) atomicOr(&s_bad, 1);
  __syncthreads();
  for (int d = tid; d < A.max_det; d += kBlock) {
    if (d >= cnt) { det_out[d] = -1; continue; }
    const int v = det_out[d];                                  // this thread's own store
    if (v == -1) continue;
    det_out[d] = v >= 0 && static_cast<unsigned>(s_win[v]) == static_cast<unsigned>(~d) ? s_cls[v] : nc;
  }
  for (int s = tid; s < m; s += kBlock) {
    const unsigned long long w = s_win[s];
    int out = nc;
    if (w) {
      const int d = static_cast<int>(~static_cast<unsigned>(w));
      cm_class(A.dets[(row0 + d) * 6 + 5], nc, A.single_cls, out);
    }
    A.lab_out[s_row[s]] = out;
  }
  if (tid == 0) { A.over[b] = 0; A.bad[b] = s_bad; }
}

__global__ __launch_bounds__(kBlock) void k_cm_count(const CmArgs A) {
  __shared__ int s_cm[kCmCells];
  __shared__ long long s_sum[kMatchWaves];
  const int tid = static_cast<int>(threadIdx.x);
  const int nc = A.nc, side = nc + 1, cells = side * side;
  long long over = 0, bad = 0;
  for (int b = tid; b < A.B; b += kBlock) { over += A.over[b]; bad += A.bad[b]; }
  over = match_block_sum(over, tid, s_sum);
  bad = match_block_sum(bad, tid, s_sum);
  const int status = over ? 1 : (bad ? 3 : 0);
  if (tid == 0) *A.status = status;
  if (status) {                                                // the call counts nothing: cm zeros, acc as it was
    for (int i = tid; i < cells; i += kBlock) A.cm[i] = 0;
    return;
  }
  for (int i = tid; i < cells; i += kBlock) s_cm[i] = 0;
  __syncthreads();
  const int n = labels_live(A.labels);
  const int rows = A.B * A.max_det;
  for (int i = tid; i < rows; i += kBlock) {                   // a counted detection that is nobody's winner: [cls(d), nc]
    if (A.det_out[i] != nc) continue;
    int c;
    if (cm_class(A.dets[static_cast<size_t>(i) * 6 + 5], nc, A.single_cls, c)) atomicAdd(&s_cm[c * side + nc], 1);
  }
  for (int r = tid; r < n; r += kBlock) {                      // a label: [cls(w(l)), cls(l)], or [nc, cls(l)] without a winner
    const int v = A.lab_out[r];
    if (v < 0 || v > nc) continue;
    int c;
    if (cm_class(A.labels.cls[r], nc, A.single_cls, c)) atomicAdd(&s_cm[v * side + c], 1);
  }
  __syncthreads();
  for (int i = tid; i < cells; i += kBlock) {
    const int v = s_cm[i];
    A.cm[i] = v;
    if (A.acc) A.acc[i] += v;
  }
}

}  // namespace mgacbam
