// Matching detections to labels for the validation metrics (include/ext/mgamatch.h), without a host read-back.
//   k_match        : one workgroup per image.  The image's rows of the flat label list are staged in LDS in flat order (labels.cuh:
//                    labels_stage, so a slot is the row's rank within its image).  Every thread strides over the
//                    image's detections and keeps the largest class-matched IoU and its slot -- a strict `>` over ascending slots, so equal
//                    IoUs go to the lower label row.  Per threshold an integer atomicMin in LDS over owner[t][slot] finds the lowest
//                    detection that qualifies: the minimum of a set, whatever order its members arrive in.  tp[d, t] = owner[t][slot] == d.
//                    best_gt carries the slot from the second phase to the last (the same thread writes and reads it), then the flat row.
//                    Workgroup 0 also copies state's counters into ws: nothing writes state during this launch.
//   k_match_append : a workgroup per image and one per kBlock label rows.  Each folds the per-image overflow words, the counts and the label
//                    rows that belong to an image into the same decision (status 0 / 1 / 2) and, if the batch fits, copies its share: an
//                    image's rows at the counters' snapshot plus the counts before it, a chunk's label rows at the rows before it plus a
//                    rank within it -- prefix sums, no atomics, so the place of a row does not depend on arrival.  Workgroup 0 alone advances
//                    state and writes the status word; the others read only the snapshot.
#pragma once
#include "labels.cuh"

namespace mgacbam {

constexpr int kMatchMaxIou = 16;               // MGAMATCH_MAX_IOU

struct MatchArgs {
  const float* dets; const int* count;
  LabelBatch labels;
  int B, max_det, m_cap, niou, single_cls;
  float img_w, img_h;
  float iouv[kMatchMaxIou];
  int rows_cap, tgt_cap;
  unsigned char* tp; float* best_iou; int* best_gt;
  unsigned char* rows_tp; float* rows_conf; float* rows_cls; int* rows_img;
  float* tgt_cls; int* tgt_img; int* state;      // all nullptr: no accumulation
  int* status;
  int* over;                                     // ws, (B): 1 for an image with more than m_cap label rows
  int* snap;                                     // ws, (4): state as k_match found it
};

__global__ __launch_bounds__(kBlock) void k_match(const MatchArgs A) {
  __shared__ float4 s_box[kMatchMaxGt];
  __shared__ float s_area[kMatchMaxGt];
  __shared__ float s_cls[kMatchMaxGt];
  __shared__ int s_row[kMatchMaxGt];
  __shared__ int s_owner[kMatchMaxIou][kMatchMaxGt];
  __shared__ int s_wave[kMatchWaves];
  const int tid = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
  const int n = labels_live(A.labels), cnt = match_live_rows(A, b), niou = A.niou;
  const int m = labels_stage(A.labels, n, b, tid, s_wave, [&](int slot, int r) {
    if (slot < A.m_cap) {
      const float4 q = labels_box_val(A.labels, r, A.img_w, A.img_h);
      s_box[slot] = q; s_area[slot] = match_area(q); s_cls[slot] = A.labels.cls[r]; s_row[slot] = r;
    }
  });
  const bool over = m > A.m_cap;
  if (tid == 0) A.over[b] = over ? 1 : 0;
  if (b == 0 && tid < 3 && A.state) A.snap[tid] = A.state[tid];  // k_match_append's workgroups read the counters here while one advances them
  const size_t row0 = static_cast<size_t>(b) * A.max_det;
  unsigned char* tp = A.tp + row0 * niou;
  float* best_iou = A.best_iou + row0;
  int* best_gt = A.best_gt + row0;
  if (over) {                                                  // this image cannot be answered
    const float nan = __int_as_float(0x7fc00000);
    for (size_t i = tid; i < static_cast<size_t>(A.max_det) * niou; i += kBlock) tp[i] = 0;
    for (int d = tid; d < A.max_det; d += kBlock) { best_iou[d] = nan; best_gt[d] = -1; }
    return;
  }
  for (int i = tid; i < niou * m; i += kBlock) s_owner[i / m][i % m] = 0x7fffffff;
  __syncthreads();                                             // the staged rows and the owners
  // every detection's best label, and the lowest detection that qualifies per (threshold, label)
  // (two detections a thread and trip, kBlock apart, so that one read of a staged label serves both and 300 rows are one trip)
  for (int d0 = tid; d0 < cnt; d0 += 2 * kBlock) {
    float4 box[2];
    float c[2], area[2], best[2] = {0.f, 0.f};
    int slot[2] = {-1, -1};
    bool on[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      on[u] = d0 + u * kBlock < cnt;
      const float* q = A.dets + (row0 + (on[u] ? d0 + u * kBlock : d0)) * 6;
      box[u] = make_float4(q[0], q[1], q[2], q[3]);
      c[u] = q[5]; area[u] = match_area(box[u]);
    }
#pragma unroll 2
    for (int s = 0; s < m; ++s) {
      const float lc = s_cls[s], la = s_area[s];
      const float4 lb = s_box[s];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (!A.single_cls && lc != c[u]) continue;
        const float iou = match_iou(lb, la, box[u], area[u]);
        if (iou > best[u]) { best[u] = iou; slot[u] = s; }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (!on[u]) continue;
      const int d = d0 + u * kBlock;
      best_iou[d] = best[u];
      best_gt[d] = slot[u];
      if (slot[u] >= 0)
        for (int t = 0; t < niou && best[u] >= A.iouv[t]; ++t) atomicMin(&s_owner[t][slot[u]], d);
    }
  }
  __syncthreads();
  for (int d = tid; d < A.max_det; d += kBlock) {
    unsigned char* row = tp + static_cast<size_t>(d) * niou;
    if (d >= cnt) {
      for (int t = 0; t < niou; ++t) row[t] = 0;
      best_iou[d] = 0.f; best_gt[d] = -1;
      continue;
    }
    const int slot = best_gt[d];                               // this thread's own store
    const float best = best_iou[d];
    for (int t = 0; t < niou; ++t) row[t] = slot >= 0 && best >= A.iouv[t] && s_owner[t][slot] == d ? 1 : 0;
    best_gt[d] = slot >= 0 ? s_row[slot] : -1;
  }
}

// Workgroup b < B copies image b's rows, workgroup B + j the label rows [j kBlock, (j + 1) kBlock).  Every workgroup folds the same words
// into the same decision and finds its own place by summing what lies before it; none reads what another writes: the counters come from
// k_match's snapshot, and workgroup 0 alone writes state and the status word.
__global__ __launch_bounds__(kBlock) void k_match_append(const MatchArgs A) {
  __shared__ long long s_sum[kMatchWaves];
  __shared__ int s_wave[kMatchWaves];
  const int tid = static_cast<int>(threadIdx.x), wg = static_cast<int>(blockIdx.x);
  const int n = labels_live(A.labels), niou = A.niou;
  const float fB = static_cast<float>(A.B);
  const bool accumulate = A.state != nullptr;
  const int r0 = (wg - A.B) * kBlock;                          // a label workgroup's first row
  long long over = 0, rows = 0, tgts = 0, before = 0;
  for (int b = tid; b < A.B; b += kBlock) {
    const int c = match_live_rows(A, b);
    over += A.over[b]; rows += c;
    if (wg < A.B && b < wg) before += c;                       // an image workgroup: the rows of the images before its own
  }
  if (accumulate)
    for (int r = tid; r < n; r += kBlock) {
      const int mine = labels_has_image(A.labels.batch_idx[r], fB) ? 1 : 0;
      tgts += mine;
      if (wg >= A.B && r < r0) before += mine;
    }
  over = match_block_sum(over, tid, s_sum);
  rows = match_block_sum(rows, tid, s_sum);
  tgts = match_block_sum(tgts, tid, s_sum);
  before = match_block_sum(before, tid, s_sum);
  if (over || !accumulate) {
    if (wg == 0 && tid == 0) *A.status = over ? 1 : 0;
    return;
  }
  const int n_rows = A.snap[0], n_tgts = A.snap[1], seen = A.snap[2];
  if (n_rows < 0 || n_tgts < 0 || n_rows + rows > A.rows_cap || n_tgts + tgts > A.tgt_cap) {
    if (wg == 0 && tid == 0) *A.status = 2;
    return;
  }
  if (wg == 0 && tid == 0) {
    A.state[0] = n_rows + static_cast<int>(rows); A.state[1] = n_tgts + static_cast<int>(tgts); A.state[2] = seen + A.B;
    *A.status = 0;
  }
  if (wg < A.B) {                                              // image wg: its rows lie together in tp and in rows_tp
    const int cnt = match_live_rows(A, wg);
    const size_t src0 = static_cast<size_t>(wg) * A.max_det, dst0 = static_cast<size_t>(n_rows + before);
    const unsigned char* from = A.tp + src0 * niou;
    unsigned char* to = A.rows_tp + dst0 * niou;
    const long long bytes = static_cast<long long>(cnt) * niou;
    for (long long i0 = 0; i0 < bytes; i0 += 4 * kBlock) {     // four loads in flight per thread, then their stores
      unsigned char v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const long long i = i0 + u * kBlock + tid; v[u] = i < bytes ? from[i] : 0; }
#pragma unroll
      for (int u = 0; u < 4; ++u) { const long long i = i0 + u * kBlock + tid; if (i < bytes) to[i] = v[u]; }
    }
    for (int d = tid; d < cnt; d += kBlock) {
      const float* q = A.dets + (src0 + d) * 6;
      A.rows_conf[dst0 + d] = q[4];
      A.rows_cls[dst0 + d] = A.single_cls ? 0.f : q[5];
      A.rows_img[dst0 + d] = seen + wg;
    }
    return;
  }
  // the label rows that belong to an image, in flat order
  const int r = r0 + tid;
  const float bi = r < n ? A.labels.batch_idx[r] : -1.f;
  const bool mine = labels_has_image(bi, fB);
  int total;
  const int k = n_tgts + static_cast<int>(before) + match_block_offset(mine ? 1 : 0, tid, s_wave, total);
  if (mine) { A.tgt_cls[k] = A.labels.cls[r]; A.tgt_img[k] = seen + static_cast<int>(bi); }
}

}  // namespace mgacbam
