// A batch's labels as the kernels see them: batch_idx (n), cls (n), bboxes (n, 4) xywh normalised, the device word n of live rows and the
// capacity n_cap.  The criterion (det.cuh), the matching (match.cuh) and the confusion matrix (confusion.cuh) read them through this one
// definition (mga_yolo_amd/detlabels.py: Python's side, and what the consumers keep apart on purpose; detmaps_host.cuh: the refusals).
#pragma once
#include "match_common.cuh"

namespace mgacbam {

struct LabelBatch {
  const float* batch_idx; const float* cls; const float* bboxes; const int* n_ptr; int n_cap;      // n_ptr: the live rows' word; nullptr: n_cap
};

__device__ __forceinline__ int labels_live(const LabelBatch& L) {
  const int n = L.n_ptr ? *L.n_ptr : L.n_cap;
  return n < 0 ? 0 : (n > L.n_cap ? L.n_cap : n);
}
// the validator's rule for a row that belongs to an image of the batch: 0 <= bi < B and integral (a NaN fails)
__device__ __forceinline__ bool labels_has_image(float bi, float fB) { return bi >= 0.f && bi < fB && bi == floorf(bi); }

// Row r's box as xyxy in pixels, in the reference's two forms.  They round differently and each is pinned bit for bit by its consumer's stored
// results: they must not be merged.  The validator's (models/yolo/detect/val.py:149, ops.xywh2xyxy, then the scale): (c -+ s / 2) * size
__device__ __forceinline__ float4 labels_box_val(const LabelBatch& L, int r, float img_w, float img_h) {
  const float cx = L.bboxes[4 * r], cy = L.bboxes[4 * r + 1], w2 = L.bboxes[4 * r + 2] / 2.f, h2 = L.bboxes[4 * r + 3] / 2.f;
  return make_float4((cx - w2) * img_w, (cy - h2) * img_h, (cx + w2) * img_w, (cy + h2) * img_h);
}
// The criterion's (utils/loss.py:231, the scale and then ops.xywh2xyxy): the row scaled by (W, H, W, H), then centre -+ half the size
template <typename Box>
__device__ __forceinline__ Box labels_box_loss(const LabelBatch& L, int r, float img_w, float img_h) {
  const float cx = L.bboxes[4 * r] * img_w, cy = L.bboxes[4 * r + 1] * img_h;
  const float hw = L.bboxes[4 * r + 2] * img_w * 0.5f, hh = L.bboxes[4 * r + 3] * img_h * 0.5f;
  return Box{cx - hw, cy - hh, cx + hw, cy + hh};
}

// Image b's rows of the flat label list, in flat order, by the whole workgroup: fn(slot, r) for every row r < n with batch_idx == b, slot being
// its rank within the image; returns the image's row count (uniform).  A chunk is kMatchStage consecutive rows per thread (a quarter of the
// barriers) and a prefix over the threads' counts places them (s_wave: match_block_offset's): no atomics, a slot does not depend on arrival.
// n: labels_live(L), read by the caller -- read again behind a kernel's stores the word is a vector load on every workgroup's way (k_cm_match).
template <typename F>
__device__ __forceinline__ int labels_stage(const LabelBatch& L, int n, int b, int tid, int* s_wave, F fn) {
  const float fb = static_cast<float>(b);
  int m = 0;                                                   // rows met so far (uniform)
  for (int base = 0; base < n; base += kMatchStage * kBlock) {
    const int r0 = base + tid * kMatchStage;
    bool mine[kMatchStage];
    int c = 0;
#pragma unroll
    for (int u = 0; u < kMatchStage; ++u) { mine[u] = r0 + u < n && L.batch_idx[r0 + u] == fb; c += mine[u] ? 1 : 0; }
    int total;
    int slot = m + match_block_offset(c, tid, s_wave, total);
#pragma unroll
    for (int u = 0; u < kMatchStage; ++u) {
      if (!mine[u]) continue;
      fn(slot, r0 + u);
      ++slot;
    }
    m += total;
  }
  return m;
}

}  // namespace mgacbam
