// The detection criterion (include/mgadet.h): task-aligned assignment, CIoU, DFL and BCE on the three Detect maps, read in place.
//   k_det_assign  : one workgroup per (image, ground-truth slot).  It finds the slot's label row, visits the rectangle of cells per level
//                   whose centres can lie inside the box, decodes each cell's box, and keeps the top-k cells by (metric, lowest anchor
//                   index): cells are staged in LDS kDetChunk at a time and the best k so far are carried from chunk to chunk, each
//                   taken by one workgroup arg-max.  It also clears its share of the image's per-anchor assignment.
//   k_det_resolve : one workgroup per image, the <= topk * m_cap candidates in LDS.  An anchor claimed by several slots goes to the
//                   arg-max over ALL slots of the overlap (which may be a slot that did not claim it); then the per-slot maxima of
//                   metric and overlap, the anchors' target scores and the image's share of their sum.
//   k_det_loss    : one thread per anchor: BCE over the classes; box and DFL terms for assigned anchors; per-workgroup partials.
//   k_det_final   : one workgroup: the partials in a fixed order, max(sum of target scores, 1), gains, the status word.
//   k_det_bwd     : one thread per anchor: every channel's gradient, in the features' element type and layout.
// Every kernel that reads the maps has the layout as a compile-time parameter (detmaps.cuh: MapsLayout).  In NHWC the two gathers read an
// anchor's row with 16-byte loads, the two sweeps move their workgroup's anchors through LDS; the arithmetic is the NCHW kernels', to the bit.
// No atomics on floating-point sums: every sum has a fixed order, two runs give the same bits.
#pragma once
#include "detmaps.cuh"
#include "labels.cuh"

namespace mgacbam {

constexpr int kDetTopkMax = 16;                // = MGADET_MAX_TOPK, kDetMMax = MGADET_MAX_GT (api_det.hip asserts these)
constexpr int kDetMMax = 256;                  // ground truths per image
constexpr int kDetChunk = 2048;                // cells a k_det_assign workgroup stages in LDS at a time

struct DetArgs {
  DetMaps maps;                                // the Detect maps (detmaps.cuh)
  void* gfeat[kMapsLevelsMax];                 // their gradients, in the same layout
  int topk, m_cap;
  float gain[3];
  float img_w, img_h;                          // W_0 * stride_0, H_0 * stride_0
  LabelBatch labels;                           // the batch's labels (labels.cuh)
  int* asg_gt; float* asg_score;               // (B, A): the label row an anchor is assigned to (-1: background), its target score
  int* cand_n; int* cand_row;                  // (B, m_cap): candidates kept, the slot's label row (-1: the image has fewer rows)
  int* cand_anchor; float* cand_metric; float* cand_overlap;   // (B, m_cap, kDetTopkMax)
  float* tss_part; int* ovf;                   // (B)
  float* partial;                              // (nblk, 3)
  float* fin;                                  // [0] = max(sum of target scores, 1), NaN for a poisoned call; [1] = the status as a float
  int nblk;
  float* out; float* items; int* status;
  const float* upstream;
};

__device__ __forceinline__ DetBox det_gt_box(const DetArgs& A, int r) { return labels_box_loss<DetBox>(A.labels, r, A.img_w, A.img_h); }
__device__ __forceinline__ bool det_gt_valid(const DetBox& g) { return ((g.x1 + g.y1) + g.x2) + g.y2 > 0.f; }      // loss.py:263
__device__ __forceinline__ int det_label(const DetArgs& A, int r) { return min(max(static_cast<int>(A.labels.cls[r]), 0), A.maps.nc - 1); }

// metrics.py:113-141 with xywh=False, CIoU=True: box1's and box2's heights carry the eps
constexpr float kDetEps = 1e-7f;
constexpr float kDetAtanK = 0.40528473456935109f;      // 4 / pi^2
__device__ __forceinline__ float det_ciou(const DetBox& p, const DetBox& q) {
  const float w1 = p.x2 - p.x1, h1 = p.y2 - p.y1 + kDetEps, w2 = q.x2 - q.x1, h2 = q.y2 - q.y1 + kDetEps;
  const float iw = fmaxf(fminf(p.x2, q.x2) - fmaxf(p.x1, q.x1), 0.f), ih = fmaxf(fminf(p.y2, q.y2) - fmaxf(p.y1, q.y1), 0.f);
  const float inter = iw * ih, uni = w1 * h1 + w2 * h2 - inter + kDetEps, iou = inter / uni;
  const float cw = fmaxf(p.x2, q.x2) - fminf(p.x1, q.x1), ch = fmaxf(p.y2, q.y2) - fminf(p.y1, q.y1);
  const float c2 = cw * cw + ch * ch + kDetEps;
  const float sx = q.x1 + q.x2 - p.x1 - p.x2, sy = q.y1 + q.y2 - p.y1 - p.y2;
  const float rho2 = (sx * sx + sy * sy) * 0.25f;
  const float da = atanf(w2 / h2) - atanf(w1 / h1), v = kDetAtanK * da * da;
  const float alpha = v / (v - iou + (1.f + kDetEps));
  return iou - (rho2 / c2 + v * alpha);
}
// the share of a two-argument max / min that goes to its first argument (torch: an equal pair shares the gradient)
__device__ __forceinline__ float det_gt_share(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }
// CIoU(p, q) and its gradient with respect to p = (x1, y1, x2, y2); alpha is a constant (metrics.py:139-140)
__device__ __forceinline__ float det_ciou_grad(const DetBox& p, const DetBox& q, float (&g)[4]) {
  const float w1 = p.x2 - p.x1, h1 = p.y2 - p.y1 + kDetEps, w2 = q.x2 - q.x1, h2 = q.y2 - q.y1 + kDetEps;
  const float iwr = fminf(p.x2, q.x2) - fmaxf(p.x1, q.x1), ihr = fminf(p.y2, q.y2) - fmaxf(p.y1, q.y1);
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float inter = iw * ih, uni = w1 * h1 + w2 * h2 - inter + kDetEps, iou = inter / uni;
  const float cw = fmaxf(p.x2, q.x2) - fminf(p.x1, q.x1), ch = fmaxf(p.y2, q.y2) - fminf(p.y1, q.y1);
  const float c2 = cw * cw + ch * ch + kDetEps;
  const float sx = q.x1 + q.x2 - p.x1 - p.x2, sy = q.y1 + q.y2 - p.y1 - p.y2;
  const float rho2 = (sx * sx + sy * sy) * 0.25f;
  const float da = atanf(w2 / h2) - atanf(w1 / h1), v = kDetAtanK * da * da;
  const float alpha = v / (v - iou + (1.f + kDetEps));
  // per coordinate: d iw or ih, d (w1 h1), d cw or ch, d rho2, d atan(w1 / h1)
  const float onx = iwr >= 0.f ? 1.f : 0.f, ony = ihr >= 0.f ? 1.f : 0.f;
  const float diw[4] = {-onx * det_gt_share(p.x1, q.x1), 0.f, onx * det_gt_share(q.x2, p.x2), 0.f};
  const float dih[4] = {0.f, -ony * det_gt_share(p.y1, q.y1), 0.f, ony * det_gt_share(q.y2, p.y2)};
  const float dwh[4] = {-h1, -w1, h1, w1};
  const float dcw[4] = {-det_gt_share(q.x1, p.x1), 0.f, det_gt_share(p.x2, q.x2), 0.f};
  const float dch[4] = {0.f, -det_gt_share(q.y1, p.y1), 0.f, det_gt_share(p.y2, q.y2)};
  const float drho[4] = {-0.5f * sx, -0.5f * sy, -0.5f * sx, -0.5f * sy};
  const float r2 = 1.f / (h1 * h1 + w1 * w1);
  const float dat[4] = {-h1 * r2, w1 * r2, h1 * r2, -w1 * r2};          // atan(w1/h1): d/dw1 = h1 / (h1^2 + w1^2), d/dh1 = -w1 / (...)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float dinter = diw[k] * ih + iw * dih[k];
    const float duni = dwh[k] - dinter;
    const float diou = (dinter - iou * duni) / uni;
    const float dc2 = 2.f * (cw * dcw[k] + ch * dch[k]);
    const float dv = -2.f * kDetAtanK * da * dat[k];
    g[k] = diou - (drho[k] * c2 - rho2 * dc2) / (c2 * c2) - alpha * dv;
  }
  return iou - (rho2 / c2 + v * alpha);
}

// tal.py:279-299: the anchor's centre, in pixels, lies inside the box by more than 1e-9
__device__ __forceinline__ bool det_inside(const DetBox& g, float px, float py) {
  return fminf(fminf(px - g.x1, py - g.y1), fminf(g.x2 - px, g.y2 - py)) > 1e-9f;
}
// tal.py:156-188 for one (ground truth, anchor) pair that passed det_inside: overlap = clamp(CIoU, 0), metric = score^0.5 overlap^6
template <typename R>
__device__ __forceinline__ void det_pair(const R& f, const MapsAnchor& t, const DetBox& g, int label, float& met, float& ov) {
  const DetBox pg = maps_decode(f, t.ax, t.ay);
  const DetBox pb{pg.x1 * t.s, pg.y1 * t.s, pg.x2 * t.s, pg.y2 * t.s};
  ov = fmaxf(det_ciou(g, pb), 0.f);
  const float sc = sigmoidf_(f.at(4 * kMapsReg + label));
  const float o2 = ov * ov;
  met = sqrtf(sc) * (o2 * o2 * o2);
}

template <typename T, MapsLayout L = MapsLayout::kNCHW>
__global__ __launch_bounds__(kBlock) void k_det_assign(const DetArgs A) {
  __shared__ float s_met[kDetChunk + kDetTopkMax], s_ov[kDetChunk + kDetTopkMax];
  __shared__ int s_anc[kDetChunk + kDetTopkMax];
  __shared__ float sel_met[kDetTopkMax], sel_ov[kDetTopkMax], r_v[kBlock / kWave];
  __shared__ int sel_anc[kDetTopkMax], r_i[kBlock / kWave], s_cnt[kBlock / kWave], s_row;
  const int tid = static_cast<int>(threadIdx.x), lane = tid & (kWave - 1), wave = tid / kWave;
  const int b = static_cast<int>(blockIdx.x) / A.m_cap, g = static_cast<int>(blockIdx.x) % A.m_cap;
  const int slot = b * A.m_cap + g;
  {                                                            // this workgroup's share of the image's assignment: background
    const int per = (A.maps.A + A.m_cap - 1) / A.m_cap, hi = min((g + 1) * per, A.maps.A);
    for (int a = g * per + tid; a < hi; a += kBlock) {
      A.asg_gt[static_cast<size_t>(b) * A.maps.A + a] = -1;
      A.asg_score[static_cast<size_t>(b) * A.maps.A + a] = 0.f;
    }
  }
  // loss.py:217-232: the g-th row whose batch_idx is b
  const int n = labels_live(A.labels);
  if (tid == 0) s_row = -1;
  int base = 0;
  for (int r0 = 0; r0 < n; r0 += kBlock) {
    const int r = r0 + tid;
    const bool mine = r < n && A.labels.batch_idx[r] == static_cast<float>(b);
    const unsigned long long mask = __ballot(mine);
    __syncthreads();
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = base;
    for (int w = 0; w < kBlock / kWave; ++w) {
      if (w < wave) before += s_cnt[w];
      base += s_cnt[w];
    }
    if (mine && before + __popcll(mask & ((1ull << lane) - 1ull)) == g) s_row = r;
  }
  __syncthreads();
  const int row = s_row;
  DetBox gt{0.f, 0.f, 0.f, 0.f};
  if (row >= 0) gt = det_gt_box(A, row);
  if (row < 0 || !det_gt_valid(gt)) {                          // uniform over the workgroup
    if (tid == 0) { A.cand_n[slot] = 0; A.cand_row[slot] = row; }
    return;
  }
  const int label = det_label(A, row);
  // per level, the rectangle of cells whose centres can lie inside the box (one cell of margin; det_inside decides)
  int ix0[kMapsLevelsMax], iy0[kMapsLevelsMax], rw[kMapsLevelsMax], tot[kMapsLevelsMax + 1];
  tot[0] = 0;
#pragma unroll
  for (int l = 0; l < kMapsLevelsMax; ++l) {
    int cells = 0;
    ix0[l] = iy0[l] = 0; rw[l] = 1;
    if (l < A.maps.n_levels) {
      const float s = A.maps.stride[l];
      const int x0 = static_cast<int>(fminf(fmaxf(floorf(gt.x1 / s - 0.5f) - 1.f, 0.f), static_cast<float>(A.maps.W[l] - 1)));
      const int y0 = static_cast<int>(fminf(fmaxf(floorf(gt.y1 / s - 0.5f) - 1.f, 0.f), static_cast<float>(A.maps.H[l] - 1)));
      const int x1 = static_cast<int>(fmaxf(fminf(ceilf(gt.x2 / s - 0.5f) + 1.f, static_cast<float>(A.maps.W[l] - 1)), 0.f));
      const int y1 = static_cast<int>(fmaxf(fminf(ceilf(gt.y2 / s - 0.5f) + 1.f, static_cast<float>(A.maps.H[l] - 1)), 0.f));
      ix0[l] = x0; iy0[l] = y0; rw[l] = max(x1 - x0 + 1, 1);
      cells = max(x1 - x0 + 1, 0) * max(y1 - y0 + 1, 0);
    }
    tot[l + 1] = tot[l] + cells;
  }
  const int T_ = tot[kMapsLevelsMax];
  int ncarry = 0;
  for (int c0 = 0; c0 < T_; c0 += kDetChunk) {
    const int cn = min(kDetChunk, T_ - c0);
    for (int i = tid; i < cn; i += kBlock) {
      const int idx = c0 + i;
      int l = 0;
#pragma unroll
      for (int k = 1; k < kMapsLevelsMax; ++k)
        if (idx >= tot[k]) l = k;                              // levels past n_levels hold no cell: tot[k] = T_ > idx
      int x0 = ix0[0], y0 = iy0[0], w = rw[0], t0 = tot[0];
#pragma unroll
      for (int k = 1; k < kMapsLevelsMax; ++k)
        if (l == k) { x0 = ix0[k]; y0 = iy0[k]; w = rw[k]; t0 = tot[k]; }
      const int local = idx - t0, x = x0 + local % w, y = y0 + local / w;
      const MapsAnchor t = maps_cell(A.maps, l, y * A.maps.W[l] + x, y, x);
      float met = -1.f, ov = 0.f;
      if (det_inside(gt, t.ax * t.s, t.ay * t.s)) det_pair(maps_feat<T, L>(A.maps, t, b), t, gt, label, met, ov);
      s_met[i] = met; s_ov[i] = ov; s_anc[i] = A.maps.a0[l] + t.p;
    }
    if (tid < ncarry) { s_met[cn + tid] = sel_met[tid]; s_ov[cn + tid] = sel_ov[tid]; s_anc[cn + tid] = sel_anc[tid]; }
    __syncthreads();
    const int have = cn + ncarry;
    int nsel = 0;
    for (int k = 0; k < A.topk; ++k) {
      float v = -1.f;
      int ai = 0x7fffffff, at_ = -1;
      for (int i = tid; i < have; i += kBlock) {
        const float m = s_met[i];
        const int a = s_anc[i];
        if (m > v || (m == v && a < ai)) { v = m; ai = a; at_ = i; }
      }
      float wv = v;
      int wi = ai;
      wave_group_argmax(wv, wi, kWave);
      if (lane == 0) { r_v[wave] = wv; r_i[wave] = wi; }
      __syncthreads();
      float bv = r_v[0];
      int bi = r_i[0];
      for (int w = 1; w < kBlock / kWave; ++w) argmax_combine(bv, bi, r_v[w], r_i[w]);
      if (bv < 0.f) break;                                     // nothing left inside the box (uniform: every thread read the same words)
      if (at_ >= 0 && ai == bi && v == bv) {                   // anchors are distinct: exactly one thread owns the winner
        sel_met[k] = v; sel_ov[k] = s_ov[at_]; sel_anc[k] = ai;
        s_met[at_] = -1.f;
      }
      nsel = k + 1;
      __syncthreads();
    }
    ncarry = nsel;
    __syncthreads();
  }
  if (tid < ncarry) {
    A.cand_anchor[slot * kDetTopkMax + tid] = sel_anc[tid];
    A.cand_metric[slot * kDetTopkMax + tid] = sel_met[tid];
    A.cand_overlap[slot * kDetTopkMax + tid] = sel_ov[tid];
  }
  if (tid == 0) { A.cand_n[slot] = ncarry; A.cand_row[slot] = row; }
}

// entry e of an image: slot e / kDetTopkMax's candidate e % kDetTopkMax.  e_gt: the slot the entry belongs to after the resolve, plus
// an action in the bits above kDetSlotMask while it runs.
constexpr int kDetSlotMask = 0x1ff, kDetDrop = 0x200, kDetLead = 0x400;
template <typename T, MapsLayout L = MapsLayout::kNCHW>
__global__ __launch_bounds__(kBlock) void k_det_resolve(const DetArgs A) {
  extern __shared__ int det_smem[];
  const int M = A.m_cap, E = M * kDetTopkMax;
  int* e_anc = det_smem;
  float* e_met = reinterpret_cast<float*>(e_anc + E);
  float* e_ov = e_met + E;
  int* pos_m = reinterpret_cast<int*>(e_ov + E);
  int* pos_o = pos_m + M;
  int* s_row = pos_o + M;
  short* e_gt = reinterpret_cast<short*>(s_row + M);
  __shared__ float red[kBlock / kWave];
  const int tid = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
  for (int g = tid; g < M; g += kBlock) { s_row[g] = A.cand_row[b * M + g]; pos_m[g] = 0; pos_o[g] = 0; }
  for (int e = tid; e < E; e += kBlock) {
    const int g = e / kDetTopkMax, j = e % kDetTopkMax;
    const bool on = j < A.cand_n[b * M + g];
    const int src = (b * M + g) * kDetTopkMax + j;
    e_anc[e] = on ? A.cand_anchor[src] : -1;
    e_met[e] = on ? A.cand_metric[src] : 0.f;
    e_ov[e] = on ? A.cand_overlap[src] : 0.f;
    e_gt[e] = static_cast<short>(g);
  }
  {                                                            // an image with more rows than slots: the call's status
    const int n = labels_live(A.labels);
    float cnt = 0.f;
    for (int r = tid; r < n; r += kBlock) cnt += A.labels.batch_idx[r] == static_cast<float>(b) ? 1.f : 0.f;
    cnt = block_sum(cnt, tid, red);
    if (tid == 0) A.ovf[b] = cnt > static_cast<float>(M) ? 1 : 0;
  }
  __syncthreads();
  // tal.py:317-326: an anchor several slots claim.  The first of its entries leads, the others go.
  for (int e = tid; e < E; e += kBlock) {
    const int a = e_anc[e];
    if (a < 0) continue;
    int lead = e;
    bool contested = false;
    for (int o = 0; o < E; ++o)
      if (o != e && e_anc[o] == a) { contested = true; lead = min(lead, o); }
    if (contested) e_gt[e] = static_cast<short>(e_gt[e] | (lead == e ? kDetLead : kDetDrop));
  }
  __syncthreads();
  for (int e = tid; e < E; e += kBlock) {
    const int act = e_gt[e];
    if (act & kDetDrop) { e_anc[e] = -1; continue; }
    if (!(act & kDetLead)) continue;
    // the arg-max over every slot of the overlap, 0 where the anchor is not inside a valid box; the first slot wins a tie
    const MapsAnchor t = maps_anchor(A.maps, e_anc[e]);
    const auto f = maps_feat<T, L>(A.maps, t, b);
    float best_ov = -1.f, best_met = 0.f;
    int best = 0;
    for (int g = 0; g < M; ++g) {
      const int row = s_row[g];
      if (row < 0) break;                                      // rows fill the slots from 0: the rest are empty, overlap 0, never first
      float met = 0.f, ov = 0.f;
      const DetBox gt = det_gt_box(A, row);
      if (det_gt_valid(gt) && det_inside(gt, t.ax * t.s, t.ay * t.s)) det_pair(f, t, gt, det_label(A, row), met, ov);
      if (ov > best_ov) { best_ov = ov; best_met = met; best = g; }
    }
    e_gt[e] = static_cast<short>(best);
    e_met[e] = best_met; e_ov[e] = fmaxf(best_ov, 0.f);
  }
  __syncthreads();
  // tal.py:121-125: per slot the largest metric and overlap among its anchors (maxima of non-negative floats: their bit patterns order)
  for (int e = tid; e < E; e += kBlock) {
    if (e_anc[e] < 0) continue;
    const int g = e_gt[e] & kDetSlotMask;
    atomicMax(&pos_m[g], __float_as_int(e_met[e]));
    atomicMax(&pos_o[g], __float_as_int(e_ov[e]));
  }
  __syncthreads();
  float sum = 0.f;
  for (int e = tid; e < E; e += kBlock) {
    const int a = e_anc[e];
    if (a < 0) continue;
    const int g = e_gt[e] & kDetSlotMask;
    const float sc = e_met[e] * __int_as_float(pos_o[g]) / (__int_as_float(pos_m[g]) + 1e-9f);
    A.asg_gt[static_cast<size_t>(b) * A.maps.A + a] = s_row[g];
    A.asg_score[static_cast<size_t>(b) * A.maps.A + a] = sc;
    sum += sc;
  }
  sum = block_sum(sum, tid, red);
  if (tid == 0) A.tss_part[b] = sum;
}

// loss.py:95-105 for one side: the target distance clamped to [0, 14.99], its two neighbouring bins and their weights
__device__ __forceinline__ void det_dfl_target(float dist, int& tl, float& wl) {
  const float t = fminf(fmaxf(dist, 0.f), 14.99f);
  tl = static_cast<int>(t);
  wl = static_cast<float>(tl + 1) - t;
}
__device__ __forceinline__ float det_side_target(const DetBox& tb, float ax, float ay, int side) {    // tal.py:394-397
  return side == 0 ? ax - tb.x1 : side == 1 ? ay - tb.y1 : side == 2 ? tb.x2 - ax : tb.y2 - ay;
}

// what a thread of the two sweeps owns: anchor `idx` of (B, A)
struct DetAnchor : MapsAnchor { int b, gi; float sc; };
__device__ __forceinline__ DetAnchor det_anchor(const DetArgs& A, long long idx) {
  return DetAnchor{maps_anchor(A.maps, static_cast<int>(idx % A.maps.A)), static_cast<int>(idx / A.maps.A), A.asg_gt[idx], A.asg_score[idx]};
}

// k_det_loss's terms of one anchor, its channels read through `f`
template <typename R>
__device__ __forceinline__ void det_loss_anchor(const DetArgs& A, const DetAnchor& t, const R& f, float& lbox, float& lcls, float& ldfl) {
  const int label = t.gi >= 0 ? det_label(A, t.gi) : -1;
  for (int c = 0; c < A.maps.nc; ++c) {                             // BCEWithLogits against onehot(label) * score (loss.py:284)
    const float x = f.at(4 * kMapsReg + c);
    lcls += fmaxf(x, 0.f) - (c == label ? x * t.sc : 0.f) + log1pf(expf(-fabsf(x)));
  }
  if (t.gi >= 0) {
    const DetBox gp = det_gt_box(A, t.gi);
    const DetBox tb{gp.x1 / t.s, gp.y1 / t.s, gp.x2 / t.s, gp.y2 / t.s};            // loss.py:288
    float d[4], dfl = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float p[kMapsReg], lse, wl;
      int tl;
      float vl = 0.f, vr = 0.f;
      det_dfl_target(det_side_target(tb, t.ax, t.ay, s), tl, wl);
#pragma unroll
      for (int j = 0; j < kMapsReg; ++j) {
        const float v = f.at(s * kMapsReg + j);
        vl = j == tl ? v : vl; vr = j == tl + 1 ? v : vr;
      }
      maps_side(f, s, p, d[s], lse);
      dfl += (lse - vl) * wl + (lse - vr) * (1.f - wl);
    }
    const DetBox pb{t.ax - d[0], t.ay - d[1], t.ax + d[2], t.ay + d[3]};
    lbox = (1.f - det_ciou(pb, tb)) * t.sc;                  // loss.py:127-129
    ldfl = dfl * 0.25f * t.sc;                               // loss.py:134: the mean over the four sides
  }
}

// NHWC sweeps: the workgroup's kBlock anchors go through LDS (detmaps.cuh: maps_stage_in) kDetStageWords of fp32 at a time -- whole rows, so a
// round holds det_stage_rows(no) anchors: all 256 up to no = 65 (nc = 1), 114 at nc = 80 -- and a thread does its anchor in the round that
// holds it: thread = anchor and block_sum's tree are the NCHW sweep's, so are the partials' bits.  66560 bytes: two workgroups fit a CU's 160 KiB.
constexpr int kDetStageWords = kBlock * (4 * kMapsReg + 1);
__device__ __forceinline__ int det_stage_rows(int no) { return min(kBlock, kDetStageWords / maps_stage_pitch(no)); }

template <typename T, MapsLayout L = MapsLayout::kNCHW>
__global__ __launch_bounds__(kBlock) void k_det_loss(const DetArgs A) {
  __shared__ float red[kBlock / kWave];
  const int tid = static_cast<int>(threadIdx.x);
  const long long idx = static_cast<long long>(blockIdx.x) * kBlock + tid, total = static_cast<long long>(A.maps.B) * A.maps.A;
  float lbox = 0.f, lcls = 0.f, ldfl = 0.f;
  if constexpr (L == MapsLayout::kNHWC) {
    __shared__ float stage[kDetStageWords];
    const long long i0 = static_cast<long long>(blockIdx.x) * kBlock, i1 = min(i0 + kBlock, total);
    const int rows = det_stage_rows(A.maps.no), pitch = maps_stage_pitch(A.maps.no);
    if (rows == 0 && idx < total) {                                 // a row longer than the stage (nc > 16575): read in place
      const DetAnchor t = det_anchor(A, idx);
      det_loss_anchor(A, t, maps_feat<T, L>(A.maps, t, t.b), lbox, lcls, ldfl);
    }
    for (long long r0 = i0; rows > 0 && r0 < i1; r0 += rows) {      // uniform over the workgroup
      const long long r1 = min(r0 + rows, i1);
      maps_segments(A.maps, r0, r1, [&](int l, size_t off, unsigned n, int row0) {
        maps_stage_in<T>(static_cast<const T*>(A.maps.feat[l]) + off, n, row0, A.maps.no, stage, tid);
      });
      __syncthreads();
      if (idx >= r0 && idx < r1) det_loss_anchor(A, det_anchor(A, idx), MapsStaged{stage + static_cast<int>(idx - r0) * pitch}, lbox, lcls, ldfl);
      __syncthreads();                                              // the next round overwrites the rows
    }
  } else {
    if (idx < total) {
      const DetAnchor t = det_anchor(A, idx);
      det_loss_anchor(A, t, maps_feat<T>(A.maps, t, t.b), lbox, lcls, ldfl);
    }
  }
  lbox = block_sum(lbox, tid, red);
  lcls = block_sum(lcls, tid, red);
  ldfl = block_sum(ldfl, tid, red);
  if (tid == 0) {
    A.partial[blockIdx.x * 3 + 0] = lbox; A.partial[blockIdx.x * 3 + 1] = lcls; A.partial[blockIdx.x * 3 + 2] = ldfl;
  }
}

__global__ __launch_bounds__(kBlock) void k_det_final(const DetArgs A) {
  __shared__ float red[kBlock / kWave];
  const int tid = static_cast<int>(threadIdx.x);
  float s[3] = {0.f, 0.f, 0.f}, tss = 0.f, bad = 0.f;
  for (int i = tid; i < A.nblk; i += kBlock) {
    s[0] += A.partial[i * 3]; s[1] += A.partial[i * 3 + 1]; s[2] += A.partial[i * 3 + 2];
  }
  for (int b = tid; b < A.maps.B; b += kBlock) { tss += A.tss_part[b]; bad += A.ovf[b] ? 1.f : 0.f; }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = block_sum(s[k], tid, red);
  tss = block_sum(tss, tid, red);
  bad = block_sum(bad, tid, red);
  if (tid != 0) return;
  const float nan = __int_as_float(0x7fc00000);
  tss = fmaxf(tss, 1.f);                                       // loss.py:280
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float item = bad > 0.f ? nan : s[k] / tss * A.gain[k];
    A.items[k] = item;
    A.out[k] = item * static_cast<float>(A.maps.B);            // loss.py:297
  }
  A.fin[0] = bad > 0.f ? nan : tss;
  A.fin[1] = bad;
  *A.status = bad > 0.f ? 1 : 0;
}

// where k_det_bwd's gradients of one anchor go: the planes of an NCHW map, rounded to T, or the anchor's row in LDS
template <typename T>
struct DetGradPlanes {
  T* __restrict__ g; size_t hw;
  __device__ __forceinline__ void put(int c, float v) const { g[c * hw] = from_f32<T>(v); }
};
// (stored as a value of T, as DetGradPlanes stores it: detmaps.cuh, maps_stage_put)
template <typename T>
struct DetGradStaged {
  float* g;
  __device__ __forceinline__ void put(int c, float v) const { maps_stage_put<T>(g + c, v); }
};
template <typename T>
struct DetGradRow {                                            // an NHWC anchor's row in global memory
  T* g;
  __device__ __forceinline__ void put(int c, float v) const { g[c] = from_f32<T>(v); }
};
// every channel's gradient of one anchor.  tss, fbox, fcls, fdfl: the call's factors (k_det_bwd).  With f and g on the same LDS row a channel is
// written after its last read: the class channels one by one, a side's bins after maps_decode and the side's own maps_side.
template <typename R, typename G>
__device__ __forceinline__ void det_bwd_anchor(const DetArgs& A, const DetAnchor& t, const R& f, const G& g, float tss, float fbox, float fcls, float fdfl) {
  const int label = t.gi >= 0 ? det_label(A, t.gi) : -1;
  for (int c = 0; c < A.maps.nc; ++c) {
    const float x = f.at(4 * kMapsReg + c);
    g.put(4 * kMapsReg + c, fcls * (sigmoidf_(x) - (c == label ? t.sc : 0.f)));
  }
  if (t.gi < 0 || !(tss == tss)) {                             // background, or the poisoned call: no box terms (NaN where poisoned)
    const float z = t.gi < 0 && tss == tss ? 0.f : tss;
    for (int c = 0; c < 4 * kMapsReg; ++c) g.put(c, z);
    return;
  }
  const DetBox gp = det_gt_box(A, t.gi);
  const DetBox tb{gp.x1 / t.s, gp.y1 / t.s, gp.x2 / t.s, gp.y2 / t.s};
  const DetBox pb = maps_decode(f, t.ax, t.ay);
  float gc[4];
  det_ciou_grad(pb, tb, gc);
  // the loss is (1 - CIoU) score: x1 = ax - d_l, y1 = ay - d_t, x2 = ax + d_r, y2 = ay + d_b
  const float wbox = fbox * t.sc, wdfl = fdfl * t.sc * 0.25f;
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {                                // a side at a time: 16 bins live, not 64
    float p[kMapsReg], d, lse, wl;
    int tl;
    const float gds = s == 0 ? gc[0] : s == 1 ? gc[1] : s == 2 ? -gc[2] : -gc[3];
    maps_side(f, s, p, d, lse);
    det_dfl_target(det_side_target(tb, t.ax, t.ay, s), tl, wl);
#pragma unroll
    for (int j = 0; j < kMapsReg; ++j) {
      const float hit = j == tl ? wl : (j == tl + 1 ? 1.f - wl : 0.f);
      g.put(s * kMapsReg + j, wdfl * (p[j] - hit) + wbox * gds * p[j] * (static_cast<float>(j) - d));
    }
  }
}

template <typename T, MapsLayout L = MapsLayout::kNCHW>
__global__ __launch_bounds__(kBlock) void k_det_bwd(const DetArgs A) {
  const long long idx = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x, total = static_cast<long long>(A.maps.B) * A.maps.A;
  if constexpr (L == MapsLayout::kNCHW) {
    if (idx >= total) return;
  }
  const float tss = uniform_load(A.fin), Bf = static_cast<float>(A.maps.B);      // tss: divided by, not multiplied with its reciprocal (one rounding less)
  const float fbox = uniform_load(A.upstream) * A.gain[0] * Bf / tss, fcls = uniform_load(A.upstream + 1) * A.gain[1] * Bf / tss,
              fdfl = uniform_load(A.upstream + 2) * A.gain[2] * Bf / tss;
  if constexpr (L == MapsLayout::kNHWC) {                      // through LDS in rounds of whole rows, as k_det_loss; the gradients leave from the same rows
    __shared__ float stage[kDetStageWords];
    const int tid = static_cast<int>(threadIdx.x);
    const long long i0 = static_cast<long long>(blockIdx.x) * kBlock, i1 = min(i0 + kBlock, total);
    const int rows = det_stage_rows(A.maps.no), pitch = maps_stage_pitch(A.maps.no);
    if (rows == 0 && idx < total) {                                 // a row longer than the stage (nc > 16575): read and written in place
      const DetAnchor t = det_anchor(A, idx);
      det_bwd_anchor(A, t, maps_feat<T, L>(A.maps, t, t.b), DetGradRow<T>{static_cast<T*>(A.gfeat[t.l]) + maps_offset<L>(A.maps, t, t.b)}, tss, fbox, fcls, fdfl);
    }
    for (long long r0 = i0; rows > 0 && r0 < i1; r0 += rows) {      // uniform over the workgroup
      const long long r1 = min(r0 + rows, i1);
      maps_segments(A.maps, r0, r1, [&](int l, size_t off, unsigned n, int row0) {
        maps_stage_in<T>(static_cast<const T*>(A.maps.feat[l]) + off, n, row0, A.maps.no, stage, tid);
      });
      __syncthreads();
      if (idx >= r0 && idx < r1) {
        float* row = stage + static_cast<int>(idx - r0) * pitch;
        det_bwd_anchor(A, det_anchor(A, idx), MapsStaged{row}, DetGradStaged<T>{row}, tss, fbox, fcls, fdfl);
      }
      __syncthreads();
      maps_segments(A.maps, r0, r1, [&](int l, size_t off, unsigned n, int row0) {
        maps_stage_out<T>(static_cast<T*>(A.gfeat[l]) + off, n, row0, A.maps.no, stage, tid);
      });
      __syncthreads();                                              // the next round overwrites the rows
    }
  } else {
    const DetAnchor t = det_anchor(A, idx);
    const size_t off = maps_offset(A.maps, t, t.b);
    det_bwd_anchor(A, t, MapsPlanes<T>{static_cast<const T*>(A.maps.feat[t.l]) + off, t.hw}, DetGradPlanes<T>{static_cast<T*>(A.gfeat[t.l]) + off, t.hw},
                      tss, fbox, fcls, fdfl);
  }
}

}  // namespace mgacbam
