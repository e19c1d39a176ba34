// libmgacbam.so, C ABI (include/ext/mgaconfusion.h): the validator's confusion matrix, in two launches
#include "detmaps_host.cuh"
#include "confusion.cuh"

#include "../../include/ext/mgaconfusion.h"

static_assert(kMatchMaxGt == MGADET_MAX_GT && kCmMaxNc == MGACM_MAX_NC, "CmArgs against the ABI");
static_assert(kCmCells * sizeof(int) + kMatchWaves * sizeof(long long) <= 65536, "k_cm_count's cells fit a workgroup's static LDS");
static_assert(sizeof(mgacm_desc_t) == 152, "the descriptor's layout (mirrored by _lib.ConfusionDesc)");

// Everything a descriptor is checked for that does not involve a pointer's value; fills the kernel arguments' geometry and the ws size.
static int cm_check(const char* what, const mgacm_desc_t* D, CmArgs& A, size_t& ws_total) {
  if (!D) return fail(MGACBAM_E_NULL, "%s: desc is NULL", what);
  if (int e = labels_check(what, D->B, D->max_det, D->n_cap, D->m_cap, D->reserved, D->img_w, D->img_h)) return e;
  if (D->nc < 1 || D->nc > MGACM_MAX_NC) return fail(MGACBAM_E_ARG, "%s: nc=%d (1 .. %d: (nc + 1)^2 cells of LDS)", what, D->nc, MGACM_MAX_NC);
  if (D->flags & ~MGACM_SINGLE_CLS) return fail(MGACBAM_E_ARG, "%s: flags=0x%x", what, D->flags);
  if (!isfinite(D->conf_thres)) return fail(MGACBAM_E_ARG, "%s: conf_thres=%g (finite)", what, D->conf_thres);
  if (!(D->iou_thres >= 0.f && D->iou_thres < 1.f)) return fail(MGACBAM_E_ARG, "%s: iou_thres=%g (in [0, 1))", what, D->iou_thres);
  A.B = D->B; A.max_det = D->max_det; A.m_cap = D->m_cap; A.nc = D->nc;
  A.single_cls = D->flags & MGACM_SINGLE_CLS ? 1 : 0;
  A.img_w = D->img_w; A.img_h = D->img_h; A.conf_thres = D->conf_thres; A.iou_thres = D->iou_thres;
  Carver cv;
  cv.take(2 * static_cast<size_t>(D->B));                                        // the images' overflow words, then their bad-class words
  ws_total = cv.total;
  return 0;
}

extern "C" size_t mgacm_ws_bytes(const mgacm_desc_t* desc) {
  CmArgs A;
  size_t total;
  if (cm_check("mgacm_ws_bytes", desc, A, total)) return 0;
  g_err[0] = 0;
  return total;
}

static int cm_bind(const char* what, const mgacm_desc_t* D, CmArgs& A, size_t ws_total) {
  if (!D->dets || !D->count || !D->det_out || !D->cm || !D->status || !D->ws)
    return fail(MGACBAM_E_NULL, "%s: dets, count, det_out, cm, status, ws must not be NULL", what);
  if (int e = labels_bind(what, D, A.labels, ", lab_out", !D->lab_out)) return e;
  if (!aligned_to(D->acc, 8)) return fail(MGACBAM_E_ALIGN, "%s: acc (int64) must be 8-byte aligned", what);
  const void* words[] = {D->dets, D->count, D->batch_idx, D->cls, D->bboxes, D->n, D->det_out, D->lab_out, D->cm, D->status};
  if (int e = check_words_and_ws(what, words, D->ws, ws_total, D->ws_bytes)) return e;
  A.dets = D->dets; A.count = D->count;
  A.det_out = D->det_out; A.lab_out = D->lab_out; A.cm = D->cm; A.acc = reinterpret_cast<long long*>(D->acc); A.status = D->status;
  A.over = at<int>(D->ws, 0); A.bad = A.over + D->B;
  return 0;
}

extern "C" int mgacm_run(const mgacm_desc_t* D, void* stream) {
  const char* what = "mgacm_run";
  CmArgs A;
  size_t ws_total;
  if (int e = cm_check(what, D, A, ws_total)) return e;
  if (int e = cm_bind(what, D, A, ws_total)) return e;
  const hipStream_t st = static_cast<hipStream_t>(stream);
  if (int e = launch("k_cm_match", k_cm_match, A.B, kBlock, 0, st, A)) return e;
  if (int e = launch("k_cm_count", k_cm_count, 1, kBlock, 0, st, A)) return e;
  g_err[0] = 0;
  return 0;
}
