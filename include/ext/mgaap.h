/* libmgacbam.so -- average precision per class on the device, from the rows a validation run accumulated: what the reference's ap_per_class
 * does on the host in numpy after reading every row back.  The fourth stage behind mganms_run, mgamatch_run (include/ext/mgamatch.h) and
 * mgacm_run (include/ext/mgaconfusion.h), in a header of its own: the headers beside and above it are unchanged by it.  It follows their
 * conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed in, return value
 * 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked before the first launch.
 * No host read-back: a call can sit in a captured graph behind mgamatch_run, or be made once at the end of a run. */
#ifndef MGAAP_H_
#define MGAAP_H_
#include "mgatargets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * What the reference computes from a run's rows (U = ultralytics: ap_per_class and compute_ap U/utils/metrics.py:727-854, called from
 * DetMetrics.process U/utils/metrics.py:1087-1117), in fp64, restated so that it can run in parallel:
 *   inputs       the accumulation mgamatch_run appends to: n_rows detection rows rows_tp (niou bytes a row, non-zero = true), rows_conf,
 *                rows_cls and n_targets label classes tgt_cls; n_rows = state[0] and n_targets = state[1] are read on the device, clamped to
 *                0 .. rows_cap and 0 .. tgt_cap, never on the host.  rows_img and tgt_img travel with the descriptor and are not read.
 *   order        within a class the rows are ordered by descending conf; equal confidences of one class stay in accumulation order (image
 *                serial, then detection index: the order of mgamatch_run's append); -0.0 compares equal to +0.0.
 *   ties         the reference's order among equal confidences is that of an unstable sort (np.argsort), so this case is defined here
 *                and excluded from reference parity.
 *   counted      a detection row whose class is not an integer in 0 .. nc - 1 belongs to no class and is ignored (the reference never
 *                visits it).  nt[c]: the target rows of class c.  A class with nt[c] = 0 produces no output row (its rows of the dense
 *                result are zeros); a class with nt[c] > 0 and no detections produces zero rows.
 *   per class    with n_p rows, at rank i = 1 .. n_p and threshold t: tpc[i, t] the running count of true positives;
 *                recall = tpc / (nt + 1e-16); precision = tpc / i (the reference's tpc / (tpc + fpc)): each one correctly rounded fp64
 *                division of exact integers.  A class has at most nt true rows per threshold, as the matching guarantees, so recall
 *                stays within [0, 1] and mrec is sorted; np.interp is undefined on abscissae that are not, and so is this.
 *   envelope     mrec = [0, recall, 1]; mpre = [1, precision, 0] made non-increasing by a running maximum from the right.
 *   ap[c, t]     the trapezoid sum over x = grid_ap (linspace(0, 1, 101)) of interp(x, mrec, mpre), the terms
 *                (x[k+1] - x[k]) * (y[k+1] + y[k]) / 2 added in ascending k.
 *   curves       at threshold 0, over x = grid_curve (linspace(0, 1, 1000)): prec_values[c] = interp(x, mrec, mpre);
 *                r_curve[c] = interp(-x, -conf, recall, left = 0); p_curve[c] = interp(-x, -conf, precision, left = 1).
 *   interp       numpy's np.interp(x, xp, fp): below xp[0] the left value (fp[0] unless given), above xp[last] fp[last]; otherwise with
 *                j the LAST index with xp[j] <= x (repeated abscissae: recall reaches exactly 1.0 whenever every label is found, because
 *                nt + 1e-16 == nt in fp64, so this is the common case): fp[j] if j is the last index or x == xp[j], else
 *                (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]) * (x - xp[j]) + fp[j], every operation rounded once (the unit is compiled without
 *                contraction).  numpy's second try where that expression is NaN (infinite abscissae) is not built: confidences are finite.
 *   the grids    are built once by the caller (np.linspace) and passed in, so the kernels and the host statement use the same doubles.
 *
 * result, dense and 8-byte aligned, 8 * nc * (niou + 3001) bytes: ap (nc, niou), p_curve (nc, 1000), r_curve (nc, 1000), prec_values
 * (nc, 1000) as fp64, then nt (nc) and n_det (nc) as int32 (n_det: the class's detection rows; the reference's prec_values has a row only
 * where nt > 0 and n_det > 0).  Every cell is stored by every call.  The caller compacts the rows to the classes with nt > 0, ascending:
 * np.unique(target_cls).  f1_curve, the smoothed maximum and p, r, f1, tp, fp at it are O(nc * 1000) and the caller's.
 *
 * status (1): 0 ok.  3: a live target class is not a finite integer in 0 .. nc - 1.  4: a live row's confidence is NaN.  3 takes precedence
 * over 4.  On a non-zero status the fp64 cells of result are NaN, nt and n_det are -1, and nothing else is touched.
 *
 * Launches: 3 + 3 * passes + 7 * niou, ordered by the stream only: no hand-off between workgroups inside a launch, no spinning, no
 * floating-point atomics; every step across workgroups is reduce / one-workgroup scan / apply, so the result is the same bits on every
 * run.  k_ap_init zeroes the counters.  k_ap_keys: per live row a sort key -- the class, and the complement of the order-preserving image of
 * the fp32 confidence -- with the row index as payload; rows of no class go behind class nc - 1; integer histograms of the targets (nt) and
 * of the detections' classes; the status flags.  k_ap_starts: the status word and the classes' first positions.  A stable LSD radix sort of
 * (key, payload) in ping-pong buffers, 8-bit digits, four confidence passes plus the class passes nc needs (none for nc = 1, one up to 256,
 * two above); per pass k_ap_hist (a digit histogram per tile of MGAAP_TILE rows), k_ap_scan (one workgroup scans the digit-major table),
 * k_ap_scatter (ranks within a tile from wave ballots per digit bit and per-wave digit counters in LDS, accumulated in wave order).  Per
 * threshold, through one column buffer: k_ap_tp_reduce / k_ap_tp_scan / k_ap_tp_apply, an inclusive scan of the tp column over the sorted
 * order (a class's running count is the scan minus its value before the class's first row); k_ap_env_reduce / k_ap_env_scan /
 * k_ap_env_apply, the running maximum of precision from the right, its carry reset at class boundaries; k_ap_curves, one workgroup per
 * class: a binary search per grid point.  Rows past n_rows are never read.
 *
 * ws, no initialisation needed, with a16(v) = v rounded up to 16 and T = ceil(rows_cap / MGAAP_TILE):
 *   mgaap_ws_bytes = a16(32) + a16(4 * (nc + 2)) + 6 * a16(4 * rows_cap) + a16(8 * rows_cap) + a16(1024 * T) + a16(4 * T) + 2 * a16(16 * T)
 * (control words; class starts; key, payload (two each), class and count columns; the envelope column; digit table; tile sums; tile envelopes
 * and carries).  niou does not enter: the thresholds run through one column.
 *
 * Refusals: niou outside 1 .. MGAMATCH_MAX_IOU, nc outside 1 .. MGAAP_MAX_NC, reserved != 0: MGACBAM_E_ARG; rows_cap or tgt_cap < 1 or
 * >= 2^31 / niou: MGACBAM_E_SHAPE; a NULL rows_tp, rows_conf, rows_cls, tgt_cls, state, grid_ap, grid_curve, result, status or ws:
 * MGACBAM_E_NULL; an fp32 / int32 buffer not 4-byte aligned, grid_ap, grid_curve or result not 8-byte aligned, ws not 16-byte aligned:
 * MGACBAM_E_ALIGN; ws smaller than mgaap_ws_bytes: MGACBAM_E_SIZE.
 * Not built: nt_per_image (the unique image / class pairs stay with the read-back of the rows), the `continuous` AP method, the segment /
 * pose / OBB metric classes, nc above MGAAP_MAX_NC, an eps other than 1e-16.
 * ------------------------------------------------------------------------------------------------ */
#define MGAAP_MAX_NC 1024
#define MGAAP_TILE 2048
#define MGAAP_AP_POINTS 101
#define MGAAP_CURVE_POINTS 1000

typedef struct mgaap_desc {
  const uint8_t* rows_tp;                  /* (rows_cap, niou)                                                                      */
  const float* rows_conf;                  /* (rows_cap)                                                                            */
  const float* rows_cls;                   /* (rows_cap)                                                                            */
  const int32_t* rows_img;                 /* (rows_cap), not read; may be NULL                                                     */
  const float* tgt_cls;                    /* (tgt_cap)                                                                             */
  const int32_t* tgt_img;                  /* (tgt_cap), not read; may be NULL                                                      */
  const int32_t* state;                    /* (4): n_rows, n_targets, seen, 0 -- read on the device                                 */
  int32_t rows_cap, tgt_cap;               /* rows the accumulation buffers hold                                                    */
  int32_t niou;                            /* 1 .. MGAMATCH_MAX_IOU                                                                 */
  int32_t nc;                              /* 1 .. MGAAP_MAX_NC                                                                     */
  const double* grid_ap;                   /* (MGAAP_AP_POINTS): linspace(0, 1, 101)                                                */
  const double* grid_curve;                /* (MGAAP_CURVE_POINTS): linspace(0, 1, 1000)                                            */
  void* result;                            /* 8 * nc * (niou + 3001) bytes out, 8-byte aligned                                      */
  int32_t* status;                         /* (1) out: 0, 3 or 4                                                                    */
  void* ws;                                /* 16-byte aligned                                                                       */
  size_t ws_bytes;                         /* capacity of ws (checked: MGACBAM_E_SIZE)                                              */
  int32_t reserved;                        /* 0                                                                                     */
} mgaap_desc_t;

/* bytes of ws the descriptor's call needs; 0 for a descriptor mgaap_run would refuse for anything but a buffer (the message then says
 * why) */
size_t mgaap_ws_bytes(const mgaap_desc_t* desc);
int mgaap_run(const mgaap_desc_t* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGAAP_H_ */
