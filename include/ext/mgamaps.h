/* libmgacbam.so -- the Detect maps in either memory layout: the detection criterion (include/mgadet.h) and the detection post-process
 * (include/mganms.h) on maps that are torch's channels_last, read and written in place.  A header of its own, in a directory of its own:
 * include/mgacbam.h (ABI 15), mgadet.h and mganms.h are unchanged by it -- no struct, constant or function of theirs moves --, and it
 * follows their conventions: plain C, caller-owned buffers, nothing allocated, copied or synchronised, every launch on the stream passed
 * in, return value 0 / MGACBAM_E_* / hipError_t, the message of a failure through mgacbam_last_error().  Every argument is checked before
 * the first launch. */
#ifndef MGAMAPS_H_
#define MGAMAPS_H_
#include "mgadet.h"
#include "mganms.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * The three entry points take the descriptors of mgadet.h and mganms.h and one more argument, `flags`:
 *   0                    exactly mgadet_forward, mgadet_backward and mganms_run: the same checks in the same order, the same launches.
 *   MGAMAPS_LAYOUT_NHWC  every feats[l], and every g_feats[l], is (B, H[l], W[l], 64 + nc) in memory: an anchor's 64 + nc channels are
 *                        contiguous, consecutive cells lie 64 + nc elements apart.  Everything else of the descriptor means what it
 *                        means there.
 *
 * Results: an NHWC call gives the SAME BITS as the NCHW call on the same values, in every output -- out, items, assign_gt, assign_score,
 * status, every gradient element; dets, count, keep --: every expression and every order of summation is the NCHW kernels'.
 *
 * Sizes: the workspace does not depend on the layout.  mgadet_ws_bytes and mganms_ws_bytes serve both, and a workspace (with what the
 * criterion's forward left in it) may be shared by calls of either layout.
 *
 * Alignment stays "to the element": a level may start at any element of a larger buffer.  The kernels use 16-byte accesses only where
 * an address of the level itself is 16-byte aligned; no byte before a level's first or after its last element is read or written.
 *
 * Launches: as mgadet.h and mganms.h state them; the kernels are the NHWC instantiations of the same templates.
 *
 * Refusals: a flag bit other than MGAMAPS_LAYOUT_NHWC: MGACBAM_E_ARG, before the descriptor is looked at; then every refusal of mgadet.h
 * or mganms.h, in their order; then, for mgamaps_nms_run, MGAMAPS_LAYOUT_NHWC together with a non-NULL pred: MGACBAM_E_ARG -- a decoded
 * prediction is (B, 4 + nc, A) and has no such layout.
 * Not built: levels of different layouts in one call.
 * ------------------------------------------------------------------------------------------------ */
#define MGAMAPS_LAYOUT_NHWC 1

int mgamaps_det_forward(const mgadet_desc_t* desc, int32_t flags, void* stream);
int mgamaps_det_backward(const mgadet_desc_t* desc, int32_t flags, void* stream);
int mgamaps_nms_run(const mganms_desc_t* desc, int32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MGAMAPS_H_ */
