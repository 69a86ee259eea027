/*
 * msckf_keyframes.h -- the cam states a prune frame removes, chosen on the
 * device and fused into the prune select of the feature map (same library,
 * conventions of msckf_hip.h and msckf_map.h; errors through msckf_last_error()).
 *
 *   msckf_keyframe_select   find_redundant_cam_states (msckf.py:691-727) on the
 *                           cam states of the device, then msckf_map_prune_select
 *                           with the two slots it chose, in one launch; the
 *                           outstanding batch's results ride in the same copy
 *
 * This text is the specification; tests/keyframe_ref.py restates the choice in
 * numpy, tests/feature_map_ref.py the select.
 *
 * ---------------------------------------------------------------------------
 * The choice
 *
 * Per named filter, n = its cam states (n < 4 for any named filter: -1 before
 * anything is copied or launched).  The cam records are read from the device
 * state as the context stores them -- float or double, the values
 * msckf_get_state returns -- each widened to double; all arithmetic is fp64.
 *   key = slot n - 4; the candidates are c_j = slot n - 3 + j, j = 0, 1.
 *   R(q) = to_rotation of q / |q| (JPL, [x y z w]):
 *          (2 w^2 - 1) I - 2 w [x]_x + 2 x x^T.
 *   M = R(q_c) R(q_key)^T, and u = to_quaternion(M) before its normalisation,
 *   with the four branches of geometry.to_quaternion in their order:
 *          M22 < 0 and M00 > M11:   u3 = M12 - M21   (the others as there)
 *          M22 < 0 otherwise:       u3 = M20 - M02
 *          M00 < -M11:              u3 = M01 - M10
 *          otherwise:               u3 = 1 + M00 + M11 + M22
 *   w = u3 / |u|;  ang = 2 acos(w);  dist = |p_c - p_key|.
 *   c_j is removed if ang < rot_thr && dist < trans_thr && tracking_rate >
 *   rate_thr; otherwise the oldest slot not yet taken is removed, starting at
 *   slot 0.  A comparison with a NaN is false, as on the host (a NaN pose or
 *   rate removes the oldest slots).
 * The two slots are distinct and returned in ascending order, cam_slots_out
 * [nfilt][2].  The reference's literals are rot_thr 0.2618, trans_thr 0.4,
 * rate_thr 0.5; tracking_rate [nfilt] is the host's tracked / (n_before + 1e-5)
 * of the frame's msckf_map_add_lost.
 *
 * Both sides evaluate the same fp64 formulas on the same stored values; their
 * roundings may differ in the last bits (contraction, the order of a sum), which
 * moves ang by about 1e-14.  A pose that far from a threshold is the only one
 * the two can decide differently.
 *
 * ---------------------------------------------------------------------------
 * The select
 *
 * With those two slots the call is msckf_map_prune_select: the same table
 * writes (k = 1: the observation is dropped; k >= 2: the row is involved; no
 * row moves), the same descriptors n_inv_out / desc_id_out / desc_info_out
 * ([nfilt], [nfilt][cap], [nfilt][cap][MSCKF_MAP_INFO]), and the same open
 * select: the removed slots stay recorded with the filter for msckf_map_load
 * (both prune forms) and msckf_map_prune_commit.
 *
 * Failure rules, those of msckf_map.h: arguments of every filter are checked
 * before anything is copied or launched (-1: no feature map, a slot out of
 * range or named twice, fewer than 4 cam states, a null array); an error leaves
 * every current table and every open select as they were.  Once the launch was
 * made the lost table of every named filter is gone, whether the call then
 * succeeds or not.  If the outstanding batch's results carry an error (below),
 * the call returns it and no table becomes current: nothing was selected.
 *
 * Ordering: the kernel runs on the context's stream after everything enqueued
 * before the call (a laned update chain is joined first), so it reads the cam
 * states as that chain left them.
 *
 * Transfers: one input block and one host-to-device copy (headers and rates);
 * one kernel, the choice and the select in it, no host round trip between
 * them; one device-to-host copy and one synchronisation return the slots, the
 * counts, the descriptors and -- if asked -- the results.
 *
 * ---------------------------------------------------------------------------
 * The outstanding batch's results
 *
 * accepted_out / gamma_out / p_w_out / valid_out / rows_out are those of
 * msckf_readback (sized for the loaded batch; rows_out [n_filters]): if any is
 * given, the loaded batch's results are read in the call's single copy, exactly
 * as msckf_batch_results would return them, errors included (-3, -4).  All
 * NULL: nothing of the batch is read.
 *
 * Kernel (csrc/msckf_map.hip): one workgroup of four wavefronts per named
 * filter.  One lane computes the choice (about a hundred fp64 operations) and
 * leaves the removed-slot mask (two words: a slot >= 64 is in the second) and
 * the two slots in LDS; after a barrier the workgroup runs the select body it
 * shares with msckf_map_prune_select.  No atomics, no data-dependent order: a
 * repeat gives the same bits.
 */
#ifndef MSCKF_KEYFRAMES_H
#define MSCKF_KEYFRAMES_H

#include <stdint.h>

#include "msckf_hip.h"
#include "msckf_map.h"

#ifdef __cplusplus
extern "C" {
#endif

int msckf_keyframe_select(msckf_ctx_t* ctx, int nfilt, const int32_t* filters,
                          const double* tracking_rate,          /* [nfilt] */
                          double rot_thr, double trans_thr, double rate_thr,
                          int32_t* cam_slots_out,               /* [nfilt][2], ascending */
                          int32_t* n_inv_out, int64_t* desc_id_out, int32_t* desc_info_out,
                          /* the outstanding batch's results, as msckf_readback; all NULL to skip */
                          uint8_t* accepted_out, double* gamma_out, double* p_w_out,
                          uint8_t* valid_out, int32_t* rows_out);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_KEYFRAMES_H */
