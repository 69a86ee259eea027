/*
 * msckf_handoff.h -- the frame's feature message handed from the front-end's
 * track tables (msckf_tracks.h, an mfe_ctx_t) to the filter's feature map
 * (msckf_map.h, an msckf_ctx_t) on the device.  Both contexts live in this one
 * library, so one entry point takes both.
 *
 *   mfe_tracks_msg_put          write a lane's message from the host
 *   mfe_tracks_msg_get          read it (tests, inspection)
 *   mfe_tracks_step_msg         mfe_tracks_step with ids / uv left on the device
 *   msckf_map_add_lost_tracks   msckf_map_add_lost fed from the lanes' messages
 *
 * This text is the specification; tests/vio_ref.py restates the calls around
 * the numpy stand-ins of msckf_tracks.h and msckf_map.h.
 *
 * ---------------------------------------------------------------------------
 * The message table
 *
 * mfe_tracks_create additionally allocates one message per lane, in the block
 * of the track tables (freed by mfe_destroy; never in the call scratch, which
 * other calls regrow):
 *   ids int64 [cap], uv double [cap][4]   on the device, fixed stride
 *                                         [lane][cap], rows in publish order
 *   n, valid                              the host library's record
 * uv is (u0 v0 u1 v1) as mfe_tracks_step's uv_out carries it, which is what
 * msckf_map_add_lost takes as z.  Every lane starts without a valid message.
 *
 * A lane's message describes the lane's CURRENT table.  mfe_tracks_put, and
 * mfe_tracks_step and mfe_tracks_step_msg once their arguments passed
 * validation -- whether the step then succeeds or not -- clear the valid flag
 * of the lanes they name.  Nothing else about mfe_tracks_put and
 * mfe_tracks_step changes.
 *
 * mfe_tracks_msg_put requires 0 <= n <= cap and distinct ids (-1, found on the
 * host before anything is copied; the message is then as it was).  It returns
 * synchronised, with the lane's message valid.  A lane's first frame, which is
 * published on the host path, enters through it.
 *
 * mfe_tracks_msg_get returns the flag and, for a valid message, n and its n
 * rows (arrays sized for cap rows).  Without a valid message *n = 0 and the
 * arrays are not written.
 *
 * ---------------------------------------------------------------------------
 * mfe_tracks_step_msg
 *
 * The arguments of mfe_tracks_step without ids_out and uv_out, steps 1-9 of
 * msckf_tracks.h through the same body: k_trk_assemble and k_trk_uv write the
 * ids and uv of step 9 straight into the named lanes' message tables, and the
 * final device-to-host copy carries only n, the counters, n_total and next_id.
 * After validation the named lanes' messages are invalid; on a good return they
 * are valid with the step's n.  After -3 (n_total > max_kp) or any other error
 * they stay invalid (a -3 step has written a truncated frame into them); the
 * messages of lanes the call does not name are never touched.  The track
 * tables behave exactly as in mfe_tracks_step.
 *
 * ---------------------------------------------------------------------------
 * msckf_map_add_lost_tracks
 *
 * msckf_map_add_lost with filter filters[w]'s message being the message of
 * front-end lane lanes[w], read where it lies.  Checked on the host before
 * anything is copied or launched, each failure -1 (msckf_last_error): the
 * front-end context has track tables; both contexts are on the same device;
 * the lanes are distinct and in range; every named lane's message is valid;
 * and the checks of msckf_map_add_lost.  The host-to-device copy is the header
 * only: per filter, the lane's offset lane * cap into the message tables and
 * the end offset + n -- the host knows n, so there is no device-side count.
 * There is no id sort: the two writers of a message guarantee distinct ids
 * (mfe_tracks_msg_put checks them, a step's ids are a table's).  Everything
 * else is msckf_map_add_lost: the same kernel, step order, -3 on overflow, the
 * lost table, the descriptors, the one copy back and synchronisation, and what
 * a later msckf_map_load accepts.  The messages stay valid after the call.
 *
 * Ordering between the two contexts' streams needs no event:
 *   - every call that writes a message (mfe_tracks_msg_put,
 *     mfe_tracks_step_msg) returns synchronised, so the message is complete
 *     before this call can be made;
 *   - this call returns synchronised, so a later step cannot overwrite a
 *     message that is still being read;
 *   - the caller must not run a front-end call on that mfe_ctx_t concurrently
 *     with this call (as no two calls on one context may run concurrently).
 */
#ifndef MSCKF_HANDOFF_H
#define MSCKF_HANDOFF_H

#include <stdint.h>

#include "msckf_map.h"
#include "msckf_tracks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ids int64 [n], uv double [n][4] */
int mfe_tracks_msg_put(mfe_ctx_t* ctx, int lane, int n, const int64_t* ids, const double* uv);

/* ids, uv sized for cap rows; *valid is 0 or 1 */
int mfe_tracks_msg_get(mfe_ctx_t* ctx, int lane, int32_t* valid, int32_t* n, int64_t* ids, double* uv);

/* Outputs as mfe_tracks_step's, without ids_out and uv_out. */
int mfe_tracks_step_msg(mfe_ctx_t* ctx, int n_lanes, const int32_t* lanes, const int32_t* slot_prev,
                        const int32_t* slot_c0, const int32_t* slot_c1, const double* Hpred,
                        const double* intrinsics0, const int32_t* model0, const double* coeffs0,
                        const double* intrinsics1, const int32_t* model1, const double* coeffs1, const double* R_guess,
                        const double* E, const double* stereo_threshold, const int32_t* ransac, const double* R0,
                        const double* R1, const uint32_t* draws, int win, int max_level, int max_iter, double eps,
                        int threshold, int max_kp, double inlier_error, int n_hyp, int32_t* n_out, int32_t* counters,
                        int32_t* n_total, int64_t* next_id_out);

/* lanes int32 [nfilt]: filter filters[w] takes the message of front-end lane lanes[w]; outputs as
 * msckf_map_add_lost's. */
int msckf_map_add_lost_tracks(msckf_ctx_t* ctx, mfe_ctx_t* fe, int nfilt, const int32_t* filters,
                              const int32_t* lanes, int32_t* tracked_out, int32_t* n_before_out,
                              int32_t* n_cand_out, int64_t* desc_id_out, int32_t* desc_info_out);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_HANDOFF_H */
