/*
 * msckf_standstill.h -- the vision standstill cue: the frame-to-frame pixel
 * motion of the front-end's tracks (msckf_tracks.h, an mfe_ctx_t) gates the
 * zero-velocity update of the filter (msckf_zupt.h, an msckf_ctx_t).  The ZUPT
 * of msckf_zupt.h decides "standing still" from the filter's own numbers only
 * (gamma and |v|); the cue is a judge outside the state.  Same library,
 * conventions of msckf_lanes.h and msckf_hip.h; errors through mfe_last_error()
 * and msckf_last_error().
 *
 *   mfe_motion_sets            the statistic of caller-supplied point pairs
 *   mfe_tracks_motion_enable   the statistic inside the tracked frame, per lane
 *   mfe_tracks_motion_get      read a lane's record
 *   msckf_zupt_batch_cued      msckf_zupt_batch with the cue in the decision
 *   msckf_zupt_cue_results     the records, with the cue as the gain kernel saw it
 *
 * This text is the specification; tests/standstill_ref.py restates it in numpy
 * around tests/zupt_ref.py.
 *
 * ---------------------------------------------------------------------------
 * The motion statistic
 *
 * Of n point pairs (prev_i, curr_i), float32 pixels, with q in [0, 1]:
 *   dx = curr.x - prev.x,  dy = curr.y - prev.y,  d2 = dx dx + dy dy
 * in float32 with no fp contraction: each product and the sum are rounded once.
 *   k = floor(q (n - 1))   in double
 * and the statistic is the k-th smallest d2, 0-based: np.sort(d2)[k] on the same
 * float32 inputs, bit for bit.  q = 0.5 is the lower median.  For n = 0 the
 * value is NaN and the record's n = 0 tells the consumer so.  The statistic is
 * a SQUARED distance in pixels^2; nothing takes a root.
 *
 * mfe_motion_sets is the set call: n_sets sets of pairs, set i the rows
 * set_off[i] .. set_off[i + 1] of prev and curr (float [..][2]); n_out[i] is the
 * set's size and d2_out[i] its statistic.  -1 before anything is copied, the
 * outputs untouched: a null argument, q outside [0, 1] or NaN, set_off not
 * starting at 0 or not monotone, more points than the context's max_points, a
 * set above MFE_RANSAC_MAX_SET_POINTS, a coordinate that is not finite.  Empty
 * sets are legal; n_sets == 0 is a no-op.  One host-to-device copy, one launch,
 * one copy back, one synchronisation.
 *
 * ---------------------------------------------------------------------------
 * The statistic inside the tracked frame
 *
 * mfe_tracks_motion_enable(ctx, on, q) requires track tables (-1 without; -1 for
 * q outside [0, 1] or NaN, the switch then stays as it was).  With the switch on,
 * the one tracking body behind mfe_tracks_step and mfe_tracks_step_msg launches
 * the statistic's kernel once behind the compaction of step 4 (msckf_tracks.h),
 * over the rows that survived it (n = after_ransac): prev = the row's cam0 in
 * the current table, curr = its tracked cam0 point (c0 of step 2).  The kernel
 * writes the lane's record {int32 n, float d2} into the block of the track
 * tables, next to the message tables, [lane]: it never moves, so another
 * context's kernel may read it where it lies.
 *
 * A lane's record is valid exactly when a step that ran with the switch on has
 * succeeded for it: mfe_tracks_put, and mfe_tracks_step / mfe_tracks_step_msg
 * once their arguments passed validation, clear the valid flag of the lanes
 * they name; a good return of a step with the switch on sets it.  After -3, any
 * other error, or a step with the switch off the record stays invalid.  The flag
 * is the host library's record, as the message's is (msckf_handoff.h).
 *
 * With the switch off, which is how a context starts, the launches, the copies
 * and every output of every call are what they were without this header, bit
 * for bit.  With it on, every other output of the step is unchanged: the kernel
 * reads the tables and the work areas and writes only the record.
 *
 * mfe_tracks_motion_get(ctx, lane, valid, n, d2) synchronises.  Without a valid
 * record *valid = 0, *n = 0, *d2 = NaN and nothing is copied.
 *
 * The kernel (csrc/msckf_frontend.hip, k_motion_sets / k_trk_motion around one
 * device function): one workgroup of 256 threads per set or lane; a set of no
 * rows writes NaN and the whole workgroup returns; a wave whose first row lies
 * beyond the count returns at once.  The d2 values (at most 4096, 16 KB) live in
 * LDS as their uint32 bit patterns: d2 is never negative and never -0, and
 * non-negative floats order as their bits.  The selection is an exact radix
 * select, most significant bit first, one bit per pass: the number of remaining
 * candidates whose bit is 0 is counted from wave ballots (popcount, summed per
 * wave in a register, the wave sums through LDS in wave order); k below that
 * count keeps the zeros, else k drops by it and the ones stay.  After 32 passes
 * the prefix is the k-th smallest pattern.  Integer counts, no atomics, no
 * data-dependent order: a repeat gives the same bits.
 *
 * ---------------------------------------------------------------------------
 * The cued update
 *
 * msckf_zupt_batch_cued is msckf_zupt_batch -- the same rows, S, gamma, W,
 * correction and k_zupt_apply, asynchronous, no copy back -- with one more
 * input per listed filter, the cue {n, d2}, and another decision rule.
 *
 * The cue's source:
 *   fe != NULL   filter filters[w] reads the motion record of front-end lane
 *                lanes[w] where it lies.  Host checks (-1): fe has track tables;
 *                both contexts are on the same device; lanes is not null, its
 *                entries are in range and distinct.  Nothing is copied but the
 *                header: per filter the lane, or -1 where the lane's record is
 *                not valid.  An invalid record is no error, it is UNKNOWN.
 *                cue_n and cue_d2 are not read.
 *   fe == NULL   cue_n int32 [nfilt] and cue_d2 float [nfilt] travel in the
 *                call's one input block; n < 0 means "no record".  lanes is not
 *                read.
 *
 * Cue status per filter, decided in the gain kernel:
 *   UNKNOWN (2)  no valid record, or n < min_tracks
 *   STILL   (1)  else, (double)d2 <= max_px max_px
 *   MOVING  (0)  else (a NaN d2 with n >= min_tracks is MOVING)
 * With imu_ok = S positive definite && gamma < chi2 && |v| <= max_speed
 * (msckf_zupt.h's rule) and pd = S positive definite:
 *   mode VETO     applied = imu_ok && (STILL || (UNKNOWN && unknown == IMU))
 *   mode EITHER   applied = (pd && STILL) ||
 *                           (imu_ok && (status != UNKNOWN || unknown == IMU))
 * unknown is IMU or REJECT: with IMU a frame without enough tracks falls back
 * to msckf_zupt.h's gate, so that losing vision does not switch the update off;
 * with REJECT it applies nothing.  VETO lets vision forbid what the state
 * believes in; EITHER also lets vision assert a standstill the state denies
 * (a velocity estimate that drifted above max_speed can then re-engage).
 *
 * Records: msckf_zupt.h's three (applied, gamma, count), written as there, plus
 * per slot cue int32 (the status), cue_n int32 and cue_d2 float as the kernel
 * saw them (-1 and NaN where there was no valid record).  They start as -1, -1
 * and NaN, are allocated with the ZUPT workspace and are written by the cued
 * call only.  msckf_zupt_cue_results reads all six in one device-to-host read (the
 * three of msckf_zupt_results and the cue's) and synchronises; any output may be
 * NULL.
 *
 * -1 before anything is enqueued: the checks of msckf_zupt_batch; a null cue;
 * max_px negative or NaN; min_tracks < 1; a mode or policy outside the two
 * constants each; the source's checks above; fe == NULL with a null cue array.
 * nfilt == 0 is a no-op (returns 1).  msckf_zupt_batch itself is unchanged: the
 * same launches, the same bits, and it leaves the cue records alone.
 *
 * ---------------------------------------------------------------------------
 * Ordering between the two contexts' streams (no event)
 *
 *   - every call that writes or invalidates a record (the steps, mfe_tracks_put)
 *     returns synchronised, so the record is complete before the cued call can
 *     be made;
 *   - the cued call is asynchronous and reads the record in place.  A front-end
 *     step or put that names the lane must therefore not be issued before a
 *     synchronising call on the filter context (msckf_zupt_results,
 *     msckf_zupt_cue_results, msckf_readback, msckf_map_add_lost_tracks, ...)
 *     has returned;
 *   - no front-end call on that mfe_ctx_t runs concurrently with the cued call.
 * In MultiStereoVIO.stereo_callbacks the rule holds by construction: the
 * frame's feature_callbacks serves "zupt" (order 1.5) before the synchronising
 * "map_add_lost_tracks" (2.5) and "states" (5) of the same frame and returns
 * only when every lane's generator has ended, before the next frame's step.
 */
#ifndef MSCKF_STANDSTILL_H
#define MSCKF_STANDSTILL_H

#include <stdint.h>

#include "msckf_tracks.h"
#include "msckf_zupt.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_CUE_MOVING  0
#define MSCKF_CUE_STILL   1
#define MSCKF_CUE_UNKNOWN 2

#define MSCKF_CUE_MODE_VETO   0
#define MSCKF_CUE_MODE_EITHER 1

#define MSCKF_CUE_UNKNOWN_IMU    0   /* fall back to msckf_zupt.h's gate */
#define MSCKF_CUE_UNKNOWN_REJECT 1   /* apply nothing */

typedef struct msckf_zupt_cue_t {
    double max_px;       /* STILL iff d2 <= max_px^2 (pixels) */
    int32_t min_tracks;  /* UNKNOWN below this many pairs, >= 1 */
    int32_t mode;        /* MSCKF_CUE_MODE_* */
    int32_t unknown;     /* MSCKF_CUE_UNKNOWN_* */
} msckf_zupt_cue_t;

/* prev, curr: float [set_off[n_sets]][2]; n_out int32 [n_sets], d2_out float [n_sets] */
int mfe_motion_sets(mfe_ctx_t* ctx, int n_sets, const int32_t* set_off, const float* prev, const float* curr,
                    double q, int32_t* n_out, float* d2_out);

int mfe_tracks_motion_enable(mfe_ctx_t* ctx, int on, double q);

/* synchronises; *valid is 0 or 1 */
int mfe_tracks_motion_get(mfe_ctx_t* ctx, int lane, int32_t* valid, int32_t* n, float* d2);

/* fe != NULL: lanes int32 [nfilt]; fe == NULL: cue_n int32 [nfilt], cue_d2 float [nfilt].
 * gyro_mean, acc_mean: double [nfilt][3]; asynchronous, no device-to-host copy */
int msckf_zupt_batch_cued(msckf_ctx_t* ctx, mfe_ctx_t* fe, int nfilt, const int32_t* filters, const int32_t* lanes,
                          const int32_t* cue_n, const float* cue_d2, const double* gyro_mean, const double* acc_mean,
                          const msckf_zupt_params_t* prm, const msckf_zupt_cue_t* cue);

/* synchronises; applied, gamma, count as msckf_zupt_results'; cue int32, cue_n int32, cue_d2 float; any may be NULL */
int msckf_zupt_cue_results(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                           int64_t* count, int32_t* cue, int32_t* cue_n, float* cue_d2);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_STANDSTILL_H */
