/*
 * msckf_anchor.h -- anchor fixes: gated EKF updates from stereo observations of
 * points whose world position is known (fiducial corners, surveyed targets, the
 * landmark archive of an earlier run).  The filter's own features are relative
 * by construction -- they are projected onto the left null space of the
 * landmark, and quirk Q3's observability constraint removes global position and
 * yaw on purpose -- so vision gives it no absolute reference.  An anchor does.
 * Same library, conventions of msckf_hip.h; errors through msckf_last_error().
 *
 *   msckf_anchor_batch     the update of the listed filters, each with its own
 *                          anchors, gates included, on the device
 *   msckf_anchor_results   the listed filters' records: applied, used, rows, count
 *   msckf_anchor_status    one filter's per-anchor status and gamma of its last call
 *
 * This text is the specification; tests/anchor_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The measurement
 *
 * Per listed filter, after propagation and before augmentation: n is the live
 * cam count, D = 21 + 6 n (n = 0 is legal), R = to_rotation(q) (world -> IMU), p
 * the record's position, R_ic = R_imu_cam0 and t_ci = t_cam0_imu from the IMU
 * record, R_cc = R_cam0_cam1 and t_cc = t_cam0_cam1 from the context's config.
 *   cam0:  R0 = R_ic R,   t0 = p + R^T t_ci
 *   cam1:  R1 = R_cc R0,  t1 = t0 - R1^T t_cc
 * This is the geometry of the augmentation and of the feature Jacobian.
 *
 * Per anchor l of the filter (its K anchors are anchors[off[k] .. off[k+1]), k
 * the filter's position in the list): p_w, Sigma (3 x 3 symmetric, given as its
 * six upper entries xx xy xz yy yz zz) and z = (u0 v0 u1 v1), the feature
 * message's normalised coordinates.
 *   a = R0 (p_w - t0),  b = R1 (p_w - t1)
 *   zhat = [a_x / a_z, a_y / a_z, b_x / b_z, b_y / b_z],  r = z - zhat
 *   dz0 (4 x 3): rows 0, 1 = [1/a_z 0 -a_x/a_z^2], [0 1/a_z -a_y/a_z^2], rows 2, 3 zero
 *   dz1 (4 x 3): rows 2, 3 the same of b, rows 0, 1 zero
 *   Hx (4 x 6), with respect to the cam0 pose:
 *       Hx[:, 0:3] = dz0 [a]x + dz1 R_cc [a]x
 *       Hx[:, 3:6] = -(dz0 R0 + dz1 R1)
 *   Hf = -Hx[:, 3:6], with respect to p_w
 *   J (6 x 21), the cam0 pose with respect to the IMU error state (order of
 *   msckf_hip.h):
 *       rows 0:3   R_ic at 0:3, I at 15:18
 *       rows 3:6   -R^T [t_ci]x at 0:3, I at 12:15, R^T at 18:21
 *   H_l = Hx J (4 x D), non-zero only in the twelve columns C = 0:3, 12:15, 15:21
 *   N_l = obs_var I_4 + Hf Sigma Hf^T
 * There is NO Q3 projection: the measurement is absolute and must keep position
 * and yaw.  J is the TRUE Jacobian under R_true = (I - [dtheta]x) R and the
 * correction of csrc/msckf_correct.h (R0_true = (I - [R_ic dtheta + dtheta_e]x)
 * R0; t0_true = t0 + dp - R^T [t_ci]x dtheta + R^T dt_ci), the convention of
 * msckf_aid.h's POS row.  It is NOT the augmentation's J, whose [3:6, 0:3] =
 * +[R^T t_ci]x and [3:6, 18:21] = I blocks are quirks of the reference kept for
 * parity there.
 *
 * ---------------------------------------------------------------------------
 * Per-anchor gate
 *
 * In double whatever the context's scalar (the state and P are read as they are
 * stored and widened).  Per anchor, in this order:
 *   status 2 DEPTH    a_z or b_z is not > min_depth; gamma_l is NaN
 *   S_l = H_l P H_l^T + N_l (only P[C, C] enters),  gamma_l = r^T S_l^-1 r
 *   status 3 NOT_PD   the Cholesky factorisation of N_l or of S_l meets a pivot
 *                     <= 0 or a NaN; gamma_l is NaN
 *   status 1 GATED    not gamma_l < chi2
 *   status 0 USED     otherwise
 *
 * Stack and compress
 *
 * Each used anchor is whitened with N_l = C_l C_l^T (C_l lower): Ht_l = C_l^-1
 * H_l, rt_l = C_l^-1 r_l.  The K' used anchors are stacked in list order: 4 K'
 * rows with identity noise.  If 4 K' > 12, with Ht[:, C] = Q R the Householder
 * thin QR of the 4 K' x 12 block: H' = R (12 x 12, in the columns C) and r' = the
 * first twelve entries of Q^T rt.  Otherwise H' = Ht, r' = rt.  m = min(4 K',
 * 12).  This is the compression of the feature update (measurement_update); it
 * keeps the update at rank <= 12 for any number of anchors.
 *
 * Update (msckf_aid.h's)
 *
 * Applied iff K' >= min_anchors and S = H' P H'^T + I_m is positive definite.
 * Applied: dx = P H'^T S^-1 r' goes through the correction of the feature update
 * (csrc/msckf_correct.h; with nulls_alias = 1 the null velocity and position are
 * the corrected velocity and position, quirk Q5, with 0 they stay), and
 *   P+ = P - W W^T,  W = P H'^T L^-T  (S = L L^T),
 * each entry rounded once to the context's scalar; a symmetric P gives a bitwise
 * symmetric P+.
 * Not applied: no byte of the filter's state or P is written.
 * Either way the records are written.  Per filter: applied (0 / 1), used (K'),
 * rows (m; 0 if nothing was stacked) and count, the number of anchor updates
 * ever applied to the slot (it grows by applied).  Per anchor of the call:
 * status (uint8) and gamma.  The records live with the context and start as
 * applied = 0, used = 0, rows = 0, count = 0, with no per-anchor entries.
 *
 * Limitation: Sigma is treated as white noise per frame, but a surveyed error
 * repeats from frame to frame.  With coarse anchors the filter grows
 * overconfident: its covariance shrinks as if every frame brought new
 * information about the anchor's position.  A consistent (Schmidt-style)
 * treatment is not part of this update; declare Sigma generously.
 *
 * ---------------------------------------------------------------------------
 * msckf_anchor_batch
 *
 * Asynchronous; no device-to-host copy.  off is [nfilt + 1], anchors is
 * [off[nfilt]].  -1 before anything is enqueued: a null argument; a filter
 * listed twice or out of range; off[0] != 0, off decreasing, or a filter with
 * more than MSCKF_ANCHOR_MAX anchors; a non-finite p_w, z or cov, or a negative
 * cov diagonal; obs_var not > 0; min_depth not > 0; min_anchors < 1; a NaN chi2.
 * A chi2 <= 0 is legal and uses no anchor.  A listed filter with zero anchors is
 * legal; its record is applied = 0, used = 0, rows = 0.  nfilt == 0 is a no-op
 * (returns 1).  The first call allocates the workspace ([n_filters][Dmax][12]
 * doubles and the records); a context that never calls it allocates nothing.
 *
 * msckf_anchor_results
 *
 * Synchronises.  applied, used, rows int32 [nfilt], count int64 [nfilt]; any may
 * be NULL.  On a context that never called msckf_anchor_batch: the records'
 * initial values.
 *
 * msckf_anchor_status
 *
 * Synchronises.  The per-anchor records of the filter's last call, in list
 * order: *n is their number, status uint8 [cap] and gamma double [cap] take the
 * first min(*n, cap) of them; status, gamma and n may be NULL.  -1: a filter out
 * of range or cap < 0.
 *
 * ---------------------------------------------------------------------------
 * Kernels (csrc/msckf_anchor.hip), stage timer names "anchor_gain" and
 * "anchor_apply"
 *
 *   k_anchor_gain   one 256-thread workgroup per listed filter.  P[C, C] is
 *                   staged in LDS; one wave takes one anchor per lane: geometry,
 *                   H_l, N_l, S_l, the two 4 x 4 Cholesky factorisations,
 *                   gamma_l, the status, the whitened rows.  The used anchors
 *                   are compacted in list order (a ballot and a prefix count).
 *                   The Householder QR of the <= 256 x 12 block runs in LDS, one
 *                   thread per row, twelve reflections, every norm and dot
 *                   product reduced in a fixed order.  Then as k_aid_gain: P
 *                   H'^T from the twelve ROWS C of P (contiguous by symmetry), S,
 *                   its factor L, W into the workspace, dx, the records, the
 *                   state correction.  Reads P, writes none of it.
 *   k_anchor_apply  32 x 32 tiles of the lower triangle x listed filters:
 *                   P_ij <- T(double(P_ij) - sum_k W_ik W_jk), k ascending over
 *                   the record's m, the tile mirrored into the upper triangle
 *                   (csrc/msckf_rank_apply.h); the workgroups of a filter whose
 *                   record says not applied return at once.
 * The gain reads rows of P that the rank-m update rewrites, hence two launches.
 * No atomics and no data-dependent order: a repeat gives the same bits.
 */
#ifndef MSCKF_ANCHOR_H
#define MSCKF_ANCHOR_H

#include <stdint.h>

#include "msckf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_ANCHOR_MAX 64            /* anchors per filter and call */

#define MSCKF_ANCHOR_USED   0
#define MSCKF_ANCHOR_GATED  1
#define MSCKF_ANCHOR_DEPTH  2
#define MSCKF_ANCHOR_NOT_PD 3

typedef struct msckf_anchor_t {
    double p_w[3];        /* the point in the filter's world frame */
    double cov[6];        /* its covariance: xx xy xz yy yz zz */
    double z[4];          /* u0 v0 u1 v1, normalised coordinates */
} msckf_anchor_t;

typedef struct msckf_anchor_params_t {
    double obs_var;       /* variance of a normalised coordinate */
    double chi2;          /* the per-anchor gate on gamma_l (four rows) */
    double min_depth;     /* a_z and b_z must exceed it */
    int32_t min_anchors;  /* the update needs this many used anchors */
} msckf_anchor_params_t;

/* asynchronous, no device-to-host copy */
int msckf_anchor_batch(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const int32_t* off,
                       const msckf_anchor_t* anchors, const msckf_anchor_params_t* prm);
/* synchronises; applied, used, rows int32, count int64 (updates ever applied), any may be NULL */
int msckf_anchor_results(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, int32_t* applied, int32_t* used,
                         int32_t* rows, int64_t* count);
/* synchronises; the filter's last call: status uint8 [cap], gamma double [cap], *n the number of anchors */
int msckf_anchor_status(msckf_ctx_t* ctx, int filter, int cap, uint8_t* status, double* gamma, int32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_ANCHOR_H */
