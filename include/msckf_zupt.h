/*
 * msckf_zupt.h -- the zero-velocity update (ZUPT): a gated EKF update that tells
 * the filter the platform is standing still.  The reference has none (its
 * check_motion only guards triangulation); a stationary MSCKF drifts, because
 * velocity and the accelerometer bias are weakly observable from the features
 * alone.  Same library, conventions of msckf_hip.h; errors through
 * msckf_last_error().
 *
 *   msckf_zupt_batch     the update of the listed filters, gate included, on the device
 *   msckf_zupt_results   the listed filters' records: applied, gamma, count
 *
 * This text is the specification; tests/zupt_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The measurement
 *
 * Per listed filter: n is the live cam count, D = 21 + 6 n (n = 0 is legal), R =
 * to_rotation(q) (world -> IMU), g the record's gravity, w = gyro_mean[k] and a =
 * acc_mean[k] the caller's mean angular rate and specific force over the interval
 * just propagated (k the filter's position in the list).  The error-state order
 * is msckf_hip.h's.  Three groups of three rows, kept in the order VEL, GYRO, ACC;
 * groups outside prm->rows are dropped, so m = 3, 6 or 9:
 *
 *   group   residual r        H                                         noise
 *   VEL     -v                I at cols 6:9                             vel_noise  I
 *   GYRO    w - b_g           I at cols 3:6                             gyro_noise I
 *   ACC     a - b_a + R g     -[R g]x at cols 0:3, I at cols 9:12       acc_noise  I
 *
 * ACC follows from the filter's own model v' = R^T (a_m - b_a) + g = 0 with
 * R_true = (I - [dtheta]x) R, the convention behind F[6:9, 0:3] = -R^T [acc]x of
 * the process model: a_m = b_a - R_true g, so r = a - (b_a - R g) and
 * d(b_a - R_true g)/d(dtheta) = -[R g]x.
 *
 * ---------------------------------------------------------------------------
 * Gate and update
 *
 * In double whatever the context's scalar (the state and P are read as they are
 * stored and widened):
 *   S = H P H^T + diag(noise),  gamma = r^T S^-1 r.
 * The update is applied iff S is positive definite (its Cholesky factorisation
 * meets no pivot <= 0 and no NaN), gamma < chi2 and |v| <= max_speed.  If S is
 * not positive definite gamma is NaN and applied is 0; that is not an error.
 *
 * Applied: dx = P H^T S^-1 r goes through the correction of the feature update
 * (msckf.py:566-595: quaternions by the small-angle product, the rest added;
 * with nulls_alias = 1 the null velocity and position are the corrected velocity
 * and position, quirk Q5, and their slots of the record are written so; with 0
 * they stay), and
 *   P+ = sym((I - K H) P),  K = P H^T S^-1,
 * measurement_update's formula (msckf.py:597-604) with diag(noise) in place of
 * sigma^2 I.  The device forms W = P H^T L^-T (S = L L^T) and P+ = P - W W^T,
 * each entry rounded once to the context's scalar; a symmetric P gives a bitwise
 * symmetric P+.
 * Not applied: no byte of the filter's state or P is written.
 * Either way the filter's record is written: applied (0 / 1), gamma, and count,
 * the number of updates ever applied to the slot (it grows by applied).  The
 * records live with the context and start as applied = 0, gamma = NaN, count = 0.
 *
 * ---------------------------------------------------------------------------
 * msckf_zupt_batch
 *
 * Asynchronous; no device-to-host copy.  gyro_mean and acc_mean are double
 * [nfilt][3].  -1 before anything is enqueued: a null argument, rows == 0 or a
 * bit outside the three groups, a noise variance that is not > 0 (NaN included,
 * masked groups too), max_speed < 0, a NaN chi2 or max_speed, a filter listed twice
 * or out of range.  A chi2 <= 0 is legal and never applies the update.
 * nfilt == 0 is a no-op (returns 1).  The first call allocates the workspace
 * ([n_filters][Dmax][9] doubles and the records); a context that never calls it
 * allocates nothing.
 *
 * msckf_zupt_results
 *
 * Synchronises.  applied int32 [nfilt], gamma double [nfilt], count int64
 * [nfilt]; any may be NULL.
 *
 * ---------------------------------------------------------------------------
 * Kernels (csrc/msckf_zupt.hip), stage timer names "zupt_gain" and "zupt_apply"
 *
 * H only selects or mixes columns 0:12 of P; by symmetry those are rows 0:12,
 * which are contiguous, so P H^T is read from rows.
 *   k_zupt_gain   one workgroup per listed filter: P H^T (D x m), S, its Cholesky
 *                 factor L, the gate, W = P H^T L^-T into the workspace, dx = W
 *                 L^-1 r, the record, the state correction.  Reads P, writes none
 *                 of it.
 *   k_zupt_apply  32 x 32 tiles of the lower triangle x listed filters:
 *                 P_ij <- T(double(P_ij) - sum_k W_ik W_jk), k ascending, the tile
 *                 mirrored into the upper triangle; the workgroups of a filter
 *                 whose record says not applied return at once.
 * The gain reads rows 0:12 of P and the rank-m update rewrites them, hence two
 * launches.  No atomics and no data-dependent order: a repeat gives the same bits.
 */
#ifndef MSCKF_ZUPT_H
#define MSCKF_ZUPT_H

#include <stdint.h>

#include "msckf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_ZUPT_VEL  1   /* rows 0:3  zero velocity                */
#define MSCKF_ZUPT_GYRO 2   /* rows 3:6  zero angular rate            */
#define MSCKF_ZUPT_ACC  4   /* rows 6:9  zero acceleration (gravity)  */

typedef struct msckf_zupt_params_t {
    double vel_noise, gyro_noise, acc_noise;  /* variances of the three row groups */
    double chi2;                               /* gate on gamma */
    double max_speed;                          /* gate on |v| */
    int32_t rows;                              /* mask of the three groups, != 0 */
} msckf_zupt_params_t;

/* gyro_mean, acc_mean: double [nfilt][3]; asynchronous, no device-to-host copy */
int msckf_zupt_batch(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const double* gyro_mean,
                     const double* acc_mean, const msckf_zupt_params_t* prm);
/* synchronises; applied int32, gamma double, count int64 (updates ever applied), any may be NULL */
int msckf_zupt_results(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                       int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_ZUPT_H */
