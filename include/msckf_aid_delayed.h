/*
 * msckf_aid_delayed.h -- delayed aiding fixes: the POS and DIR rows of
 * msckf_aid.h for a fix that describes a PAST instant (GNSS, motion capture and
 * UWB pipelines deliver 100-300 ms late).  msckf_aid.h compensates an age Delta
 * by -Delta v, a constant-velocity guess that leaves a Delta^2 / 2 in the residual
 * and ignores the lever arm's rotation.  The window's cam-state clones are the
 * platform's poses at past frame times, correlated with the present IMU state
 * through P: a late fix is a measurement of the pose interpolated between the two
 * clones that bracket its timestamp, and the update on those clones corrects the
 * present state through the cross-covariance.  No re-propagation.  Same library,
 * conventions of msckf_hip.h; errors through msckf_last_error().
 *
 *   msckf_aid_delayed_batch     the update of the listed filters, each with its
 *                               own fix, gate included, on the device
 *   msckf_aid_delayed_results   the listed filters' records
 *
 * This text is the specification; tests/aid_delayed_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The measurement
 *
 * Per listed filter: n is the live cam count, D = 21 + 6 n; fix = fixes[k] (k the
 * filter's position in the list), s = fix.slot a clone slot and lambda =
 * fix.lambda in [0, 1) the fraction of the way from clone s to clone s + 1.
 * (R_s, p_s) and (R_s+1, p_s+1) are the clones' world -> cam0 rotations and cam0
 * positions as stored; R_ic, t_ci the extrinsics of the IMU record (error columns
 * 15:18 and 18:21); l = prm->lever, d_w = prm->dir_w (msckf_aid_params_t; R_body
 * is not used).  A clone carries no velocity, so only two groups of three rows
 * exist, POS then DIR; row 3 group + axis is kept iff that bit of fix.rows is
 * set.  m = popcount(fix.rows), 1 <= m <= 6; z and var of the kept rows are fix.z
 * / fix.var at the row's index 0..5.
 *
 * Interpolation.  Exp, Log, J_l are SO(3)'s: Exp(phi) = I + a [phi]x + b [phi]x^2,
 * J_l(phi) = I + b [phi]x + c [phi]x^2, J_l(phi)^-1 = I - [phi]x / 2 + d [phi]x^2 with
 * theta = |phi|, a = sin theta / theta, b = (1 - cos theta) / theta^2, c = (theta -
 * sin theta) / theta^3, d = 1 / theta^2 - (1 + cos theta) / (2 theta sin theta);
 * J_r(phi) = J_l(phi)^T.
 *   p_c = (1 - lambda) p_s + lambda p_s+1
 *   phi = Log(R_s+1 R_s^T),   R_c = Exp(lambda phi) R_s
 * Log takes M's skew part v = vee(M - M^T) / 2 = sin(theta) axis and phi = v
 * atan2(|v|, (tr M - 1) / 2) / |v|; |phi| < pi is assumed (two clones of a window
 * are a fraction of a second apart).  Below theta = 1e-4 rad (|v| for Log) the
 * series a = 1 - theta^2 / 6, b = 1 / 2 - theta^2 / 24, c = 1 / 6 - theta^2 / 120,
 * d = 1 / 12 + theta^2 / 720 and phi = v (1 + |v|^2 / 6) are used; their truncation
 * error is below theta^4 / 120 = 1e-18 there, and phi = 0 gives Exp = J_l = I exactly,
 * finite.  lambda == 0 uses clone s alone: R_c = R_s, p_c = p_s, clone s + 1 is
 * neither read nor required to exist.
 *
 *   group  measured                      prediction h(x)
 *   POS    antenna position, world       p_c + R_c^T m_c,  m_c = R_ic (l - t_ci)
 *   DIR    d_w seen in the IMU frame     R_ic^T u,         u = R_c d_w
 *
 * (cam0 sits at p + R^T t_ci and R_c = R_ic R, so these are msckf_aid.h's p + R^T l
 * and R d_w of the platform pose at the fix's time.)  Jacobians under R_true = (I -
 * [dtheta]x) R for every rotation (msckf_correct.h) and additive position and
 * translation errors:
 *
 *   POS   I w.r.t. dp_c;  -R_c^T [m_c]x w.r.t. dtheta_c;  +R_c^T [m_c]x at 15:18;
 *         -R_c^T R_ic at 18:21
 *   DIR   +R_ic^T [u]x w.r.t. dtheta_c;  -R_ic^T [u]x at 15:18
 *   dp_c     = (1 - lambda) dp_s + lambda dp_s+1
 *   dtheta_c = [Exp(lambda phi) - lambda J_l(lambda phi) J_r(phi)^-1] dtheta_s
 *              + lambda J_l(lambda phi) J_l(phi)^-1 dtheta_s+1
 *
 * (R_s+1' R_s'^T = Exp(-dtheta_s+1) Exp(phi) Exp(dtheta_s) gives dphi = J_r(phi)^-1
 * dtheta_s - J_l(phi)^-1 dtheta_s+1, and Exp(lambda (phi + dphi)) Exp(-dtheta_s) =
 * Exp(lambda J_l(lambda phi) dphi) Exp(-Exp(lambda phi) dtheta_s) Exp(lambda phi).)
 * It is dtheta_s at lambda = 0 and dtheta_s+1 at lambda = 1, and agrees with central
 * differences through the oracle's apply_correction to 1.5e-10
 * (tests/test_aid_delayed_ref.py).  A clone's error columns are 21 + 6 s : + 3
 * (dtheta) and + 3 : + 6 (dp).  H touches 18 columns at most: 15:21 and the twelve
 * of clones s, s + 1; twelve with lambda == 0.  The rows use the current estimates:
 * no null-space values, no observability edits (as the anchors).
 * r = z - h(x); the noise is diag(var) of the kept rows.
 *
 * ---------------------------------------------------------------------------
 * Gate and update (msckf_aid.h's, word for word)
 *
 * In double whatever the context's scalar:
 *   S = H P H^T + diag(var),  gamma = r^T S^-1 r.
 * Applied iff S is positive definite (its Cholesky factorisation meets no pivot
 * <= 0 and no NaN) and gamma < prm->chi2[m - 1].  If S is not positive definite
 * gamma is NaN and applied is 0; that is not an error.
 * Applied: dx = P H^T S^-1 r goes through the correction of the feature update
 * (csrc/msckf_correct.h, quirk Q5 as in msckf_aid.h), and P+ = P - W W^T with W =
 * P H^T L^-T (S = L L^T), each entry rounded once to the context's scalar; a
 * symmetric P gives a bitwise symmetric P+.
 * Not applied: no byte of the filter's state or P is written.
 *
 * A slot pair that is not inside the filter's LIVE window -- s >= n, or lambda > 0
 * with s + 1 >= n -- is not an error and touches no memory of the state: the record
 * is applied = 0, gamma = NaN, status = BAD_SLOT and nothing else is written.
 *
 * Either way the filter's record is written: applied (0 / 1), gamma, rows (the
 * fix's mask), status (MSCKF_AID_DELAYED_*) and count, the number of delayed
 * fixes ever applied to the slot.  The records live with the context and start
 * as applied = 0, gamma = NaN, rows = 0, status = NONE, count = 0.
 *
 * ---------------------------------------------------------------------------
 * msckf_aid_delayed_batch
 *
 * Asynchronous; no device-to-host copy.  fixes is [nfilt].  -1 before anything
 * is enqueued: a null argument; a filter listed twice or out of range; rows == 0
 * or a bit above 5; a kept row whose var is not > 0 or whose z is NaN; lambda
 * outside [0, 1) or NaN; slot < 0 or slot >= the context's cam capacity; | |dir_w|
 * - 1 | > 1e-6 when any fix keeps a DIR row; a NaN chi2[m - 1] for an m that
 * occurs.  z / var of masked rows are ignored and may be anything.  A chi2 <= 0
 * is legal and never applies the update.  nfilt == 0 is a no-op (returns 1).  The
 * first call allocates the workspace ([n_filters][Dmax][12] doubles, msckf_aid.h's
 * layout, and the records); a context that never calls it allocates nothing.
 *
 * msckf_aid_delayed_results
 *
 * Synchronises.  applied int32 [nfilt], gamma double [nfilt], rows int32 [nfilt],
 * status int32 [nfilt], count int64 [nfilt]; any may be NULL.  On a context that
 * never called msckf_aid_delayed_batch: the records' initial values.
 *
 * ---------------------------------------------------------------------------
 * Kernels (csrc/msckf_aid_delayed.hip), stage timer names "aid_delayed_gain" and
 * "aid_delayed_apply"
 *
 * H only mixes columns 15:21 and 21 + 6 s : 21 + 6 s + 12 (+ 6 with lambda == 0) of
 * P; by symmetry those are rows, which are contiguous, so P H^T is read from rows.
 *   k_aid_delayed_gain   one workgroup per listed filter: the window check, the
 *                        interpolation and the kept rows of H on one lane, P H^T
 *                        (D x m), S, its Cholesky factor, the gate, W = P H^T L^-T
 *                        into the workspace, dx = W L^-1 r, the record, the state
 *                        correction.  Reads P, writes none of it.
 *   k_aid_delayed_apply  32 x 32 tiles of the lower triangle x listed filters, the
 *                        tile body of csrc/msckf_rank_apply.h; the workgroups of a
 *                        filter whose record says not applied return at once.
 * The gain reads rows of P that the rank-m update rewrites, hence two launches.
 * No atomics and no data-dependent order: a repeat gives the same bits.
 */
#ifndef MSCKF_AID_DELAYED_H
#define MSCKF_AID_DELAYED_H

#include <stdint.h>

#include "msckf_aid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_AID_DELAYED_POS 0x07   /* rows 0:3  antenna position, world            */
#define MSCKF_AID_DELAYED_DIR 0x38   /* rows 3:6  a world direction in the IMU frame */

/* the record's status */
#define MSCKF_AID_DELAYED_NONE     (-1)   /* no fix yet */
#define MSCKF_AID_DELAYED_APPLIED  0
#define MSCKF_AID_DELAYED_GATED    1      /* gamma >= chi2[m - 1] */
#define MSCKF_AID_DELAYED_NOT_PD   2      /* S has no Cholesky factor */
#define MSCKF_AID_DELAYED_BAD_SLOT 3      /* the clone pair is not inside the live window */

/* per listed filter: rows 3 group + axis of z / var; the clone slot and the fraction towards slot + 1 */
typedef struct msckf_aid_delayed_fix_t {
    double z[6], var[6], lambda;
    int32_t rows, slot;
} msckf_aid_delayed_fix_t;

/* asynchronous, no device-to-host copy; prm's lever, dir_w and chi2[0:6] are used */
int msckf_aid_delayed_batch(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const msckf_aid_delayed_fix_t* fixes,
                            const msckf_aid_params_t* prm);
/* synchronises; applied int32, gamma double, rows int32, status int32, count int64, any may be NULL */
int msckf_aid_delayed_results(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                              int32_t* rows, int32_t* status, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_AID_DELAYED_H */
