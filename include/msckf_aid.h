/*
 * msckf_aid.h -- aiding fixes: gated EKF updates with an external position, a
 * world or body-frame velocity, or a known world direction (GNSS / motion
 * capture, wheel or Doppler odometry, magnetometer / dual-antenna heading).
 * The reference has none; without vision the filter dead-reckons on the IMU and
 * nothing pulls it back, and its yaw and position are unobservable from vision
 * alone.  Same library, conventions of msckf_hip.h; errors through
 * msckf_last_error().
 *
 *   msckf_aid_batch     the update of the listed filters, each with its own fix,
 *                       gate included, on the device
 *   msckf_aid_results   the listed filters' records: applied, gamma, rows, count
 *
 * This text is the specification; tests/aid_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The measurement
 *
 * Per listed filter: n is the live cam count, D = 21 + 6 n (n = 0 is legal), R =
 * to_rotation(q) (world -> IMU), p and v the record's position and velocity; l =
 * prm->lever, R_body = prm->R_body, d_w = prm->dir_w; fix = fixes[k] (k the
 * filter's position in the list) and Delta = fix.dt >= 0 the age of the fix at
 * the frame time.  The error-state order is msckf_hip.h's.  Four groups of three
 * rows, in the order POS, VEL, BVEL, DIR; row 3 group + axis is kept iff that
 * bit of fix.rows is set, so single axes can be used (a barometer is POS z, a
 * non-holonomic constraint BVEL y, z = 0).  m = popcount(fix.rows), 1 <= m <= 12;
 * z and var of the kept rows are fix.z / fix.var at the row's index 0..11.
 *
 *   group  measured                       prediction h(x)     H (non-zero columns)
 *   POS    antenna position, world        p + R^T l - Delta v -R^T [l]x at 0:3, -Delta I at 6:9, I at 12:15
 *   VEL    IMU velocity, world            v                   I at 6:9
 *   BVEL   velocity, odometer frame       R_body R v          R_body [R v]x at 0:3, R_body R at 6:9
 *   DIR    d_w seen in the IMU frame      R d_w               [R d_w]x at 0:3
 *
 * r = z - h(x); the noise is diag(var) of the kept rows.  The signs follow
 * R_true = (I - [dtheta]x) R, the convention of msckf_zupt.h's ACC rows: R_true^T
 * l = R^T l + R^T [dtheta]x l = R^T l - R^T [l]x dtheta, and R_true u = R u +
 * [R u]x dtheta.  POS predicts the antenna where it was Delta ago with the
 * present velocity held constant.  The lever-arm term of VEL (the antenna's
 * velocity R^T [w]x l) is ignored: VEL is taken as the IMU's velocity.  DIR's
 * three rows have rank 2; that is legal because S stays positive definite
 * through the noise.
 *
 * ---------------------------------------------------------------------------
 * Gate and update (msckf_zupt.h's)
 *
 * In double whatever the context's scalar (the state and P are read as they are
 * stored and widened):
 *   S = H P H^T + diag(var),  gamma = r^T S^-1 r.
 * The update is applied iff S is positive definite (its Cholesky factorisation
 * meets no pivot <= 0 and no NaN) and gamma < prm->chi2[m - 1].  If S is not
 * positive definite gamma is NaN and applied is 0; that is not an error.
 *
 * Applied: dx = P H^T S^-1 r goes through the correction of the feature update
 * (csrc/msckf_correct.h; with nulls_alias = 1 the null velocity and position are
 * the corrected velocity and position, quirk Q5, with 0 they stay), and
 *   P+ = sym((I - K H) P),  K = P H^T S^-1.
 * The device forms W = P H^T L^-T (S = L L^T) and P+ = P - W W^T, each entry
 * rounded once to the context's scalar; a symmetric P gives a bitwise symmetric
 * P+.
 * Not applied: no byte of the filter's state or P is written.
 * Either way the filter's record is written: applied (0 / 1), gamma, rows (the
 * fix's mask) and count, the number of fixes ever applied to the slot (it grows
 * by applied).  The records live with the context and start as applied = 0,
 * gamma = NaN, rows = 0, count = 0.
 *
 * ---------------------------------------------------------------------------
 * msckf_aid_batch
 *
 * Asynchronous; no device-to-host copy.  fixes is [nfilt].  -1 before anything
 * is enqueued: a null argument; a filter listed twice or out of range; rows == 0
 * or a bit above 11; a kept row whose var is not > 0 or whose z is NaN; dt
 * negative or NaN; R_body not orthonormal to 1e-6 (max |R_body R_body^T - I|) when
 * any fix keeps a BVEL row; | |dir_w| - 1 | > 1e-6 when any fix keeps a DIR row; a
 * NaN chi2[m - 1] for an m that occurs.  z / var of masked rows are ignored and
 * may be anything.  A chi2 <= 0 is legal and never applies the update.
 * nfilt == 0 is a no-op (returns 1).  The first call allocates the workspace
 * ([n_filters][Dmax][12] doubles and the records); a context that never calls it
 * allocates nothing.
 *
 * msckf_aid_results
 *
 * Synchronises.  applied int32 [nfilt], gamma double [nfilt], rows int32
 * [nfilt], count int64 [nfilt]; any may be NULL.  On a context that never called
 * msckf_aid_batch: the records' initial values.
 *
 * ---------------------------------------------------------------------------
 * Kernels (csrc/msckf_aid.hip), stage timer names "aid_gain" and "aid_apply"
 *
 * H only selects or mixes columns 0:3, 6:9 and 12:15 of P; by symmetry those are
 * rows, which are contiguous, so P H^T is read from rows.
 *   k_aid_gain   one workgroup per listed filter: the kept rows of H, r and the
 *                noise from the filter's own fix (m differs per filter within a
 *                launch), P H^T (D x m), S, its Cholesky factor L, the gate, W = P
 *                H^T L^-T into the workspace, dx = W L^-1 r, the record, the state
 *                correction.  Reads P, writes none of it.
 *   k_aid_apply  32 x 32 tiles of the lower triangle x listed filters:
 *                P_ij <- T(double(P_ij) - sum_k W_ik W_jk), k ascending over the
 *                record's m, the tile mirrored into the upper triangle; the
 *                workgroups of a filter whose record says not applied return at
 *                once.  The tile body is msckf_zupt.h's k_zupt_apply's
 *                (csrc/msckf_rank_apply.h).
 * The gain reads rows of P that the rank-m update rewrites, hence two launches.
 * No atomics and no data-dependent order: a repeat gives the same bits.
 */
#ifndef MSCKF_AID_H
#define MSCKF_AID_H

#include <stdint.h>

#include "msckf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_AID_POS  0x007   /* rows 0:3   antenna position, world            */
#define MSCKF_AID_VEL  0x038   /* rows 3:6   IMU velocity, world                */
#define MSCKF_AID_BVEL 0x1c0   /* rows 6:9   velocity in the odometer frame     */
#define MSCKF_AID_DIR  0xe00   /* rows 9:12  a world direction in the IMU frame */

typedef struct msckf_aid_params_t {
    double lever[3];      /* antenna in the IMU frame */
    double R_body[9];     /* IMU -> odometer frame, row-major */
    double dir_w[3];      /* the reference direction in the filter's world frame, unit length */
    double chi2[12];      /* gate by number of kept rows m (index m-1) */
} msckf_aid_params_t;

/* per listed filter: rows 3 group + axis of z / var; dt the fix's age at the frame time */
typedef struct msckf_aid_fix_t {
    double z[12], var[12], dt;
    int32_t rows;
} msckf_aid_fix_t;

/* asynchronous, no device-to-host copy */
int msckf_aid_batch(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const msckf_aid_fix_t* fixes,
                    const msckf_aid_params_t* prm);
/* synchronises; applied int32, gamma double, rows int32, count int64 (fixes ever applied), any may be NULL */
int msckf_aid_results(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                      int32_t* rows, int64_t* count);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_AID_H */
