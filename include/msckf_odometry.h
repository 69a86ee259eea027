/*
 * msckf_odometry.h -- what an odometry consumer expects beside the pose and the
 * filter computes anyway: the covariance of the published pose and velocity, and
 * the landmarks, i.e. the triangulated positions of the features that leave the
 * map through the lost-feature update, archived on the device (same library,
 * conventions of msckf_hip.h and msckf_map.h; errors through msckf_last_error()).
 *
 *   msckf_landmarks_create    the filters' rings, in the context
 *   msckf_landmarks_clear     empty rings
 *   msckf_landmarks_archive   the accepted features of the lost-form batch just
 *                             updated, appended on the device
 *   msckf_landmarks_get       one filter's rows from a sequence number on
 *   msckf_readback_odom       msckf_readback plus the pose / velocity covariance
 *
 * This text is the specification; tests/landmarks_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The ring
 *
 * Each filter slot has a ring of cap rows in device memory (msckf_landmarks_create;
 * the map tables must exist and map cap <= cap <= 65536, otherwise -1; a context
 * holds one set of rings, a second create is -1; msckf_destroy frees them).  A
 * row is
 *   id      int64
 *   p_w     double[3]
 *   n_obs   int32   the set bits of the feature's mask in the table the load read
 *   gamma   double  the gate's Mahalanobis distance as msckf_batch_results returns it
 *   stamp   int32   the caller's (a frame index)
 * and each slot has a device-resident int64 counter seq, the number of rows ever
 * appended.  Row k of the ring holds the append with seq % cap == k.
 * msckf_landmarks_clear sets seq = 0 of the named filters (asynchronous).
 *
 * ---------------------------------------------------------------------------
 * msckf_landmarks_archive
 *
 * Follows msckf_map_load(MSCKF_MAP_LOAD_LOST, nfilt, filters, feat_off, rows, ..)
 * and msckf_batch_update, with the same nfilt, filters, feat_off and rows, and no
 * other load of a batch (msckf_batch_load, msckf_map_load, msckf_update,
 * msckf_triangulate) and no call that gives up a named filter's lost table
 * (msckf_map.h) in between.  Any other order, form or list is -1 before anything
 * is enqueued, as is a second archive of the same batch.  Asynchronous; no
 * device-to-host copy.
 *
 * For each named filter w the call walks the filter's features of the loaded
 * batch in batch order.  Every feature whose `accepted` (msckf_batch_results) is 1
 * is appended at seq % cap, and seq grows by the number appended.  "accepted"
 * excludes the gate's rejects, the failed triangulations and the features behind
 * the update's row cap.  An appended row takes id and n_obs from the lost-table
 * row the feature was loaded from, p_w and gamma from the batch's device results
 * widened to double exactly as msckf_batch_results widens them, and stamp =
 * stamps[w].
 *
 * Prune-form batches are not archived: their features are still in the map and
 * retire through the lost form later, so every id is appended once.
 *
 * ---------------------------------------------------------------------------
 * msckf_landmarks_get
 *
 * Synchronises.  With seq the filter's counter, lo = min(max(first_seq, seq - cap,
 * 0), seq): returns the rows with sequence numbers lo, lo + 1, .. oldest first,
 * at most max_rows of them (the oldest max_rows if there are more); *seq_out =
 * seq, *first_out = lo.  The return value is the number of rows written (>= 0).
 * lo > first_seq tells a polling consumer that it was lapped.  Output arrays hold
 * max_rows rows; any may be NULL.
 *
 * ---------------------------------------------------------------------------
 * msckf_readback_odom
 *
 * msckf_readback (same arguments, same outputs bit for bit, the same gather
 * launch and the same single synchronisation), and per listed filter, with
 * theta = rows 0:3, v = rows 6:9 and p = rows 12:15 of P and G = blockdiag(R_body,
 * R_body):
 *   pose_cov (6 x 6, row-major) = G [[P_tt, P_tp], [P_pt, P_pp]] G^T
 *   vel_cov  (3 x 3, row-major) = R_body P_vv R_body^T
 * The arithmetic is double whatever the context's scalar.  R_body (row-major) is
 * the rotation of T_imu_body, the matrix the published body velocity is rotated
 * by.  Frame: the orientation block is the covariance of the JPL error angle of
 * the world -> IMU quaternion (the filter's own error state), rotated by R_body;
 * the position block is the world-frame IMU position error rotated by R_body.
 *
 * Kernel (csrc/msckf_map.hip, k_lm_archive): one workgroup of four wavefronts per
 * named filter, the filter's features in passes of 256, order-preserving
 * compaction by 64-bit ballot rank with the wave totals through LDS in wave order
 * and a running base carried from pass to pass; rows written with plain stores,
 * seq once by one thread at the end; no atomics, no data-dependent order: a
 * repeat gives the same bits.
 */
#ifndef MSCKF_ODOMETRY_H
#define MSCKF_ODOMETRY_H

#include <stdint.h>

#include "msckf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_LANDMARKS_MAX_CAP 65536

int msckf_landmarks_create(msckf_ctx_t* ctx, int cap);
int msckf_landmarks_clear(msckf_ctx_t* ctx, int nfilt, const int32_t* filters);

/* feat_off int32 [nfilt + 1], rows int32 [feat_off[nfilt]], stamps int32 [nfilt] */
int msckf_landmarks_archive(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const int32_t* feat_off,
                            const int32_t* rows, const int32_t* stamps);

/* ids int64, p_w double [.][3], n_obs int32, gamma double, stamp int32: max_rows rows each */
int msckf_landmarks_get(msckf_ctx_t* ctx, int filter, int64_t first_seq, int max_rows, int64_t* seq_out,
                        int64_t* first_out, int64_t* ids, double* p_w, int32_t* n_obs, double* gamma, int32_t* stamp);

/* pose_cov_out double [nfilt][36], vel_cov_out double [nfilt][9] */
int msckf_readback_odom(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, double* imu_out, double* cams_out,
                        int32_t* ncams_out, int i0, int n, double* cov_out, uint8_t* accepted_out, double* gamma_out,
                        double* p_w_out, uint8_t* valid_out, int32_t* rows_out, const double* R_body,
                        double* pose_cov_out, double* vel_cov_out);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_ODOMETRY_H */
