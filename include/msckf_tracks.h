/*
 * msckf_tracks.h -- the front-end's feature tracks kept on the device: one
 * call runs a whole tracked frame (ImageProcessor.track_features,
 * add_new_features, prune_features and the undistortion of publish) for many
 * lanes, on the same mfe_ctx_t (same library, conventions of msckf_lanes.h).
 *
 *   mfe_tracks_create   the lanes' track tables, in the context
 *   mfe_tracks_put      write a lane's current table (a lane's first frame)
 *   mfe_tracks_get      read it (tests, inspection)
 *   mfe_tracks_step     one tracked frame for each named lane
 *
 * This text is the specification; tests/frontend_tracks_ref.py restates it in
 * numpy around the set calls of msckf_lanes.h.
 *
 * ---------------------------------------------------------------------------
 * The table
 *
 * A lane's table is n rows in order plus the lane's next_id.  A row is
 *   id int64, lifetime int32, cam0 float[2], cam1 float[2]   (pixels).
 * The row order is the order in which ImageProcessor chains curr_features at
 * the end of a frame: cell-major, within a cell the list order.  That is the
 * order publish emits and the order in which the next track_features reads
 * prev_features.
 *
 * mfe_tracks_create allocates two tables per lane, a current and a next one
 * (freed by mfe_destroy); a context holds one set of tables, a second create
 * is an error.  With cells = grid_row grid_col:
 *   cap >= cells (grid_min + grid_max),  cap <= MFE_RANSAC_MAX_SET_POINTS,
 *   1 <= grid_max <= MFE_GRID_MAX_K,  0 <= grid_min,  1 <= cells <=
 *   MFE_GRID_MAX_CELLS,  1 <= n_lanes, 3 n_lanes <= the context's slots.
 * Every lane starts empty with next_id = 0.
 *
 * mfe_tracks_put requires n + cells grid_min <= cap: a step adds at most
 * grid_min rows per cell before it prunes.  A lane's first frame stays on the
 * existing path (mfe_fast without a per-cell cap, mfe_stereo_match, the
 * host's _assign_new) and enters through put.  mfe_tracks_get returns the
 * current table; its arrays hold cap entries.
 *
 * ---------------------------------------------------------------------------
 * mfe_tracks_step
 *
 * n_lanes named lanes (distinct; any subset of the tables' lanes), per lane
 * (arrays with one entry or row per named lane, as in msckf_lanes.h):
 *   slot_prev, slot_c0, slot_c1   the previous cam0 image and the current pair
 *   Hpred       double[9], K R_p_c K^-1 as predict_feature_tracking forms it
 *   the camera models, R_guess, E, stereo_threshold   as mfe_stereo_match_sets
 *   ransac      int32 flag; R0, R1 double[9] (the two R_p_c) and draws uint32
 *               [2][n_hyp][2] per lane (R0, R1, draws may be NULL when no lane
 *               sets the flag; the entries of lanes without it are not read)
 * shared: win, max_level, max_iter, eps (LK), threshold, max_kp (FAST),
 * inlier_error, n_hyp (RANSAC).
 *
 * Per lane, in this order, with no fp contraction anywhere (W x H the image):
 *
 *  1. before_tracking = n.  For each row, with (x, y) the double of cam0:
 *     q_r = Hpred[3r] x + Hpred[3r+1] y + Hpred[3r+2] in fp64, left to right
 *     (r = 0, 1, 2); the guess is ((float)(q_0 / q_2), (float)(q_1 / q_2)).
 *  2. Forward LK from slot_prev to slot_c0, previous point cam0, the guess of
 *     step 1: the algorithm of mfe_lk, bit for bit.  A row is dropped when the
 *     status is 0 or when x < 0, x > W - 1, y < 0 or y > H - 1 (float
 *     comparisons).  after_tracking = the rows left.
 *  3. mfe_stereo_match of the survivors' new cam0 point (the double of the
 *     float) from slot_c0 to slot_c1; rows that are not inliers are dropped.
 *     after_matching = the rows left.
 *  4. With the lane's ransac flag: mfe_two_point_ransac (the unchanged
 *     kernel) of two sets over the matched rows -- cam0 previous -> current
 *     with R0 and cam0's model, cam1 previous -> current with R1 and cam1's
 *     model, points as the doubles of the floats, the lane's draws [0] and
 *     [1].  A row stays only if both sets keep it.  after_ransac = the rows
 *     left (= after_matching without the flag).
 *  5. Survivors keep their id, lifetime += 1.  The cell of a point is
 *     _grid_code of the new cam0: (int)(y / gh) grid_col + (int)(x / gw) with
 *     gh = ceil(H / grid_row), gw = ceil(W / grid_col), the divisions in
 *     float32, truncated.  The host's `int(pt[1] / gh)` has pt[1] an
 *     np.float32 and gh a Python int; under NumPy 2 (verified with 2.2.6) the
 *     quotient is an np.float32, so the host divides in float32 too.
 *  6. The stages of mfe_fast_grid_sets on slot_c0 with the survivors' cam0 as
 *     the occupied list (read on the device) and k = grid_max: the same
 *     kernels, the same per-set work areas.  n_total = the keypoints that
 *     passed, before selection.
 *  7. The candidates come cell-major, within a cell response-descending with
 *     raster ties (msckf_pipeline.h).  mfe_stereo_match of every candidate;
 *     in each cell the new features are the first grid_min inliers in
 *     candidate order, ids from next_id in cell order, then candidate order;
 *     lifetime = 1.  (The host's _assign_new buckets the inliers by
 *     _grid_code -- for a keypoint's integer coordinates the float32 quotient
 *     truncates to the integer quotient of the selection -- and takes the
 *     first grid_min of a stable sort by response, descending.  The
 *     candidates of a cell already arrive in that order, and a stable sort of
 *     a sorted list leaves it as it is: the first grid_min inliers in
 *     candidate order are the same features with the same ids.)
 *  8. A cell is its surviving rows in previous-table order, then its new rows.
 *     A cell of more than grid_max rows keeps the first grid_max of a stable
 *     sort by lifetime, descending (prune_features): row i goes to the
 *     position given by the number of rows with a greater lifetime, or an
 *     equal lifetime and an earlier position.  Ids of pruned new rows stay
 *     consumed.
 *  9. The next table is the cells chained; next_id advances by the new
 *     features of step 7.  Outputs per lane: n, ids, uv double [n][4] =
 *     mfe_undistort of cam0 and of cam1 with R = identity and new intrinsics
 *     [1 1 0 0] (the arguments of ImageProcessor._undistort_args), the
 *     counters [before_tracking, after_tracking, after_matching,
 *     after_ransac], n_total and next_id.
 *
 * Every argument of every lane is validated before anything is copied, the
 * host's record of the lane's n included (n + cells grid_min <= cap).  The call
 * packs its inputs into one block, makes one host-to-device copy, launches
 * with no host round trip in between, and ends with one device-to-host copy
 * and one synchronisation.  The counts live on the device: launches are sized
 * by cap over the fixed-stride layout [lane][cap], and a wavefront or thread
 * beyond its lane's count exits at once.
 *
 * The step reads the current tables and writes only the next ones; after a
 * good return the call makes each named lane's next table its current one.
 * If any lane's n_total exceeds max_kp the call returns -3 with every n_total
 * set and nothing else written, and no table changes.  On any other error the
 * outputs and the tables are untouched.
 *
 * Kernels: LK and the stereo match are thin wrappers of the device functions
 * mfe_lk and mfe_stereo_match are made of, one wavefront per row; the
 * order-preserving compactions are one workgroup per lane (ballot rank within
 * a wave, the wave counts through LDS in wave order); assembly and prune are
 * one workgroup per (lane, cell).  No atomics, fixed-order reductions: a step
 * gives the same bits every run.
 */
#ifndef MSCKF_TRACKS_H
#define MSCKF_TRACKS_H

#include <stdint.h>

#include "msckf_frontend.h"
#include "msckf_lanes.h"
#include "msckf_pipeline.h"
#include "msckf_ransac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFE_TRACKS_COUNTERS 4

int mfe_tracks_create(mfe_ctx_t* ctx, int n_lanes, int cap, int grid_row, int grid_col, int grid_min,
                      int grid_max);

/* ids int64 [n], lifetimes int32 [n], cam0 and cam1 float [n][2] */
int mfe_tracks_put(mfe_ctx_t* ctx, int lane, int n, const int64_t* ids, const int32_t* lifetimes,
                   const float* cam0, const float* cam1, int64_t next_id);

/* outputs sized for cap rows; *n rows are written */
int mfe_tracks_get(mfe_ctx_t* ctx, int lane, int32_t* n, int64_t* ids, int32_t* lifetimes, float* cam0,
                   float* cam1, int64_t* next_id);

/* Outputs: n_out int32 [n_lanes], ids_out int64 [n_lanes][cap], uv_out double
 * [n_lanes][cap][4] (the first n_out rows of each lane), counters int32
 * [n_lanes][MFE_TRACKS_COUNTERS], n_total int32 [n_lanes], next_id_out int64
 * [n_lanes]. */
int mfe_tracks_step(mfe_ctx_t* ctx, int n_lanes, const int32_t* lanes, const int32_t* slot_prev,
                    const int32_t* slot_c0, const int32_t* slot_c1, const double* Hpred, const double* intrinsics0,
                    const int32_t* model0, const double* coeffs0, const double* intrinsics1, const int32_t* model1,
                    const double* coeffs1, const double* R_guess, const double* E, const double* stereo_threshold,
                    const int32_t* ransac, const double* R0, const double* R1, const uint32_t* draws, int win,
                    int max_level, int max_iter, double eps, int threshold, int max_kp, double inlier_error,
                    int n_hyp, int32_t* n_out, int64_t* ids_out, double* uv_out, int32_t* counters,
                    int32_t* n_total, int64_t* next_id_out);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_TRACKS_H */
