/*
 * msckf_lanes.h -- the front-end's device calls for many stereo streams
 * (lanes) at once, on the same mfe_ctx_t (same library, conventions of
 * msckf_frontend.h).  Each call is, per set, exactly its single-stream
 * counterpart, bit for bit -- the single call is this call with one set, on
 * the same kernels; this text states only what the set form adds:
 *
 *   mfe_upload_many        mfe_upload          (msckf_frontend.h)
 *   mfe_lk_sets            mfe_lk              (msckf_frontend.h)
 *   mfe_stereo_match_sets  mfe_stereo_match    (msckf_pipeline.h)
 *   mfe_fast_grid_sets     mfe_fast_grid       (msckf_pipeline.h)
 *   mfe_undistort_sets     mfe_undistort       (msckf_frontend.h)
 *
 * (mfe_two_point_ransac of msckf_ransac.h takes sets already.)
 *
 * Conventions
 *
 *  * A set is one lane's work item.  The points of all sets are concatenated;
 *    set s owns the points set_off[s] .. set_off[s + 1] - 1 (set_off int32
 *    [n_sets + 1], set_off[0] = 0, not decreasing), as mfe_two_point_ransac
 *    takes them.  A set may be empty.  The context's max_points bounds the
 *    total, set_off[n_sets]; 0 <= n_sets <= MFE_MAX_SETS.
 *  * Per-set arguments are arrays with one entry (or one row) per set; the
 *    arguments without a set dimension are shared by all sets of the call.
 *  * Every argument of every set is validated before anything is copied or
 *    launched: on any error (a negative return value, mfe_last_error) the
 *    outputs are untouched and, for mfe_upload_many, so are the slots.
 *  * Each call packs its inputs into one block, makes one host-to-device copy
 *    of it, launches its kernels with no host round trip in between, and ends
 *    with one device-to-host copy of all outputs and one synchronisation
 *    (mfe_upload_many has no output and makes no copy back).  The blocks are
 *    the context's scratch blocks of msckf_pipeline.h, grown to the largest
 *    call seen.  A call with n_sets = 0 or without any point returns 0 and
 *    does nothing (mfe_fast_grid_sets detects whatever its occupied lists
 *    hold).
 *  * The kernels take the set from the launch grid where a set's extent is
 *    fixed (an image, a grid cell) and from a per-point set index, which the
 *    call derives from set_off, for point lists.  The slots' pyramid
 *    descriptors and the per-set arguments are read from device tables; the
 *    descriptor table is written once, by mfe_create.
 *
 * mfe_create accepts up to 96 slots (three per lane, 32 lanes).
 *
 * ---------------------------------------------------------------------------
 * mfe_upload_many
 *
 * images: uint8 [n][H][W]; image i goes to slot slots[i], 1 <= n <= the
 * context's slots.  A slot named twice is an error.  The pyramids and Scharr
 * derivatives of all n images are built by one launch per level and kernel,
 * the image index in the grid.  Every slot then holds what mfe_upload of its
 * image leaves there.
 *
 * ---------------------------------------------------------------------------
 * mfe_lk_sets
 *
 * Set s tracks its points from slot_prev[s] to slot_next[s].  next_pts holds
 * the initial guesses on entry and the tracked positions on return, as in
 * mfe_lk; win, max_level, max_iter and eps are shared.  Two sets may name the
 * same slots, in either order.
 *
 * ---------------------------------------------------------------------------
 * mfe_stereo_match_sets
 *
 * Per set: slot_cam0, slot_cam1, both camera models (intrinsics0/1 and
 * coeffs0/1 double [n_sets][4], model0/1 int32 [n_sets]), R_guess and E
 * (double [n_sets][9], row-major) and stereo_threshold (double [n_sets]); the
 * LK parameters are shared.  Outputs cam1_pts, inlier and reason per point as
 * mfe_stereo_match.
 *
 * ---------------------------------------------------------------------------
 * mfe_fast_grid_sets
 *
 * Per set: slots[s] and an occupied list, occ_off int32 [n_sets + 1] into
 * occupied (float [occ_off[n_sets]][2]); threshold, grid_row, grid_col, k and
 * max_kp are shared, with the limits of mfe_fast_grid.  With cells = grid_row
 * grid_col, the outputs of set s are those of mfe_fast_grid at a fixed place:
 *   xy_out       float [n_sets][cells k][2]  the kept keypoints of set s packed
 *   response_out float [n_sets][cells k]     from the start of its row
 *   cell_count   int32 [n_sets][cells]
 *   n_total      int32 [n_sets]
 * (set s keeps sum over its cells of min(k, cell_count) keypoints; the rest of
 * its row is not written).  If any set's n_total exceeds max_kp the call
 * returns -3 with every n_total set and nothing else written.
 *
 * The score map, mask, row counts / offsets and raster keypoint list of
 * mfe_fast_grid exist once per set; mfe_create allocates them for one set and
 * a call with more sets than any before allocates them again.  The
 * stages run as in mfe_fast_grid with the set in the grid, one launch per
 * stage; the same fixed-order reductions, no atomics.  The call makes no
 * read of the totals in between: as in mfe_fast_grid, the raster list and the
 * selection are bounded by max_kp on the device, everything comes back in the
 * one copy, and an overflow is found on the host before any output is
 * written.
 *
 * ---------------------------------------------------------------------------
 * mfe_undistort_sets
 *
 * Per set a camera model (intrinsics, coeffs double [n_sets][4], model int32
 * [n_sets]) with its rectification R (double [n_sets][9]) and new intrinsics
 * (double [n_sets][4]); neither may be NULL.  fp64, one thread per point.
 */
#ifndef MSCKF_LANES_H
#define MSCKF_LANES_H

#include <stdint.h>

#include "msckf_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFE_MAX_SLOTS 96
#define MFE_MAX_SETS 1024

int mfe_upload_many(mfe_ctx_t* ctx, int n, const int32_t* slots, const uint8_t* images);

int mfe_lk_sets(mfe_ctx_t* ctx, int n_sets, const int32_t* set_off, const int32_t* slot_prev,
                const int32_t* slot_next, const float* prev_pts, float* next_pts, uint8_t* status, int win,
                int max_level, int max_iter, double eps);

int mfe_stereo_match_sets(mfe_ctx_t* ctx, int n_sets, const int32_t* set_off, const int32_t* slot_cam0,
                          const int32_t* slot_cam1, const double* cam0_pts, const double* intrinsics0,
                          const int32_t* model0, const double* coeffs0, const double* intrinsics1,
                          const int32_t* model1, const double* coeffs1, const double* R_guess, const double* E,
                          const double* stereo_threshold, int win, int max_level, int max_iter, double eps,
                          float* cam1_pts, uint8_t* inlier, uint8_t* reason);

int mfe_fast_grid_sets(mfe_ctx_t* ctx, int n_sets, const int32_t* slots, const int32_t* occ_off,
                       const float* occupied, int threshold, int grid_row, int grid_col, int k, int max_kp,
                       float* xy_out, float* response_out, int32_t* cell_count, int32_t* n_total);

int mfe_undistort_sets(mfe_ctx_t* ctx, int n_sets, const int32_t* set_off, const double* pts_in, double* pts_out,
                       const double* intrinsics, const int32_t* model, const double* coeffs, const double* R,
                       const double* new_intrinsics);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_LANES_H */
