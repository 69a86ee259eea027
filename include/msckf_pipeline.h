/*
 * msckf_pipeline.h -- the two stages of the reference ImageProcessor that
 * msckf_frontend.h leaves to the host, as single device calls on the same
 * mfe_ctx_t (same library, conventions of msckf_frontend.h):
 *
 *   mfe_stereo_match   ImageProcessor.stereo_match (image.py:554-638)
 *   mfe_fast_grid      the masked detection and per-cell sieve of
 *                      add_new_features (image.py:317-360)
 *
 * Each call is one host-to-device copy, device work with no host round trip in
 * between, one device-to-host copy and one synchronisation.  Their scratch is
 * one device block and one pinned host block per context, grown to the
 * largest call seen (shared with mfe_two_point_ransac: every call ends with
 * its synchronisation, so nothing is in flight when a block grows).
 *
 * This text is the specification; tests/frontend_pipeline_ref.py restates it
 * on the CPU oracle's operators (oracle/frontend_oracle.py).
 *
 * ---------------------------------------------------------------------------
 * mfe_stereo_match
 *
 * For each of the n cam0 points pt (pixels, fp64, as mfe_undistort takes them)
 * exactly what ImageProcessor.stereo_match composes from mfe_undistort,
 * mfe_distort, mfe_lk, mfe_lk and two more mfe_undistort calls; one wavefront
 * per point (k_stereo_match_sets).  No fp contraction anywhere.
 *
 *  1. Initial guess, fp64: g = distort_cam1(undistort_cam0(pt, R_guess, new
 *     intrinsics [1 1 0 0])) -- the arithmetic of mfe_undistort followed by
 *     mfe_distort, a rejected fisheye solution's (-1e6, -1e6) included (it is
 *     distorted like any other point).  R_guess (row-major 3x3) is the
 *     rotation the reference passes to undistort_points: R_cam0_cam1 for a
 *     radtan cam0; the identity for an equidistant cam0, whose rectification
 *     the reference never applies (image.py:669-670, kept by the caller).
 *  2. Forward LK (the algorithm of mfe_lk, bit for bit) from slot_cam0 to
 *     slot_cam1, previous point c0 = (float)pt, initial guess (float)g; gives
 *     c1 and the forward status.  cam1_pts[i] = c1 for every point, whatever
 *     the tests below say.
 *  3. Backward LK from slot_cam1 to slot_cam0, previous point c1, initial
 *     guess c0; gives b.  Its status is ignored.
 *  4. Tests, in this order; reason[i] is the number of the first that fails,
 *     0 if none does, and inlier[i] = (reason[i] == 0):
 *       1  forward LK status 0;
 *       2  not (err < 3), err = sqrtf(dx dx + dy dy) in float, (dx, dy) = c0 - b;
 *       3  not (|g.y - c1.y| < 20), in fp64 with the unrounded g.y;
 *       4  c1.x < 0, c1.x > W - 1, c1.y < 0 or c1.y > H - 1;
 *       5  the epipolar test: u0, u1 = the normalised undistorted c0 (cam0's
 *          model) and c1 (cam1's model), i.e. mfe_undistort with R = identity
 *          and new intrinsics [1 1 0 0], (-1e6, -1e6) if rejected;
 *          line = E (u0.x, u0.y, 1)^T, each row as E[3r] u0.x + E[3r+1] u0.y +
 *          E[3r+2] left to right;
 *          error = |u1.x line.x| / sqrt(line.x^2 + line.y^2) -- only the
 *          first component of pt1 * line, the reference's quirk at
 *          image.py:~626, kept;
 *          fails if error > stereo_threshold * 4 / (fx0 + fy0 + fx1 + fy1).
 *          (A NaN error, 0 / 0, does not fail, as in the reference.)
 *     So the forward status of point i is (reason[i] != 1).
 *
 * E (row-major 3x3) is passed directly: the caller forms
 * skew(t_cam0_cam1) R_cam0_cam1 as the reference does, independent of R_guess.
 * For a pure x baseline line.x = 0 and the quirk makes test 5 vacuous.
 *
 * ---------------------------------------------------------------------------
 * mfe_fast_grid
 *
 * Requires an image of at least 16 x 16; 1 <= k <= MFE_GRID_MAX_K; grid_row,
 * grid_col >= 1 with grid_row * grid_col <= MFE_GRID_MAX_CELLS; 1 <= max_kp <=
 * 65536 (the context's keypoint capacity).
 *
 *  Mask    Built on the device in a context buffer (no W x H upload): all
 *          ones, then every occupied point (float xy), with x = (int)px and
 *          y = (int)py, clears rows y-3 .. y+3 and columns x-3 .. x+3, clipped
 *          at the right and bottom edges.  A point with x < 3 or y < 3 clears
 *          nothing: that is what the reference's slice mask[y-3:y+4, x-3:x+4]
 *          does with a negative start (image.py:317-360).  A NaN coordinate
 *          clears nothing.
 *  Detect  FAST 9/16, score, 3x3 non-max suppression and the mask exactly as
 *          mfe_fast (the same k_fast_sets and k_fast_rows_sets), the keypoints in
 *          raster order; the row offsets come from a device scan.  *n_total =
 *          the keypoints that passed, before selection.
 *  Select  A keypoint's cell is (y / gh) grid_col + x / gw (integer division),
 *          gh = ceil(H / grid_row), gw = ceil(W / grid_col).  cell_count[c] =
 *          the keypoints of cell c (their sum is *n_total).  Each cell keeps
 *          its min(k, cell_count[c]) best by response.  The output is grouped
 *          by cell in cell order and packed (cell c starts at the sum of the
 *          kept counts before it); within a cell it is ordered by response
 *          descending, ties in raster order (y, then x).  Fixed-order
 *          reductions, no atomics: the same bits every run.
 *  Error   If *n_total > max_kp the call returns -3 with *n_total set and
 *          cell_count, xy and response untouched: never a truncated selection.
 *
 * The reference's rule sorts a cell only when it holds more than k and leaves
 * it in raster order otherwise (image.py:317-360).  The messages published
 * from either order are the same: the host's _collect_new then sorts every
 * cell again by response with a stable sort, so a cell's final order is
 * response-descending with raster ties either way.
 */
#ifndef MSCKF_PIPELINE_H
#define MSCKF_PIPELINE_H

#include <stdint.h>

#include "msckf_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFE_GRID_MAX_K 16
#define MFE_GRID_MAX_CELLS 1024

/* intrinsics [fx fy cx cy], model MFE_RADTAN / MFE_EQUIDISTANT and 4
 * coefficients per camera; win, max_level, max_iter, eps as mfe_lk.  Outputs:
 * cam1_pts float [n][2], inlier and reason uint8 [n]. */
int mfe_stereo_match(mfe_ctx_t* ctx, int slot_cam0, int slot_cam1, int n, const double* cam0_pts,
                     const double* intrinsics0, int model0, const double* coeffs0, const double* intrinsics1,
                     int model1, const double* coeffs1, const double* R_guess, const double* E, int win,
                     int max_level, int max_iter, double eps, double stereo_threshold, float* cam1_pts,
                     uint8_t* inlier, uint8_t* reason);

/* occupied: float [n_occ][2] (may be NULL when n_occ = 0).  Outputs: xy float
 * [grid_row grid_col k][2] and response float [grid_row grid_col k] (the kept
 * keypoints, packed), cell_count int32 [grid_row grid_col], *n_total. */
int mfe_fast_grid(mfe_ctx_t* ctx, int slot, int threshold, int n_occ, const float* occupied, int grid_row,
                  int grid_col, int k, int max_kp, float* xy_out, float* response_out, int32_t* cell_count,
                  int* n_total);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_PIPELINE_H */
