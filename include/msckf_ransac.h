/*
 * msckf_ransac.h -- C-ABI of the two-point RANSAC outlier rejection of the GPU
 * stereo front-end (the temporal outlier test of the stereo MSCKF, Sun et al.,
 * msckf_vio; the reference's track_features stubs it, MSCKF/image.py:292-293).
 *
 * One entry point on the front-end context of msckf_frontend.h, with that
 * header's conventions: plain pointers, host arrays copied in and out on the
 * context's stream, one stream synchronisation per call, 0 on success and < 0
 * on error with mfe_last_error().  Everything is fp64.
 *
 * A call serves n_sets independent point sets in ONE launch (one workgroup
 * per set): both cameras of a frame, or every lane's pair of sets of the
 * multi-sequence scheduler.  Set s owns points [set_off[s], set_off[s + 1]) of
 * the concatenated arrays and has its own rotation, camera model and draws.
 *
 * Algorithm per set (n = its point count):
 *   1. unit = 2 / (fx + fy).
 *   2. Both point lists are undistorted to normalised coordinates (the
 *      per-point math of mfe_undistort with identity R and new intrinsics).
 *   3. The previous points are rotation-compensated: (x, y) <- first two
 *      components of R_p_c (x, y, 1), no division by the third.
 *   4. scale = sqrt(2) 2n / sum(|p_prev,i| + |p_curr,i|); every point of both
 *      lists and unit are multiplied by scale.
 *   5. d_i = p_prev,i - p_curr,i.
 *   6. Pre-filter: a point with |d_i| > 50 unit gets marker 0; the others form
 *      the raw list in index order (n_raw of them, mean_dist = mean |d_i|).
 *   7. n_raw < 3: all markers 0, status 2.
 *   8. mean_dist < unit (degenerate motion): the raw points with |d_i| >
 *      inlier_error unit get marker 0, the rest 1; status 1.
 *   9. Otherwise c_i = (d_i.y, -d_i.x, x_prev y_curr - y_prev x_curr), and
 *  10. for hypothesis h = 0 .. n_hyp - 1 with draws (u1, u2): i1 = u1 mod
 *      n_raw, i2 = (i1 + 1 + u2 mod (n_raw - 1)) mod n_raw; a, b = entries i1,
 *      i2 of the raw list; the base k* is the column k with the smallest
 *      |c_a[k]| + |c_b[k]| (lowest index on a tie); the model m has m[k*] = 1
 *      and its other two components solve the 2 x 2 system of rows a, b (a
 *      zero or non-finite determinant skips the hypothesis); its inlier set is
 *      the raw points with |c_i . m| < inlier_error unit, and it qualifies with
 *      at least 0.2 n of them.  The best hypothesis is the qualifying one with
 *      the largest set, the lowest h on a tie.  Its set is refitted (same
 *      base, least squares, 2 x 2 normal equations; a zero or non-finite
 *      determinant leaves m_refit and refit_err NaN): markers 1 on the set, 0
 *      elsewhere, status 0.  No qualifying hypothesis: all markers 0, status 3.
 *
 * info record (MFE_RANSAC_INFO_LEN doubles per set; fields a status leaves
 * undefined are NaN):
 *   [0] status   [1] n_raw   [2] scale   [3] unit after scaling
 *   [4] mean_dist (NaN when n_raw = 0)
 *   [5] best h (-1 where no hypothesis was chosen: statuses 1, 2, 3)
 *   [6] best inlier count (status 1: the markers set; statuses 2, 3: 0)
 *   [7:10] m_refit   [10] refit_err (status 0 only)   [11] 0
 *
 * Determinism: no floating-point atomics and a fixed order in every
 * reduction -- the same call twice gives bit-identical outputs.
 */
#ifndef MSCKF_RANSAC_H
#define MSCKF_RANSAC_H

#include <stdint.h>

#include "msckf_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFE_RANSAC_INFO_LEN 12
#define MFE_RANSAC_MAX_SET_POINTS 4096 /* per set (its c_i live in the workgroup's LDS) */
#define MFE_RANSAC_MAX_HYP 256

/* Errors (< 0, outputs untouched, the context stays usable): null arguments,
 * n_sets < 0, set_off[0] != 0 or set_off not monotone, a set above
 * MFE_RANSAC_MAX_SET_POINTS, a model other than MFE_RADTAN / MFE_EQUIDISTANT,
 * n_hyp outside [1, MFE_RANSAC_MAX_HYP].  n_sets == 0 or zero total points is
 * a successful no-op: nothing is launched and the outputs are left as they
 * are.  The device scratch is owned by the context and grown lazily to the
 * largest call seen (the total number of points is not bounded by
 * mfe_create's max_points). */
int mfe_two_point_ransac(mfe_ctx_t* ctx, int n_sets, const int32_t* set_off /* n_sets+1 */,
        const double* pts_prev, const double* pts_curr,   /* pixels, 2 per point, all sets concatenated */
        const double* R_p_c,        /* n_sets x 9 row-major: previous -> current camera rotation */
        const double* intrinsics,   /* n_sets x 4 */  const int32_t* model /* n_sets */,
        const double* coeffs,       /* n_sets x 4 */
        double inlier_error,        /* pixels (FrontendConfig.ransac_threshold) */
        int n_hyp, const uint32_t* draws,   /* n_sets x n_hyp x 2 */
        uint8_t* inlier_out,        /* one per point */
        double* info_out);          /* n_sets x MFE_RANSAC_INFO_LEN */

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_RANSAC_H */
