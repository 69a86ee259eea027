/*
 * msckf_equalize.h -- histogram equalisation and CLAHE of an image on the
 * device at upload, on the same mfe_ctx_t (same library, conventions of
 * msckf_frontend.h and msckf_lanes.h), and the read-back of a slot.
 *
 * The front-end detects with a fixed FAST threshold on the image as uploaded;
 * on a dark or low-contrast image that finds nothing.  mfe_upload_many_eq is
 * mfe_upload_many with image i equalised by mode[i] between the scatter of the
 * packed block and the pyramids: level 0 of the slot then holds the equalised
 * image, and the pyramid, the Scharr planes, FAST, LK and the stereo match all
 * read that.  mfe_upload / mfe_upload_many are unchanged.
 *
 * cv2 is absent here, so the kernels restate the published OpenCV 4.x
 * algorithms for 8-bit single-channel images (imgproc/histogram.cpp
 * equalizeHist, imgproc/clahe.cpp), the same restatement as
 * tests/equalize_ref.py, against which level 0 is bit-pinned; parity against
 * cv2 itself is unpinned.  All float arithmetic is float32, one rounding per
 * operation in the order written (no contraction); sat(x) rounds half to even
 * and clips to 0..255.
 *
 * MFE_EQ_HIST (cv2.equalizeHist)
 *   h = the 256-bin histogram, i = its first non-empty bin.  If h[i] is the
 *   image's size the image is left as it is.  Otherwise scale = 255.f /
 *   float(size - h[i]), lut[i] = 0 and lut[k] = sat(float(sum of h[j], i < j
 *   <= k) * scale) for k > i; out = lut[in].
 *
 * MFE_EQ_CLAHE (cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply)
 *   1. If W is no multiple of tiles_x or H none of tiles_y, the image is
 *      padded on the right by tiles_x - W % tiles_x and at the bottom by
 *      tiles_y - H % tiles_y columns / rows, BORDER_REFLECT_101 -- for the
 *      histograms only.  tw x th = the padded size / the tile counts, area =
 *      tw th, lut_scale = 255.f / float(area).
 *   2. clip = 0 if clip_limit <= 0, else max(int(clip_limit area / 256), 1)
 *      (in double, from the float32 clip_limit; never above area).
 *   3. Per tile: its histogram; if clip > 0 every bin is cut at clip, excess =
 *      what was cut, every bin gains excess / 256, and with residual = excess
 *      % 256 > 0 and step = max(256 / residual, 1) the bins 0, step, 2 step,
 *      ... gain 1 each while the bin is below 256 and residual ones remain.
 *      lut[tile][k] = sat(float(cumulative sum up to k) * lut_scale).
 *   4. Per pixel (x, y) of value v: txf = x * (1.f / tw) - 0.5f, tx1 =
 *      floor(txf), xa = txf - tx1, xa1 = 1 - xa, then tx2 = min(tx1 + 1,
 *      tiles_x - 1) and tx1 = max(tx1, 0); y likewise;
 *      out = sat((lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 +
 *                (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya).
 *
 * ---------------------------------------------------------------------------
 * mfe_upload_many_eq
 *
 * slots and images as mfe_upload_many.  mode int32 [n], one of MFE_EQ_*;
 * clip_limit float [n], read for MFE_EQ_CLAHE images only (may be NULL if
 * there is none); tiles_x, tiles_y in [1, MFE_EQ_MAX_TILES] are the call's one
 * tile grid, with W >= tiles_x and H >= tiles_y (the reflected pad stays within
 * the image).  An unknown mode, a tile count outside its range or above the
 * image size and a NaN clip_limit are errors (-1), found before anything is
 * copied or launched: the slots are untouched.
 *
 * One host-to-device copy of the packed block (slots, modes, clips, images),
 * then three launches that serve all n images, the image in blockIdx.z and
 * the mode read per image, then the pyramid launches of mfe_upload_many:
 *   k_eq_hist_sets   integer histograms in LDS, one workgroup per CLAHE tile
 *                    (MFE_EQ_HIST: per 1/64 of the image), 16 interleaved
 *                    copies so that the lanes of a wave that meet in one bin
 *                    (a low-contrast image) spread over 16 addresses; stored
 *                    per workgroup, no global atomics
 *   k_eq_lut_sets    one workgroup per tile, one thread per bin: clip and
 *                    redistribute, block scan, the 256-byte table
 *                    (MFE_EQ_HIST: the 64 partial histograms summed first)
 *   k_eq_apply_sets  packed image -> level 0 of the slot; one workgroup per
 *                    interpolation cell (the pixels that share their four
 *                    tiles), the four tables in LDS.  An MFE_EQ_NONE image is
 *                    copied, so it ends bit-identical to mfe_upload_many.
 * The histograms are integer sums: the result does not depend on the order of
 * the adds.  The work areas (histograms and tables per image) belong to the
 * context and grow to the largest call seen.
 *
 * ---------------------------------------------------------------------------
 * mfe_download
 *
 * Synchronises and copies level `level` (0 .. the context's max_level) of a
 * slot, w_l x h_l bytes with w_l = ceil(w_{l-1} / 2), to out.
 *
 * mfe_download_deriv
 *
 * The same for the level's two Scharr planes (calcScharrDeriv of the level's
 * image, what LK reads): w_l x h_l int16 each, to ix and iy.  Same argument
 * checks and errors; a null ix or iy is an error (-1), nothing is written.
 */
#ifndef MSCKF_EQUALIZE_H
#define MSCKF_EQUALIZE_H

#include <stdint.h>

#include "msckf_frontend.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MFE_EQ_NONE 0
#define MFE_EQ_HIST 1
#define MFE_EQ_CLAHE 2
#define MFE_EQ_MAX_TILES 16

/* mfe_upload_many, with image i equalised by mode[i] before its pyramid is built;
 * clip_limit[i] is read for MFE_EQ_CLAHE only; one tile grid per call. */
int mfe_upload_many_eq(mfe_ctx_t* ctx, int n, const int32_t* slots, const uint8_t* images,
                       const int32_t* mode, const float* clip_limit, int tiles_x, int tiles_y);
/* level `level` (0..max_level) of a slot as the device holds it, w_l x h_l bytes */
int mfe_download(mfe_ctx_t* ctx, int slot, int level, uint8_t* out);
/* the Scharr planes of that level as the device holds them, w_l x h_l int16 each */
int mfe_download_deriv(mfe_ctx_t* ctx, int slot, int level, int16_t* ix, int16_t* iy);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_EQUALIZE_H */
