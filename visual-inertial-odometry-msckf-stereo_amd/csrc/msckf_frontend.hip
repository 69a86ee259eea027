// msckf_frontend.hip -- the stereo front-end's image operators on gfx950
// (MSCKF/image.py:95-702); C-ABI in
// include/msckf_frontend.h.
//
// The reference does this work through OpenCV (FastFeatureDetector,
// calcOpticalFlowPyrLK, undistortPoints / projectPoints / fisheye).  cv2 is
// absent from this image and from the GPU box, so the kernels restate the
// published OpenCV 4.x algorithms -- the same restatement as
// oracle/frontend_oracle.py (test infrastructure), which the GPU tests check
// them against:
//   k_eq_*_sets      histogram equalisation / CLAHE of level 0 at upload (equalizeHist,
//               clahe.cpp; include/msckf_equalize.h): LDS histograms per tile, the
//               tiles' tables, the bilinear blend of four tables per pixel
//   k_pyrdown_sets   Gaussian pyramid level (pyrDown, 5x5 [1 4 6 4 1]^2, REFLECT_101)
//   k_scharr_sets    Scharr derivatives of a level (calcScharrDeriv)
//   k_fast_sets      FAST 9/16 segment test + corner score (fast.cpp, fast_score.cpp)
//   k_fast_rows_sets 3x3 non-max suppression + mask, raster-order compaction: one
//               wave per image row, ballot / popcount, two passes around the
//               prefix sum of the row counts, k_row_scan_sets (deterministic order)
//   k_lk_sets   pyramidal Lucas-Kanade (LKTrackerInvoker), one wavefront per
//               point: the 15 x 15 window over the 64 lanes, 14-bit fixed-point
//               bilinear weights, window sums of the integer products reduced
//               exactly (int64) across the wave
//   k_undistort_sets / k_distort   radtan and equidistant camera models, fp64
//   k_two_point_ransac   temporal outlier rejection (include/msckf_ransac.h): one
//               workgroup per point set, one wave per hypothesis
//   k_stereo_match_sets   ImageProcessor.stereo_match in one launch
//               (include/msckf_pipeline.h): one wavefront per point, the camera
//               models and both LK runs from the functions k_undistort_sets,
//               k_distort and k_lk_sets are made of
//   k_mask_clear_sets / k_row_scan_sets / k_grid_select_sets   masked detection
//               with the per-cell selection (include/msckf_pipeline.h) around
//               k_fast_sets and k_fast_rows_sets: device-built mask, device scan
//               of the row counts, one workgroup per grid cell
// Each of these takes a list of sets (include/msckf_lanes.h); a single-image call
// is the list of one.
//   k_trk_*     the feature tracks kept on the device (include/msckf_tracks.h): a
//               whole tracked frame of many streams chained on the device, around
//               lk_point, stereo_point, k_two_point_ransac and the detection stages;
//               k_trk_assemble and k_trk_uv write the published ids / uv into the
//               call's block or into the lanes' message tables (include/msckf_handoff.h)
//   k_motion_sets / k_trk_motion   the motion statistic of include/msckf_standstill.h:
//               a quantile of the squared pixel displacement of point pairs, one
//               workgroup per set or lane, an exact radix select over LDS
// Images are 8-bit, small (752 x 480 for EuRoC) and read through the cache:
// these kernels are latency-class work, not HBM-bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/msckf_frontend.h"
#include "../../include/msckf_lanes.h"
#include "../../include/msckf_pipeline.h"
#include "../../include/msckf_ransac.h"
#include "../../include/msckf_handoff.h"
#include "../../include/msckf_tracks.h"
#include "../../include/msckf_equalize.h"
#include "../../include/msckf_standstill.h"
#include "msckf_handoff_dev.h"
#include "msckf_standstill_dev.h"

namespace {

thread_local char g_err[512] = "";
void set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
#define MFE_FAIL(rc, ...)      \
    do {                       \
        set_err(__VA_ARGS__);  \
        return rc;             \
    } while (0)
#define MFE_HIP(x)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) MFE_FAIL(-2, "HIP error %s at %s", hipGetErrorString(e_), #x); \
    } while (0)

constexpr int MAXL = 8;        // pyramid levels (level 0 .. MAXL - 1)
constexpr int W_BITS = 14;     // lkpyramid.cpp interpolation weights
constexpr float FLT_SCALE = 1.0f / (1 << 20);

struct Level {
    int w, h;
    uint8_t* img;
    int16_t* ix;
    int16_t* iy;
};
struct Pyr {
    Level lv[MAXL];
};

__device__ __forceinline__ int refl101(int i, int n) {   // BORDER_REFLECT_101
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// ---------------------------------------------------------------- pyramid --
// Every operator has one kernel, the set form of msckf_lanes.h (k_*_sets), around a
// __device__ body: it takes the set index from the grid or from a per-point index
// and reads the slots' Pyr descriptors and the per-set arguments from device tables.
// The single-image calls of msckf_frontend.h / msckf_pipeline.h run it with one set.
__device__ __forceinline__ void pyrdown_px(const uint8_t* __restrict__ src, int sw, int sh,
                                           uint8_t* __restrict__ dst, int dw, int dh, int x, int y) {
    if (x >= dw || y >= dh) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int cols[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) cols[j] = refl101(2 * x - 2 + j, sw);
    int s = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const uint8_t* row = src + (size_t)refl101(2 * y - 2 + i, sh) * sw;
        int hsum = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) hsum += k[j] * row[cols[j]];
        s += k[i] * hsum;
    }
    dst[(size_t)y * dw + x] = (uint8_t)((s + 128) >> 8);
}

// blockIdx.z = the image of the call; its slot's level - 1 -> level
__global__ void __launch_bounds__(256) k_pyrdown_sets(const Pyr* __restrict__ tab, const int32_t* __restrict__ slots,
                                                      int level) {
    const Pyr& P = tab[slots[blockIdx.z]];
    const Level U = P.lv[level - 1], L = P.lv[level];
    pyrdown_px(U.img, U.w, U.h, L.img, L.w, L.h, blockIdx.x * 16 + (threadIdx.x & 15),
               blockIdx.y * 16 + (threadIdx.x >> 4));
}

__device__ __forceinline__ void scharr_px(const uint8_t* __restrict__ img, int w, int h, int16_t* __restrict__ ix,
                                          int16_t* __restrict__ iy, int x, int y) {
    if (x >= w || y >= h) return;
    const int xm = refl101(x - 1, w), xp = refl101(x + 1, w);
    const uint8_t* rm = img + (size_t)refl101(y - 1, h) * w;
    const uint8_t* r0 = img + (size_t)y * w;
    const uint8_t* rp = img + (size_t)refl101(y + 1, h) * w;
    const int gx = 3 * (rm[xp] + rp[xp]) + 10 * r0[xp] - (3 * (rm[xm] + rp[xm]) + 10 * r0[xm]);
    const int gy = 3 * (rp[xm] + rp[xp]) + 10 * rp[x] - (3 * (rm[xm] + rm[xp]) + 10 * rm[x]);
    ix[(size_t)y * w + x] = (int16_t)gx;
    iy[(size_t)y * w + x] = (int16_t)gy;
}

__global__ void __launch_bounds__(256) k_scharr_sets(const Pyr* __restrict__ tab, const int32_t* __restrict__ slots,
                                                     int level) {
    const Level L = tab[slots[blockIdx.z]].lv[level];
    scharr_px(L.img, L.w, L.h, L.ix, L.iy, blockIdx.x * 16 + (threadIdx.x & 15), blockIdx.y * 16 + (threadIdx.x >> 4));
}

// mfe_upload_many: image blockIdx.z of the packed block -> level 0 of its slot;
// 16 bytes per thread where the image size allows it, single bytes otherwise
__global__ void __launch_bounds__(256) k_image_scatter_sets(const Pyr* __restrict__ tab,
                                                            const int32_t* __restrict__ slots,
                                                            const uint8_t* __restrict__ images, size_t bytes, int vec) {
    const uint8_t* src = images + (size_t)blockIdx.z * bytes;
    uint8_t* dst = tab[slots[blockIdx.z]].lv[0].img;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        if (16 * t < bytes) ((uint4*)dst)[t] = ((const uint4*)src)[t];
    } else if (t < bytes) {
        dst[t] = src[t];
    }
}

// ----------------------------------------------------------- equalisation --
// include/msckf_equalize.h: mfe_upload_many_eq's three launches between the packed block and
// the pyramids.  blockIdx.z = the image of the call; its mode is read per image.
constexpr int EQ_HCH = 64;      // MFE_EQ_HIST: partial histograms per image
constexpr int EQ_COPIES = 16;   // interleaved copies of a workgroup's histogram in LDS

struct EqArgs {
    const Pyr* tab;
    const int32_t* slots;
    const int32_t* mode;     // [n]
    const int32_t* clip;     // [n], bin limit of a CLAHE image (0: none)
    const uint8_t* images;   // the packed block's [n][H][W]
    unsigned* hist;          // [n][units][256]
    uint8_t* lut;            // [n][tiles][256]
    int W, H, tiles_x, tiles_y, tw, th;
    int units;               // max(tiles, EQ_HCH)
};

// One workgroup per histogram: tile blockIdx.x of a CLAHE image (over the padded image,
// REFLECT_101), or the blockIdx.x-th of EQ_HCH equal runs of a HIST image's pixels.  Lane l adds
// into copy l % 16 of the bin, the copies of a bin in consecutive words: the lanes of a wave that
// meet in one bin (a low-contrast image) spread over 16 addresses and banks.  Integer adds: the
// order does not matter.
__global__ void __launch_bounds__(256) k_eq_hist_sets(EqArgs a) {
    const int img = blockIdx.z, u = blockIdx.x, mode = a.mode[img];
    if (mode == MFE_EQ_NONE || u >= (mode == MFE_EQ_HIST ? EQ_HCH : a.tiles_x * a.tiles_y)) return;
    __shared__ unsigned h[256 * EQ_COPIES];
    for (int i = threadIdx.x; i < 256 * EQ_COPIES; i += 256) h[i] = 0;
    __syncthreads();
    const uint8_t* src = a.images + (size_t)img * a.W * a.H;
    const int c = threadIdx.x & (EQ_COPIES - 1);
    if (mode == MFE_EQ_HIST) {
        const size_t px = (size_t)a.W * a.H;
        const size_t lo = px * u / EQ_HCH, hi = px * (u + 1) / EQ_HCH;
        for (size_t i = lo + threadIdx.x; i < hi; i += 256) atomicAdd(&h[src[i] * EQ_COPIES + c], 1u);
    } else {
        const int x0 = (u % a.tiles_x) * a.tw, y0 = (u / a.tiles_x) * a.th;
        const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
        for (int j = ly; j < a.th; j += 8) {
            const uint8_t* row = src + (size_t)refl101(y0 + j, a.H) * a.W;
            for (int i = lx; i < a.tw; i += 32) atomicAdd(&h[row[refl101(x0 + i, a.W)] * EQ_COPIES + c], 1u);
        }
    }
    __syncthreads();
    const int k = threadIdx.x;
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < EQ_COPIES; ++j) s += h[k * EQ_COPIES + ((j + k) & (EQ_COPIES - 1))];
    a.hist[((size_t)img * a.units + u) * 256 + k] = s;
}

// inclusive sum over the 256 threads of a workgroup; sh[255] holds the total until the next barrier
__device__ __forceinline__ int eq_scan256(int v, int* sh) {
    const int k = threadIdx.x;
    sh[k] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int t = k >= d ? sh[k - d] : 0;
        __syncthreads();
        sh[k] += t;
        __syncthreads();
    }
    return sh[k];
}

__device__ __forceinline__ uint8_t eq_sat(float x) {   // saturate_cast<uchar>: half to even, clipped
    return (uint8_t)(int)fminf(fmaxf(rintf(x), 0.f), 255.f);
}

// One workgroup per table, thread k = bin k: a CLAHE tile's clipped and redistributed histogram,
// or (blockIdx.x = 0 only) a HIST image's, summed over its EQ_HCH parts, from the first non-empty bin.
__global__ void __launch_bounds__(256) k_eq_lut_sets(EqArgs a) {
#pragma clang fp contract(off)
    const int img = blockIdx.z, t = blockIdx.x, mode = a.mode[img], k = threadIdx.x;
    if (mode == MFE_EQ_NONE || (mode == MFE_EQ_HIST && t > 0)) return;
    __shared__ int sh[256];
    __shared__ int first[2];
    const unsigned* hist = a.hist + (size_t)img * a.units * 256;
    uint8_t* lut = a.lut + ((size_t)img * a.tiles_x * a.tiles_y + t) * 256;
    if (mode == MFE_EQ_HIST) {
        int h = 0;
        for (int u = 0; u < EQ_HCH; ++u) h += (int)hist[u * 256 + k];
        const int cum = eq_scan256(h, sh);
        if (h > 0 && cum == h) {   // the first non-empty bin: one thread
            first[0] = k;
            first[1] = h;
        }
        __syncthreads();
        const int px = a.W * a.H, i = first[0], hi = first[1];
        if (hi == px) {            // a constant image stays as it is
            lut[k] = (uint8_t)k;
        } else {
            const float scale = 255.f / (float)(px - hi);
            lut[k] = k <= i ? (uint8_t)0 : eq_sat((float)(cum - hi) * scale);
        }
        return;
    }
    int h = (int)hist[t * 256 + k];
    const int clip = a.clip[img];
    if (clip > 0) {
        eq_scan256(h > clip ? h - clip : 0, sh);
        const int excess = sh[255];
        __syncthreads();
        h = min(h, clip) + excess / 256;
        const int residual = excess % 256;
        if (residual) {
            const int step = max(256 / residual, 1);
            if (k % step == 0 && k / step < residual) ++h;
        }
    }
    const int cum = eq_scan256(h, sh);
    const float lut_scale = 255.f / (float)(a.tw * a.th);
    lut[k] = eq_sat((float)cum * lut_scale);
}

// Packed image -> level 0 of its slot.  One workgroup per interpolation cell (cx, cy), 0 <= cx <=
// tiles_x: the pixels with floor(txf) = cx - 1 and floor(tyf) = cy - 1, which share their (at most)
// four tiles; the four tables in LDS.  The cell's extent is taken one pixel wider than the exact
// bounds and every pixel tested with the float expression the blend itself uses, so each pixel
// is written by exactly one workgroup whatever the rounding of x * (1.f / tw).  HIST and NONE
// images go through the same cells with one table and none.
__global__ void __launch_bounds__(256) k_eq_apply_sets(EqArgs a) {
#pragma clang fp contract(off)
    const int img = blockIdx.z, mode = a.mode[img];
    const int cx = blockIdx.x % (a.tiles_x + 1), cy = blockIdx.x / (a.tiles_x + 1);
    const uint8_t* src = a.images + (size_t)img * a.W * a.H;
    uint8_t* dst = a.tab[a.slots[img]].lv[0].img;
    __shared__ uint8_t l[4][256];
    if (mode != MFE_EQ_NONE) {
        const uint8_t* lut = a.lut + (size_t)img * a.tiles_x * a.tiles_y * 256;
        const int tx1 = max(cx - 1, 0), tx2 = min(cx, a.tiles_x - 1);
        const int ty1 = max(cy - 1, 0), ty2 = min(cy, a.tiles_y - 1);
        const int k = threadIdx.x;
        if (mode == MFE_EQ_HIST) {
            l[0][k] = lut[k];
        } else {
            l[0][k] = lut[(ty1 * a.tiles_x + tx1) * 256 + k];
            l[1][k] = lut[(ty1 * a.tiles_x + tx2) * 256 + k];
            l[2][k] = lut[(ty2 * a.tiles_x + tx1) * 256 + k];
            l[3][k] = lut[(ty2 * a.tiles_x + tx2) * 256 + k];
        }
        __syncthreads();
    }
    const int x_lo = max(((2 * cx - 1) * a.tw) / 2 - 1, 0), x_hi = min(((2 * cx + 1) * a.tw) / 2 + 1, a.W - 1);
    const int y_lo = max(((2 * cy - 1) * a.th) / 2 - 1, 0), y_hi = min(((2 * cy + 1) * a.th) / 2 + 1, a.H - 1);
    const float inv_tw = 1.f / (float)a.tw, inv_th = 1.f / (float)a.th;
    for (int y = y_lo + (int)(threadIdx.x >> 5); y <= y_hi; y += 8) {
        const float tyf = (float)y * inv_th - 0.5f, fy = floorf(tyf);
        if ((int)fy != cy - 1) continue;
        const float ya = tyf - fy, ya1 = 1.f - ya;
        for (int x = x_lo + (int)(threadIdx.x & 31); x <= x_hi; x += 32) {
            const float txf = (float)x * inv_tw - 0.5f, fx = floorf(txf);
            if ((int)fx != cx - 1) continue;
            const size_t o = (size_t)y * a.W + x;
            const int v = src[o];
            if (mode == MFE_EQ_NONE) {
                dst[o] = (uint8_t)v;
            } else if (mode == MFE_EQ_HIST) {
                dst[o] = l[0][v];
            } else {
                const float xa = txf - fx, xa1 = 1.f - xa;
                const float top = (float)l[0][v] * xa1 + (float)l[1][v] * xa;
                const float bot = (float)l[2][v] * xa1 + (float)l[3][v] * xa;
                dst[o] = eq_sat(top * ya1 + bot * ya);
            }
        }
    }
}

// ------------------------------------------------------------------- FAST --
// circle of radius 3 (fast.cpp makeOffsets, pattern 16): (dx, dy)
__constant__ int c_fast_dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__constant__ int c_fast_dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

// cornerScore<16> (fast_score.cpp): d[k] = v - circle[k mod 16], k = 0..24
__device__ int fast_corner_score(const int* d, int threshold) {
    int a0 = threshold;
    for (int k = 0; k < 16; k += 2) {
        int a = min(min(d[k + 1], d[k + 2]), d[k + 3]);
        if (a <= a0) continue;
        a = min(a, d[k + 4]);
        a = min(a, d[k + 5]);
        a = min(a, d[k + 6]);
        a = min(a, d[k + 7]);
        a = min(a, d[k + 8]);
        a0 = max(a0, min(a, d[k]));
        a0 = max(a0, min(a, d[k + 9]));
    }
    int b0 = -a0;
    for (int k = 0; k < 16; k += 2) {
        int b = max(max(d[k + 1], d[k + 2]), d[k + 3]);
        b = max(b, d[k + 4]);
        b = max(b, d[k + 5]);
        if (b >= b0) continue;
        b = max(b, d[k + 6]);
        b = max(b, d[k + 7]);
        b = max(b, d[k + 8]);
        b0 = min(b0, max(b, d[k]));
        b0 = min(b0, max(b, d[k + 9]));
    }
    return -b0 - 1;
}

// true if the 16-bit circle mask holds 9 contiguous set bits (cyclically)
__device__ __forceinline__ bool run9(unsigned m) {
    const unsigned m2 = m | (m << 16);
    unsigned r = m2 & (m2 >> 1);   // 2 in a row
    r &= r >> 2;                   // 4
    r &= r >> 4;                   // 8
    r &= m2 >> 8;                  // 9
    return (r & 0xffffu) != 0;
}

// score map: 0x100 | score for corners, 0 elsewhere (the non-max test reads
// non-corner neighbours as score 0, as fast.cpp's row buffers do)
__device__ __forceinline__ void fast_px(const uint8_t* __restrict__ img, int w, int h, int threshold,
                                        uint16_t* __restrict__ score, int x, int y) {
    if (x >= w || y >= h) return;
    uint16_t out = 0;
    if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
        const int v = img[(size_t)y * w + x];
        int c[16];
        unsigned bright = 0, dark = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            c[k] = img[(size_t)(y + c_fast_dy[k]) * w + x + c_fast_dx[k]];
            bright |= (unsigned)(c[k] > v + threshold) << k;
            dark |= (unsigned)(c[k] < v - threshold) << k;
        }
        if (run9(bright) || run9(dark)) {
            int d[25];
#pragma unroll
            for (int k = 0; k < 25; ++k) d[k] = v - c[k & 15];
            out = (uint16_t)(0x100 | (fast_corner_score(d, threshold) & 0xff));
        }
    }
    score[(size_t)y * w + x] = out;
}

// blockIdx.z = the set: level 0 of its slot -> the set's score map
__global__ void __launch_bounds__(256) k_fast_sets(const Pyr* __restrict__ tab, const int32_t* __restrict__ slots,
                                                   int threshold, uint16_t* __restrict__ score) {
    const Level L = tab[slots[blockIdx.z]].lv[0];
    fast_px(L.img, L.w, L.h, threshold, score + (size_t)blockIdx.z * L.w * L.h, blockIdx.x * 16 + (threadIdx.x & 15),
            blockIdx.y * 16 + (threadIdx.x >> 4));
}

// one wave per row: corners whose score beats all 8 neighbours (and pass the
// mask); pass 0 counts per row, pass 1 writes at row_off[y] + rank in raster order
__device__ __forceinline__ void fast_rows_row(const uint16_t* __restrict__ score, const uint8_t* __restrict__ mask,
                                              int w, int h, int pass, int* __restrict__ row_count,
                                              const int* __restrict__ row_off, int max_kp, float* __restrict__ xy,
                                              float* __restrict__ resp, int y, int lane) {
    if (y >= h) return;
    int count = 0;
    for (int x0 = 0; x0 < w; x0 += 64) {
        const int x = x0 + lane;
        bool keep = false;
        int s = 0;
        if (x >= 3 && x < w - 3 && y >= 3 && y < h - 3) {
            const uint16_t c = score[(size_t)y * w + x];
            s = c & 0xff;
            keep = (c >> 8) != 0;
            if (keep) {
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx)
                        if ((dx || dy) && !(s > (score[(size_t)(y + dy) * w + x + dx] & 0xff))) keep = false;
                if (mask && mask[(size_t)y * w + x] == 0) keep = false;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (pass == 1 && keep) {
            const int rank = __popcll(bal & ((1ull << lane) - 1ull));
            const int pos = row_off[y] + count + rank;
            if (pos < max_kp) {
                xy[2 * pos] = (float)x;
                xy[2 * pos + 1] = (float)y;
                resp[pos] = (float)s;
            }
        }
        count += __popcll(bal);
    }
    if (pass == 0 && lane == 0) row_count[y] = count;
}

// The per-set work areas of mfe_fast_grid_sets, set s at s times the single call's
// extent: score and mask [w h], rows [2][h] (counts, offsets), kp [kp_cap][3] (xy,
// then the responses).
struct GridWork {
    uint16_t* score;
    uint8_t* mask;
    int* rows;
    float* kp;
    int w, h, kp_cap;
};

// blockIdx.y = the set
__global__ void __launch_bounds__(256) k_fast_rows_sets(GridWork g, int pass, int max_kp) {
    const size_t s = blockIdx.y, px = (size_t)g.w * g.h;
    int* rows = g.rows + s * 2 * g.h;
    float* kp = g.kp + s * 3 * g.kp_cap;
    fast_rows_row(g.score + s * px, g.mask + s * px, g.w, g.h, pass, rows, rows + g.h, max_kp, kp,
                  kp + 2 * (size_t)g.kp_cap, blockIdx.x * 4 + (threadIdx.x >> 6), threadIdx.x & 63);
}

// --------------------------------------------------------------------- LK --
__device__ __forceinline__ long long wave_sum64(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor((int)(v & 0xffffffffLL), m, 64);
        const int hi = __shfl_xor((int)(v >> 32), m, 64);
        v += ((long long)hi << 32) | (unsigned int)lo;
    }
    return v;
}

template <typename Px>
__device__ __forceinline__ int bilinear(const Px* img, int w, int h, int x, int y, int w00, int w01, int w10,
                                        int w11) {
    const int x0 = refl101(x, w), x1 = refl101(x + 1, w);
    const Px* r0 = img + (size_t)refl101(y, h) * w;
    const Px* r1 = img + (size_t)refl101(y + 1, h) * w;
    return (int)r0[x0] * w00 + (int)r0[x1] * w01 + (int)r1[x0] * w10 + (int)r1[x1] * w11;
}

// The derivatives beyond the image are zero: given raw images,
// calcOpticalFlowPyrLK pads derivI with copyMakeBorder(BORDER_CONSTANT)
// (lkpyramid.cpp); only the pyramid images use BORDER_REFLECT_101.
__device__ __forceinline__ int bilinear_zero(const int16_t* img, int w, int h, int x, int y, int w00, int w01,
                                             int w10, int w11) {
    auto at = [&](int yy, int xx) -> int {
        return (xx >= 0 && xx < w && yy >= 0 && yy < h) ? (int)img[(size_t)yy * w + xx] : 0;
    };
    return at(y, x) * w00 + at(y, x + 1) * w01 + at(y + 1, x) * w10 + at(y + 1, x + 1) * w11;
}

__device__ __forceinline__ void lk_weights(float a, float b, int& w00, int& w01, int& w10, int& w11) {
    w00 = (int)rintf((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
    w01 = (int)rintf(a * (1.f - b) * (float)(1 << W_BITS));
    w10 = (int)rintf((1.f - a) * b * (float)(1 << W_BITS));
    w11 = (1 << W_BITS) - w00 - w01 - w10;
}

constexpr int LK_SLOTS = 4;   // window pixels per lane: win <= 16 (win^2 <= 256)

// One point on one wavefront (every lane calls it with the same arguments):
// (nx, ny) is nextPts[ptidx], the initial guess on entry and the tracked
// position on exit, the same in every lane; returns the status.  Shared by
// k_lk_sets, k_stereo_match_sets and the k_trk_* kernels.
__device__ __forceinline__ bool lk_point(const Pyr& P, const Pyr& N, float ppx, float ppy, float& nx, float& ny,
                                         int win, int max_level, int max_iter, double eps, int lane) {
#pragma clang fp contract(off)
    const float half = (float)(win - 1) * 0.5f;
    const int npix = win * win;
    bool st = true;
    for (int level = max_level; level >= 0; --level) {
        const Level I = P.lv[level], J = N.lv[level];
        const float sc = (float)(1. / (1 << level));
        const float px = ppx * sc - half, py = ppy * sc - half;
        float gx, gy;
        if (level == max_level) {
            gx = nx * sc;
            gy = ny * sc;
        } else {
            gx = nx * 2.f;
            gy = ny * 2.f;
        }
        nx = gx;
        ny = gy;
        gx -= half;
        gy -= half;
        const int ipx = (int)floorf(px), ipy = (int)floorf(py);
        if (ipx < -win || ipx >= I.w || ipy < -win || ipy >= I.h) {
            if (level == 0) st = false;
            continue;
        }
        int w00, w01, w10, w11;
        lk_weights(px - (float)ipx, py - (float)ipy, w00, w01, w10, w11);
        int ival[LK_SLOTS], ixv[LK_SLOTS], iyv[LK_SLOTS];
        long long s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int q = 0; q < LK_SLOTS; ++q) {
            const int p = lane + 64 * q;
            ival[q] = ixv[q] = iyv[q] = 0;
            if (p < npix) {
                const int yy = p / win, xx = p - yy * win;
                ival[q] = descale(bilinear(I.img, I.w, I.h, ipx + xx, ipy + yy, w00, w01, w10, w11), W_BITS - 5);
                ixv[q] = descale(bilinear_zero(I.ix, I.w, I.h, ipx + xx, ipy + yy, w00, w01, w10, w11), W_BITS);
                iyv[q] = descale(bilinear_zero(I.iy, I.w, I.h, ipx + xx, ipy + yy, w00, w01, w10, w11), W_BITS);
                s11 += (long long)ixv[q] * ixv[q];
                s12 += (long long)ixv[q] * iyv[q];
                s22 += (long long)iyv[q] * iyv[q];
            }
        }
        s11 = wave_sum64(s11);
        s12 = wave_sum64(s12);
        s22 = wave_sum64(s22);
        const float A11 = (float)s11 * FLT_SCALE, A12 = (float)s12 * FLT_SCALE, A22 = (float)s22 * FLT_SCALE;
        float D = A11 * A22 - A12 * A12;
        const float min_eig =
            (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
        if ((double)min_eig < 1e-4 || D < 1.1920928955078125e-7f) {
            if (level == 0) st = false;
            continue;
        }
        D = 1.f / D;
        float pdx = 0.f, pdy = 0.f;
        for (int j = 0; j < max_iter; ++j) {
            const int inx = (int)floorf(gx), iny = (int)floorf(gy);
            if (inx < -win || inx >= J.w || iny < -win || iny >= J.h) {
                if (level == 0) st = false;
                break;
            }
            lk_weights(gx - (float)inx, gy - (float)iny, w00, w01, w10, w11);
            long long t1 = 0, t2 = 0;
#pragma unroll
            for (int q = 0; q < LK_SLOTS; ++q) {
                const int p = lane + 64 * q;
                if (p < npix) {
                    const int yy = p / win, xx = p - yy * win;
                    const int diff =
                        descale(bilinear(J.img, J.w, J.h, inx + xx, iny + yy, w00, w01, w10, w11), W_BITS - 5) -
                        ival[q];
                    t1 += (long long)diff * ixv[q];
                    t2 += (long long)diff * iyv[q];
                }
            }
            t1 = wave_sum64(t1);
            t2 = wave_sum64(t2);
            const float b1 = (float)t1 * FLT_SCALE, b2 = (float)t2 * FLT_SCALE;
            const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
            gx += dx;
            gy += dy;
            nx = gx + half;
            ny = gy + half;
            if ((double)dx * dx + (double)dy * dy <= eps * eps) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
                nx -= dx * 0.5f;
                ny -= dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
    }
    return st;
}

// mfe_lk_sets: the per-point set index is the same in every lane of the
// wavefront, so the descriptors come through scalar loads
struct LkSetsArgs {
    const Pyr* tab;
    const int32_t* pt_set;      // [n]
    const int32_t* set_slots;   // [n_sets][2]: previous, next
    const float* prev_pts;
    float* next_pts;
    uint8_t* status;
    double eps;
    int n, win, max_level, max_iter;
};

__global__ void __launch_bounds__(64) k_lk_sets(LkSetsArgs a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= a.n) return;
    const int s = __builtin_amdgcn_readfirstlane(a.pt_set[i]);
    const Pyr& P = a.tab[a.set_slots[2 * s]];
    const Pyr& N = a.tab[a.set_slots[2 * s + 1]];
    float nx = a.next_pts[2 * i], ny = a.next_pts[2 * i + 1];
    const bool st = lk_point(P, N, a.prev_pts[2 * i], a.prev_pts[2 * i + 1], nx, ny, a.win, a.max_level, a.max_iter,
                             a.eps, lane);
    if (lane == 0) {
        a.next_pts[2 * i] = nx;
        a.next_pts[2 * i + 1] = ny;
        a.status[i] = st ? 1 : 0;
    }
}

// ---------------------------------------------------------- camera models --
struct CamModel {
    double fx, fy, cx, cy, k[4], R[9], nfx, nfy, ncx, ncy;
    int model;
};

// Pixel -> normalised, undistorted coordinates (before any rectification);
// false = the fisheye solution was rejected.  Shared by k_undistort_sets and
// k_two_point_ransac.
__device__ __forceinline__ bool undistort_norm(const CamModel& c, double px, double py, double& xo, double& yo) {
#pragma clang fp contract(off)
    double x = (px - c.cx) / c.fx, y = (py - c.cy) / c.fy;
    if (c.model == MFE_EQUIDISTANT) {
        // cv2.fisheye.undistortPoints (4.x) with its default criteria (COUNT +
        // EPS, 10, 1e-8): theta_d clamped to the model's 180-degree field of
        // view, Newton on theta until |step| < 1e-8; a solution that did not
        // converge or flipped sign goes out as (-1e6, -1e6), unrectified
        const double td = fmin(sqrt(x * x + y * y), M_PI / 2);
        double th = td, scale = 0.0;
        bool conv = false;
        if (td > 1e-8) {
            for (int it = 0; it < 10; ++it) {
                const double t2 = th * th, t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
                const double k0t2 = c.k[0] * t2, k1t4 = c.k[1] * t4, k2t6 = c.k[2] * t6, k3t8 = c.k[3] * t8;
                const double fix = (th * (1 + k0t2 + k1t4 + k2t6 + k3t8) - td) /
                                   (1 + 3 * k0t2 + 5 * k1t4 + 7 * k2t6 + 9 * k3t8);
                th = th - fix;
                if (fabs(fix) < 1e-8) { conv = true; break; }
            }
            scale = tan(th) / td;
        } else {
            conv = true;
        }
        if (!conv || th < 0) return false;
        x = x * scale;
        y = y * scale;
    } else {   // cv2.undistortPoints: 5 fixed-point iterations
        const double x0 = x, y0 = y, k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = 0.0;
        for (int it = 0; it < 5; ++it) {
            const double r2 = x * x + y * y;
            const double icdist = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
            const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
            const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
    }
    xo = x;
    yo = y;
    return true;
}

// mfe_undistort of one point: undistort_norm, the rectification c.R and the new
// intrinsics; a rejected fisheye solution goes out as (-1e6, -1e6), unrectified.
// Shared by k_undistort_sets and k_stereo_match_sets.
__device__ __forceinline__ void undistort_rect(const CamModel& c, double px, double py, double& xo, double& yo) {
#pragma clang fp contract(off)
    double x, y;
    if (!undistort_norm(c, px, py, x, y)) {
        xo = -1000000.0;
        yo = -1000000.0;
        return;
    }
    const double X = c.R[0] * x + c.R[1] * y + c.R[2];
    const double Y = c.R[3] * x + c.R[4] * y + c.R[5];
    const double Wz = c.R[6] * x + c.R[7] * y + c.R[8];
    xo = c.nfx * X / Wz + c.ncx;
    yo = c.nfy * Y / Wz + c.ncy;
}

// mfe_distort of one normalised point.  Shared by k_distort and k_stereo_match_sets.
__device__ __forceinline__ void distort_pix(const CamModel& c, double x, double y, double& xo, double& yo) {
#pragma clang fp contract(off)
    double xd, yd;
    if (c.model == MFE_EQUIDISTANT) {   // cv2.fisheye.distortPoints
        const double r = sqrt(x * x + y * y);
        const double th = atan(r), t2 = th * th;
        const double td = th * (1 + c.k[0] * t2 + c.k[1] * (t2 * t2) + c.k[2] * (t2 * t2 * t2) + c.k[3] * (t2 * t2 * t2 * t2));
        const double s = r > 1e-8 ? td / r : 1.0;
        xd = x * s;
        yd = y * s;
    } else {   // cv2.projectPoints, zero pose
        const double k1 = c.k[0], k2 = c.k[1], p1 = c.k[2], p2 = c.k[3], k3 = 0.0;
        const double r2 = x * x + y * y;
        const double radial = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;
        xd = x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        yd = y * radial + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    }
    xo = c.fx * xd + c.cx;
    yo = c.fy * yd + c.cy;
}

// mfe_undistort_sets: point t with the model of its set
__global__ void __launch_bounds__(256) k_undistort_sets(const CamModel* __restrict__ cams,
                                                        const int32_t* __restrict__ pt_set, int n,
                                                        const double* __restrict__ in, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double x, y;
    undistort_rect(cams[pt_set[t]], in[2 * t], in[2 * t + 1], x, y);
    out[2 * t] = x;
    out[2 * t + 1] = y;
}

__global__ void __launch_bounds__(256) k_distort(CamModel c, int n, const double* __restrict__ in,
                                                 double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    double x, y;
    distort_pix(c, in[2 * t], in[2 * t + 1], x, y);
    out[2 * t] = x;
    out[2 * t + 1] = y;
}

// ------------------------------------------------------- two-point RANSAC --
// include/msckf_ransac.h states the algorithm.  One workgroup of 8 waves per
// point set; the set's c_i (compacted to the raw list), |d_i|, the raw ->
// point index map and the markers live in LDS (148 KB of the CU's 160 KB at
// the 4096-point cap).  The per-point passes spread the points over the 512
// threads; the hypotheses go one per wave, the raw list over its 64 lanes.
// Every sum is a per-thread partial in index order, an xor butterfly over the
// wave and the 8 wave partials added in wave order: the same bits every run.
constexpr int RS_THREADS = 512, RS_WAVES = RS_THREADS / 64, RS_MAXN = MFE_RANSAC_MAX_SET_POINTS;

struct RansacArgs {
    const int32_t* set_off;
    const double *pts_prev, *pts_curr, *R, *intr, *coeffs;
    const int32_t* model;
    const uint32_t* draws;
    double* work;   // [total][4]: compensated previous point, current point (normalised)
    uint8_t* inlier;
    double* info;
    double inlier_error;
    int n_hyp;
};

template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m, 64);
    __syncthreads();   // red may still be read by the reduction before
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) s += red[w * K + k];
        v[k] = s;
    }
}

__device__ __forceinline__ double pick3(double v0, double v1, double v2, int k) {
    return k == 0 ? v0 : (k == 1 ? v1 : v2);
}

__global__ void __launch_bounds__(RS_THREADS) k_two_point_ransac(RansacArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_c0[RS_MAXN], s_c1[RS_MAXN], s_c2[RS_MAXN], s_dist[RS_MAXN];
    __shared__ int s_ridx[RS_MAXN];
    __shared__ uint8_t s_mark[RS_MAXN];   // by point index
    __shared__ double s_red[RS_WAVES * 5];
    __shared__ int s_wcnt[2][RS_WAVES];
    __shared__ double s_bm[RS_WAVES][3];
    __shared__ int s_bi[RS_WAVES][3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = a.set_off[s], n = a.set_off[s + 1] - o0;
    const double nan = __builtin_nan("");
    CamModel cam{};
    cam.fx = a.intr[4 * s]; cam.fy = a.intr[4 * s + 1]; cam.cx = a.intr[4 * s + 2]; cam.cy = a.intr[4 * s + 3];
    for (int i = 0; i < 4; ++i) cam.k[i] = a.coeffs[4 * s + i];
    cam.model = a.model[s];
    const double* R = a.R + 9 * s;
    const double r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5];
    double unit = 2.0 / (cam.fx + cam.fy);

    // steps 2-3: undistort, rotation-compensate, sum of the norms
    double nsum[1] = {0.0};
    for (int i = tid; i < n; i += RS_THREADS) {
        const size_t g = (size_t)(o0 + i);
        double xp, yp, xc, yc;
        if (!undistort_norm(cam, a.pts_prev[2 * g], a.pts_prev[2 * g + 1], xp, yp)) xp = yp = -1000000.0;
        if (!undistort_norm(cam, a.pts_curr[2 * g], a.pts_curr[2 * g + 1], xc, yc)) xc = yc = -1000000.0;
        const double xr = r0 * xp + r1 * yp + r2, yr = r3 * xp + r4 * yp + r5;
        a.work[4 * g] = xr; a.work[4 * g + 1] = yr; a.work[4 * g + 2] = xc; a.work[4 * g + 3] = yc;
        nsum[0] += sqrt(xr * xr + yr * yr) + sqrt(xc * xc + yc * yc);
    }
    block_sum(nsum, s_red);
    const double scale = M_SQRT2 * (double)(2 * n) / nsum[0];   // step 4 (NaN for an empty set)
    unit = unit * scale;

    // steps 5-6 and 9: each thread re-reads the points it wrote; the kept ones are
    // compacted in index order, 512 at a time (ballot rank within the wave, the wave
    // counts of the chunk through LDS)
    const double pre_thr = 50.0 * unit;
    double dsum[1] = {0.0};
    int n_raw = 0;
    for (int c0 = 0, it = 0; c0 < n; c0 += RS_THREADS, ++it) {
        const int i = c0 + tid;
        bool keep = false;
        double cx = 0.0, cy = 0.0, cz = 0.0, dist = 0.0;
        if (i < n) {
            const size_t g = (size_t)(o0 + i);
            const double xp = a.work[4 * g] * scale, yp = a.work[4 * g + 1] * scale;
            const double xc = a.work[4 * g + 2] * scale, yc = a.work[4 * g + 3] * scale;
            const double dx = xp - xc, dy = yp - yc;
            dist = sqrt(dx * dx + dy * dy);
            keep = !(dist > pre_thr);
            cx = dy; cy = -dx; cz = xp * yc - yp * xc;
            s_mark[i] = 0;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wcnt[it & 1][wave] = __popcll(bal);
        __syncthreads();
        int off = n_raw, tot = 0;
#pragma unroll
        for (int w = 0; w < RS_WAVES; ++w) {
            const int cw = s_wcnt[it & 1][w];
            if (w < wave) off += cw;
            tot += cw;
        }
        if (keep) {
            const int r = off + __popcll(bal & ((1ull << lane) - 1ull));   // r <= i < RS_MAXN
            s_c0[r] = cx; s_c1[r] = cy; s_c2[r] = cz; s_dist[r] = dist; s_ridx[r] = i;
            dsum[0] += dist;
        }
        n_raw += tot;
    }
    block_sum(dsum, s_red);   // its barriers also publish the LDS lists
    const double mean_dist = n_raw > 0 ? dsum[0] / (double)n_raw : nan;
    const double thr = a.inlier_error * unit;

    double status, best_h = -1.0, best_cnt = 0.0, mr0 = nan, mr1 = nan, mr2 = nan, refit_err = nan;
    if (n_raw < 3) {   // step 7
        status = 2.0;
    } else if (mean_dist < unit) {   // step 8
        double cnt[1] = {0.0};
        for (int r = tid; r < n_raw; r += RS_THREADS) {
            const bool mk = !(s_dist[r] > thr);
            if (mk) s_mark[s_ridx[r]] = 1;
            cnt[0] += mk ? 1.0 : 0.0;
        }
        block_sum(cnt, s_red);
        best_cnt = cnt[0];
        status = 1.0;
    } else {   // step 10
        const double need = 0.2 * (double)n;
        int bc = -1, bh = -1, bk = 0;
        double bm0 = 0.0, bm1 = 0.0, bm2 = 0.0;
        for (int h = wave; h < a.n_hyp; h += RS_WAVES) {
            const size_t dq = ((size_t)s * a.n_hyp + h) * 2;
            const uint32_t i1 = a.draws[dq] % (uint32_t)n_raw;
            const uint32_t i2 = (i1 + 1u + a.draws[dq + 1] % (uint32_t)(n_raw - 1)) % (uint32_t)n_raw;
            const double a0 = s_c0[i1], a1 = s_c1[i1], a2 = s_c2[i1], b0 = s_c0[i2], b1 = s_c1[i2], b2 = s_c2[i2];
            const double t0 = fabs(a0) + fabs(b0), t1 = fabs(a1) + fabs(b1), t2 = fabs(a2) + fabs(b2);
            int k = 0;
            double tm = t0;
            if (t1 < tm) { k = 1; tm = t1; }
            if (t2 < tm) k = 2;
            const int ka = k == 0 ? 1 : 0, kb = k == 2 ? 1 : 2;   // the other two columns, ascending
            const double pa = pick3(a0, a1, a2, ka), qa = pick3(a0, a1, a2, kb), ra = pick3(a0, a1, a2, k);
            const double pb = pick3(b0, b1, b2, ka), qb = pick3(b0, b1, b2, kb), rb = pick3(b0, b1, b2, k);
            const double det = pa * qb - qa * pb;
            if (det == 0.0 || !isfinite(det)) continue;   // wave-uniform
            const double x0 = (qa * rb - ra * qb) / det, x1 = (ra * pb - pa * rb) / det;
            const double m0 = k == 0 ? 1.0 : x0, m1 = k == 1 ? 1.0 : (k == 0 ? x0 : x1), m2 = k == 2 ? 1.0 : x1;
            int cnt = 0;
            for (int r = lane; r < n_raw; r += 64)
                cnt += fabs(s_c0[r] * m0 + s_c1[r] * m1 + s_c2[r] * m2) < thr ? 1 : 0;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
            if ((double)cnt >= need && cnt > bc) {   // h ascends within the wave: the lowest h keeps a tie
                bc = cnt; bh = h; bk = k; bm0 = m0; bm1 = m1; bm2 = m2;
            }
        }
        if (lane == 0) {
            s_bi[wave][0] = bc; s_bi[wave][1] = bh; s_bi[wave][2] = bk;
            s_bm[wave][0] = bm0; s_bm[wave][1] = bm1; s_bm[wave][2] = bm2;
        }
        __syncthreads();
        int ww = 0;   // the largest set; among equals the lowest h
        for (int w = 1; w < RS_WAVES; ++w)
            if (s_bi[w][0] > s_bi[ww][0] || (s_bi[w][0] == s_bi[ww][0] && s_bi[w][1] < s_bi[ww][1])) ww = w;
        bc = s_bi[ww][0]; bh = s_bi[ww][1]; bk = s_bi[ww][2];
        bm0 = s_bm[ww][0]; bm1 = s_bm[ww][1]; bm2 = s_bm[ww][2];
        if (bc < 0) {
            status = 3.0;
        } else {
            status = 0.0;
            best_h = (double)bh;
            best_cnt = (double)bc;
            const int ka = bk == 0 ? 1 : 0, kb = bk == 2 ? 1 : 2;
            double ne[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // Spp Spq Sqq Spr Sqr of the best set
            for (int r = tid; r < n_raw; r += RS_THREADS) {
                const double c0 = s_c0[r], c1 = s_c1[r], c2 = s_c2[r];
                if (fabs(c0 * bm0 + c1 * bm1 + c2 * bm2) < thr) {
                    s_mark[s_ridx[r]] = 1;
                    const double p = pick3(c0, c1, c2, ka), q = pick3(c0, c1, c2, kb), rr = pick3(c0, c1, c2, bk);
                    ne[0] += p * p; ne[1] += p * q; ne[2] += q * q; ne[3] += p * rr; ne[4] += q * rr;
                }
            }
            block_sum(ne, s_red);
            const double det = ne[0] * ne[2] - ne[1] * ne[1];
            if (det != 0.0 && isfinite(det)) {
                const double x0 = (ne[1] * ne[4] - ne[3] * ne[2]) / det, x1 = (ne[3] * ne[1] - ne[0] * ne[4]) / det;
                mr0 = bk == 0 ? 1.0 : x0; mr1 = bk == 1 ? 1.0 : (bk == 0 ? x0 : x1); mr2 = bk == 2 ? 1.0 : x1;
                double es[1] = {0.0};
                for (int r = tid; r < n_raw; r += RS_THREADS)   // s_mark[..] here is the thread's own store
                    if (s_mark[s_ridx[r]]) es[0] += fabs(s_c0[r] * mr0 + s_c1[r] * mr1 + s_c2[r] * mr2);
                block_sum(es, s_red);
                refit_err = es[0] / (double)bc;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += RS_THREADS) a.inlier[o0 + i] = s_mark[i];
    if (tid == 0) {
        double* info = a.info + (size_t)s * MFE_RANSAC_INFO_LEN;
        info[0] = status; info[1] = (double)n_raw; info[2] = scale; info[3] = unit; info[4] = mean_dist;
        info[5] = best_h; info[6] = best_cnt; info[7] = mr0; info[8] = mr1; info[9] = mr2; info[10] = refit_err;
        info[11] = 0.0;
    }
}

// ----------------------------------------------------------- stereo match --
// include/msckf_pipeline.h states the algorithm: ImageProcessor.stereo_match
// as one kernel, one wavefront per point.  Every lane computes the same fp64
// camera arithmetic; the two LK runs spread their windows over the lanes.
// One point on one wavefront: steps 1-4 of the header; (c1x, c1y) is cam1_pts[i],
// the return value reason[i].  Shared by k_stereo_match_sets and k_trk_stereo*.
__device__ __forceinline__ int stereo_point(const Pyr& P0, const Pyr& P1, const CamModel& cam0, const CamModel& cam1,
                                            const double* E, double epi_thr, double eps, int win, int max_level,
                                            int max_iter, double px, double py, int lane, float& c1x, float& c1y) {
#pragma clang fp contract(off)
    double ux, uy, gx, gy;
    undistort_rect(cam0, px, py, ux, uy);   // step 1
    distort_pix(cam1, ux, uy, gx, gy);
    const float c0x = (float)px, c0y = (float)py;
    c1x = (float)gx;
    c1y = (float)gy;
    const bool st = lk_point(P0, P1, c0x, c0y, c1x, c1y, win, max_level, max_iter, eps, lane);   // step 2
    float bx = c0x, by = c0y;
    (void)lk_point(P1, P0, c1x, c1y, bx, by, win, max_level, max_iter, eps, lane);   // step 3
    const float dx = c0x - bx, dy = c0y - by;
    const float err = sqrtf(dx * dx + dy * dy);
    const float xmax = (float)(P1.lv[0].w - 1), ymax = (float)(P1.lv[0].h - 1);
    int reason = 0;
    if (!st) {
        reason = 1;
    } else if (!(err < 3.f)) {
        reason = 2;
    } else if (!(fabs(gy - (double)c1y) < 20.0)) {
        reason = 3;
    } else if (c1x < 0.f || c1x > xmax || c1y < 0.f || c1y > ymax) {
        reason = 4;
    } else {
        double u0x, u0y, u1x, u1y;
        if (!undistort_norm(cam0, (double)c0x, (double)c0y, u0x, u0y)) u0x = u0y = -1000000.0;
        if (!undistort_norm(cam1, (double)c1x, (double)c1y, u1x, u1y)) u1x = u1y = -1000000.0;
        const double lx = E[0] * u0x + E[1] * u0y + E[2], ly = E[3] * u0x + E[4] * u0y + E[5];
        const double error = fabs(u1x * lx) / sqrt(lx * lx + ly * ly);
        if (error > epi_thr) reason = 5;
    }
    return reason;
}

// mfe_stereo_match_sets: one table entry per set (cam0.R = R_guess, both cameras
// with new intrinsics [1 1 0 0]), read by every lane of the point's
// wavefront at the same address
struct StereoSet {
    CamModel cam0, cam1;
    double E[9];
    double epi_thr;
    int slot0, slot1;
};
struct StereoSetsArgs {
    const Pyr* tab;
    const StereoSet* sets;
    const int32_t* pt_set;
    const double* pts;
    float* cam1_pts;
    uint8_t *inlier, *reason;
    double eps;
    int n, win, max_level, max_iter;
};

__global__ void __launch_bounds__(64) k_stereo_match_sets(StereoSetsArgs a) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (i >= a.n) return;
    const StereoSet& S = a.sets[__builtin_amdgcn_readfirstlane(a.pt_set[i])];
    float c1x, c1y;
    const int reason = stereo_point(a.tab[S.slot0], a.tab[S.slot1], S.cam0, S.cam1, S.E, S.epi_thr, a.eps, a.win,
                                    a.max_level, a.max_iter, a.pts[2 * i], a.pts[2 * i + 1], lane, c1x, c1y);
    if (lane == 0) {
        a.cam1_pts[2 * i] = c1x;
        a.cam1_pts[2 * i + 1] = c1y;
        a.inlier[i] = reason == 0 ? 1 : 0;
        a.reason[i] = (uint8_t)reason;
    }
}

// ---------------------------------------------------- grid-selected detection --
// include/msckf_pipeline.h states the stages.  k_mask_clear_sets: 7 threads per
// occupied point, one per row of its 7 x 7 block (threads of overlapping blocks
// store the same 0).
__device__ __forceinline__ void mask_clear_row(float px, float py, int r, uint8_t* __restrict__ mask, int w, int h) {
    if (!(px >= 3.f && py >= 3.f && px < (float)(w + 3) && py < (float)(h + 3))) return;   // NaN: nothing
    const int x = (int)px, yy = (int)py - 3 + r;   // 3 <= x <= w + 2, yy >= 0
    if (yy >= h) return;
    const int x1 = min(x + 3, w - 1);
    for (int xx = x - 3; xx <= x1; ++xx) mask[(size_t)yy * w + xx] = 0;
}

// the occupied points of all sets, each in the mask of its set (occ_set[p])
__global__ void __launch_bounds__(256) k_mask_clear_sets(const float* __restrict__ occ,
                                                         const int32_t* __restrict__ occ_set, int n_occ,
                                                         uint8_t* __restrict__ mask, int w, int h) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int p = t / 7, r = t - 7 * p;
    if (p >= n_occ) return;
    mask_clear_row(occ[2 * p], occ[2 * p + 1], r, mask + (size_t)occ_set[p] * w * h, w, h);
}

// exclusive scan of the row counts in one workgroup: a contiguous run of rows
// per thread, the 256 run sums through LDS; *total = the sum
__device__ __forceinline__ void row_scan_block(const int* __restrict__ cnt, int* __restrict__ off, int h,
                                               int* __restrict__ total, int* s_part) {
    const int tid = threadIdx.x, per = (h + 255) / 256;
    const int r0 = min(tid * per, h), r1 = min(r0 + per, h);
    int s = 0;
    for (int r = r0; r < r1; ++r) s += cnt[r];
    s_part[tid] = s;
    __syncthreads();
    int base = 0;
    for (int j = 0; j < tid; ++j) base += s_part[j];
    for (int r = r0; r < r1; ++r) {
        off[r] = base;
        base += cnt[r];
    }
    if (tid == 255) *total = base;
}

// blockIdx.x = the set
__global__ void __launch_bounds__(256) k_row_scan_sets(GridWork g, int* __restrict__ totals) {
    __shared__ int s_part[256];
    int* rows = g.rows + (size_t)blockIdx.x * 2 * g.h;
    row_scan_block(rows, rows + g.h, g.h, totals + blockIdx.x, s_part);
}

struct GridArgs {
    const float *xy, *resp;   // the raster list
    const int* total;
    float *out_xy, *out_resp;   // [cell][k]
    int* cell_count;
    int cap, gh, gw, grid_col, k;
};

__device__ __forceinline__ long long wave_max64(long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor((int)(v & 0xffffffffLL), m, 64);
        const int hi = __shfl_xor((int)(v >> 32), m, 64);
        const long long o = ((long long)hi << 32) | (unsigned int)lo;
        v = o > v ? o : v;
    }
    return v;
}

// one workgroup per cell: the cell's keypoints counted, then k rounds of
// arg-max over the raster list.  key = response << 32 | (INT_MAX - index), so
// the larger key is the larger response and, among equals, the earlier
// keypoint; round r takes the largest key below round r - 1's.
__device__ __forceinline__ void grid_select_cell(const GridArgs& a, int cell, long long* s_key, int* s_cnt) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(*a.total, a.cap);
    auto in_cell = [&](int i) -> bool {
        const int x = (int)a.xy[2 * i], y = (int)a.xy[2 * i + 1];
        return (y / a.gh) * a.grid_col + x / a.gw == cell;
    };
    int cnt = 0;
    for (int i = tid; i < n; i += 256) cnt += in_cell(i) ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) a.cell_count[cell] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    long long prev = 0x7fffffffffffffffLL;
    for (int r = 0; r < a.k; ++r) {
        long long best = -1;
        for (int i = tid; i < n; i += 256) {
            if (!in_cell(i)) continue;
            const long long key = ((long long)(int)a.resp[i] << 32) | (long long)(0x7fffffff - i);
            if (key < prev && key > best) best = key;
        }
        best = wave_max64(best);
        __syncthreads();   // s_key may still be read by the round before
        if (lane == 0) s_key[wave] = best;
        __syncthreads();
        best = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
        if (best < 0) break;   // the same in every thread
        if (tid == 0) {
            const int idx = 0x7fffffff - (int)(best & 0xffffffffLL);
            const size_t o = (size_t)cell * a.k + r;
            a.out_xy[2 * o] = a.xy[2 * idx];
            a.out_xy[2 * o + 1] = a.xy[2 * idx + 1];
            a.out_resp[o] = a.resp[idx];
        }
        prev = best;
    }
}

// blockIdx.y = the set; a holds set 0's pointers, the outputs [n_sets][cells k]
__global__ void __launch_bounds__(256) k_grid_select_sets(GridArgs a, int kp_cap) {
    __shared__ long long s_key[4];
    __shared__ int s_cnt[4];
    const size_t s = blockIdx.y, cells = gridDim.x;
    a.xy += s * 3 * kp_cap;
    a.resp += s * 3 * kp_cap;
    a.total += s;
    a.out_xy += s * cells * a.k * 2;
    a.out_resp += s * cells * a.k;
    a.cell_count += s * cells;
    grid_select_cell(a, blockIdx.x, s_key, s_cnt);
}

// ------------------------------------------------------ device-side tracks --
// include/msckf_tracks.h states the steps.  The tables and every work area have
// the fixed stride [lane][cap]; the counts live on the device, so the launches are
// sized by cap and a wavefront or thread beyond its lane's count exits at once.
// Per-row work (the new cam0 / cam1 point, the keep flag, the cell) is indexed by
// the row of the previous table; the survivors of steps 2, 3 and 4 are index lists
// into it, each an order-preserving compaction of the one before.
constexpr int TRK_THREADS = 256, TRK_WAVES = TRK_THREADS / 64;

struct TrkHdr {
    long long next_id;
    int n, pad;
};

struct TrkDev {
    // the tables, [2][n_lanes] (a lane's current one is TrkLane::cur)
    long long* ids;   // [..][cap]
    int* life;        // [..][cap]
    float* cam0;      // [..][cap][2]
    float* cam1;
    TrkHdr* hdr;
    // work areas by the lane's place l in the call, rows as in the previous table
    float* c0;        // [l][cap][2] the tracked cam0 point
    float* c1;        // [l][cap][2] its stereo match
    uint8_t* flag;    // [l][cap]
    int* code;        // [l][cap] the cell of c0
    int* idx;         // [3][n_lanes][cap] the rows left after steps 2, 3, 4
    int* cnt;         // [3][n_lanes]
    // detection: the outputs of k_grid_select_sets and the candidates' matches
    int* g_cnt;       // [l][cells]
    float* g_resp;    // [l][cells k]
    float* g_xy;      // [l][cells k][2]
    float* cand_c1;   // [l][cells k][2]
    uint8_t* cand_inl;
    int* new_off;     // [l][cells] new features / rows of the next table before the cell
    int* out_off;
    // two-point RANSAC: sets 2 i and 2 i + 1 of the call's i-th RANSAC lane
    int* rs_off;      // [2 n_lanes + 1]
    double *rs_prev, *rs_curr, *rs_work, *rs_info;
    uint8_t* rs_inl;
    int n_lanes, cap, cells, grid_col, grid_min, grid_max, gh, gw;
};

struct TrkLane {
    StereoSet st;    // slot0 / slot1 = the current pair
    CamModel pub0;   // cam0 as publish undistorts it (st.cam1 serves for cam1)
    double H[9];
    int lane, cur, slot_prev, rs;   // rs: the lane's place among the call's RANSAC lanes, or -1
};

// what comes back, [l] as the call names the lanes
struct TrkOut {
    int* n;             // [l]
    int* counters;      // [l][4]
    int* n_total;       // [l]
    long long* next_id; // [l]
    long long* ids;     // [l][cap]
    double* uv;         // [l][cap][4]
    int by_lane;        // ids / uv are the message tables (msckf_handoff.h): [TrkLane::lane][cap], not [l][cap]
};

__device__ __forceinline__ int trk_cell(const TrkDev& d, float x, float y) {
    return (int)(y / (float)d.gh) * d.grid_col + (int)(x / (float)d.gw);
}

// steps 1-2: one wavefront per row of the lane's current table
__global__ void __launch_bounds__(64) k_trk_lk(TrkDev d, const TrkLane* __restrict__ lanes,
                                               const Pyr* __restrict__ tab, int win, int max_level, int max_iter,
                                               double eps) {
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    const int l = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const TrkLane& L = lanes[l];
    const size_t t = (size_t)L.cur * d.n_lanes + L.lane;
    if (r >= d.hdr[t].n) return;
    const size_t row = t * d.cap + r, w = (size_t)l * d.cap + r;
    const float px = d.cam0[2 * row], py = d.cam0[2 * row + 1];
    const double x = (double)px, y = (double)py;
    const double q0 = L.H[0] * x + L.H[1] * y + L.H[2];
    const double q1 = L.H[3] * x + L.H[4] * y + L.H[5];
    const double q2 = L.H[6] * x + L.H[7] * y + L.H[8];
    float nx = (float)(q0 / q2), ny = (float)(q1 / q2);
    const Pyr& N = tab[L.st.slot0];
    const bool st = lk_point(tab[L.slot_prev], N, px, py, nx, ny, win, max_level, max_iter, eps, lane);
    if (lane == 0) {
        const float xmax = (float)(N.lv[0].w - 1), ymax = (float)(N.lv[0].h - 1);
        d.c0[2 * w] = nx;
        d.c0[2 * w + 1] = ny;
        d.flag[w] = (st && !(nx < 0.f || nx > xmax || ny < 0.f || ny > ymax)) ? 1 : 0;
    }
}

// step 3: one wavefront per row left after step 2
__global__ void __launch_bounds__(64) k_trk_stereo(TrkDev d, const TrkLane* __restrict__ lanes,
                                                   const Pyr* __restrict__ tab, int win, int max_level, int max_iter,
                                                   double eps) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int l = __builtin_amdgcn_readfirstlane(blockIdx.y);
    if (j >= d.cnt[l]) return;
    const StereoSet& S = lanes[l].st;
    const size_t w = (size_t)l * d.cap + d.idx[(size_t)l * d.cap + j];
    float c1x, c1y;
    const int reason = stereo_point(tab[S.slot0], tab[S.slot1], S.cam0, S.cam1, S.E, S.epi_thr, eps, win, max_level,
                                    max_iter, (double)d.c0[2 * w], (double)d.c0[2 * w + 1], lane, c1x, c1y);
    if (lane == 0) {
        d.c1[2 * w] = c1x;
        d.c1[2 * w + 1] = c1y;
        d.flag[w] = reason == 0 ? 1 : 0;
    }
}

// step 7: one wavefront per candidate of the detection, b = cell k + place in the cell
__global__ void __launch_bounds__(64) k_trk_stereo_new(TrkDev d, const TrkLane* __restrict__ lanes,
                                                       const Pyr* __restrict__ tab, int win, int max_level,
                                                       int max_iter, double eps) {
    const int b = blockIdx.x, lane = threadIdx.x, k = d.grid_max;
    const int l = __builtin_amdgcn_readfirstlane(blockIdx.y);
    const int cell = b / k;
    if (b - cell * k >= min(k, d.g_cnt[(size_t)l * d.cells + cell])) return;
    const StereoSet& S = lanes[l].st;
    const size_t g = (size_t)l * d.cells * k + b;
    float c1x, c1y;
    const int reason = stereo_point(tab[S.slot0], tab[S.slot1], S.cam0, S.cam1, S.E, S.epi_thr, eps, win, max_level,
                                    max_iter, (double)d.g_xy[2 * g], (double)d.g_xy[2 * g + 1], lane, c1x, c1y);
    if (lane == 0) {
        d.cand_c1[2 * g] = c1x;
        d.cand_c1[2 * g + 1] = c1y;
        d.cand_inl[g] = reason == 0 ? 1 : 0;
    }
}

// Order-preserving compaction, one workgroup per lane: the rows of list stage - 1
// (stage 0: all rows of the table) whose flag is set become list stage.  256 rows at a
// time: the rank within the wave from the ballot, the wave counts of the chunk through
// LDS, added in wave order.
__global__ void __launch_bounds__(TRK_THREADS) k_trk_compact(TrkDev d, const TrkLane* __restrict__ lanes, int stage) {
    __shared__ int s_wcnt[2][TRK_WAVES];
    const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t NLC = (size_t)d.n_lanes * d.cap, base = (size_t)l * d.cap;
    const int n_in = min(stage == 0 ? d.hdr[(size_t)lanes[l].cur * d.n_lanes + lanes[l].lane].n
                                    : d.cnt[(stage - 1) * d.n_lanes + l], d.cap);
    const int* in = stage == 0 ? nullptr : d.idx + (stage - 1) * NLC + base;
    int* out = d.idx + stage * NLC + base;
    int n_out = 0;
    for (int c0 = 0, it = 0; c0 < n_in; c0 += TRK_THREADS, ++it) {
        const int j = c0 + tid;
        int r = 0;
        bool keep = false;
        if (j < n_in) {
            r = in ? in[j] : j;
            keep = d.flag[base + r] != 0;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wcnt[it & 1][wave] = __popcll(bal);
        __syncthreads();
        int off = n_out, tot = 0;
#pragma unroll
        for (int w = 0; w < TRK_WAVES; ++w) {
            const int cw = s_wcnt[it & 1][w];
            if (w < wave) off += cw;
            tot += cw;
        }
        if (keep) out[off + __popcll(bal & ((1ull << lane) - 1ull))] = r;   // off + rank <= j < cap
        n_out += tot;
    }
    if (tid == 0) d.cnt[stage * d.n_lanes + l] = n_out;
}

// ------------------------------------------- the motion statistic (msckf_standstill.h) --
// The k-th smallest (k = floor(q (n - 1))) of d2_j = |curr_j - prev_j|^2, j < n <=
// MOT_MAXN, in float32 with each product and the sum rounded once, by one workgroup of
// MOT_THREADS.  Pair j is row (idx ? idx[j] : j) of prev and curr.  The values live in
// LDS as their bit patterns (d2 >= +0, and non-negative floats order as their bits); the
// selection fixes one bit per pass from the most significant down: the candidates whose
// bit is 0 are counted from ballots, per wave in a register, the wave counts through LDS
// in wave order.  A wave whose first row lies beyond n returns at once (the barriers
// wait on the waves that remain); for n = 0 the value is NaN.  Thread 0 returns true
// and the value in `out`.  A caller must do nothing after the call but thread 0's stores of
// the result: no barrier, no LDS, no work that counts on the waves that have returned.
constexpr int MOT_THREADS = 256, MOT_WAVES = MOT_THREADS / 64, MOT_MAXN = MFE_RANSAC_MAX_SET_POINTS;

__device__ __forceinline__ bool motion_quantile(int n, double q, const float* __restrict__ prev,
                                                const float* __restrict__ curr, const int* __restrict__ idx,
                                                float& out) {
#pragma clang fp contract(off)
    __shared__ unsigned s_key[MOT_MAXN];
    __shared__ int s_wcnt[2][MOT_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6;
    n = min(n, MOT_MAXN);
    if (n <= 0) {
        out = __builtin_nanf("");
        return tid == 0;
    }
    if (wave * 64 >= n) return false;
    const int nw = min(MOT_WAVES, (n + 63) >> 6);   // the waves that stay: the first nw
    for (int j = tid; j < n; j += MOT_THREADS) {
        const size_t r = idx ? (size_t)idx[j] : (size_t)j;
        const float dx = curr[2 * r] - prev[2 * r], dy = curr[2 * r + 1] - prev[2 * r + 1];
        const float xx = dx * dx, yy = dy * dy;
        s_key[j] = __float_as_uint(xx + yy);
    }
    __syncthreads();
    int k = (int)floor(q * (double)(n - 1));
    k = max(0, min(k, n - 1));
    unsigned prefix = 0u, mask = 0u;
    for (int bit = 31, it = 0; bit >= 0; --bit, ++it) {
        const unsigned b = 1u << bit;
        int c = 0;
        for (int j0 = wave * 64; j0 < n; j0 += MOT_THREADS) {   // wave-uniform bounds: every lane ballots
            const int j = j0 + (tid & 63);
            bool zero = false;
            if (j < n) {
                const unsigned key = s_key[j];
                zero = (key & mask) == prefix && !(key & b);
            }
            c += __popcll(__ballot(zero));
        }
        if ((tid & 63) == 0) s_wcnt[it & 1][wave] = c;
        __syncthreads();
        int zeros = 0;
        for (int w = 0; w < nw; ++w) zeros += s_wcnt[it & 1][w];
        if (k >= zeros) {
            k -= zeros;
            prefix |= b;
        }
        mask |= b;
    }
    out = __uint_as_float(prefix);
    return tid == 0;
}

// mfe_motion_sets: one workgroup per set
__global__ void __launch_bounds__(MOT_THREADS) k_motion_sets(const int32_t* __restrict__ set_off,
                                                             const float* __restrict__ prev,
                                                             const float* __restrict__ curr, double q,
                                                             int32_t* __restrict__ n_out, float* __restrict__ d2_out) {
    const int s = blockIdx.x;
    const size_t o = (size_t)set_off[s];
    const int n = set_off[s + 1] - set_off[s];
    float v;
    if (motion_quantile(n, q, prev + 2 * o, curr + 2 * o, nullptr, v)) {
        n_out[s] = n;
        d2_out[s] = v;
    }
}

// behind step 4's compaction, one workgroup per lane of the call: the survivors' cam0 in the
// current table against their tracked point; writes the lane's record
__global__ void __launch_bounds__(MOT_THREADS) k_trk_motion(TrkDev d, const TrkLane* __restrict__ lanes, double q,
                                                            msckf::MotionRec* __restrict__ rec) {
    const int l = blockIdx.x;
    const TrkLane& L = lanes[l];
    const size_t row = ((size_t)L.cur * d.n_lanes + L.lane) * d.cap, w = (size_t)l * d.cap;
    const int n = min(d.cnt[2 * d.n_lanes + l], d.cap);
    float v;
    if (motion_quantile(n, q, d.cam0 + 2 * row, d.c0 + 2 * w, d.idx + ((size_t)2 * d.n_lanes + l) * d.cap, v)) {
        rec[L.lane].n = n;
        rec[L.lane].d2 = v;
    }
}

// step 4, before k_two_point_ransac: set_off of the call's 2 n_rs sets
__global__ void __launch_bounds__(64) k_trk_rs_off(TrkDev d, const int32_t* __restrict__ rs_lane, int n_rs) {
    if (threadIdx.x != 0) return;
    int off = 0;
    d.rs_off[0] = 0;
    for (int i = 0; i < n_rs; ++i) {
        const int c = d.cnt[d.n_lanes + rs_lane[i]];
        d.rs_off[2 * i + 1] = off + c;
        d.rs_off[2 * i + 2] = off + 2 * c;
        off += 2 * c;
    }
}

// blockIdx.y = the set: the matched rows' previous and current points as doubles
__global__ void __launch_bounds__(256) k_trk_rs_pack(TrkDev d, const TrkLane* __restrict__ lanes,
                                                     const int32_t* __restrict__ rs_lane) {
    const int s = blockIdx.y, l = rs_lane[s >> 1], j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.cnt[d.n_lanes + l]) return;
    const TrkLane& L = lanes[l];
    const int r = d.idx[((size_t)d.n_lanes + l) * d.cap + j];
    const size_t row = ((size_t)L.cur * d.n_lanes + L.lane) * d.cap + r, w = (size_t)l * d.cap + r;
    const float* prev = (s & 1) ? d.cam1 : d.cam0;
    const float* curr = (s & 1) ? d.c1 : d.c0;
    const size_t g = (size_t)d.rs_off[s] + j;
    d.rs_prev[2 * g] = (double)prev[2 * row];
    d.rs_prev[2 * g + 1] = (double)prev[2 * row + 1];
    d.rs_curr[2 * g] = (double)curr[2 * w];
    d.rs_curr[2 * g + 1] = (double)curr[2 * w + 1];
}

// steps 4-5: the RANSAC verdict of the matched rows (all kept in a lane without RANSAC)
// and the cell of each
__global__ void __launch_bounds__(256) k_trk_rs_flag(TrkDev d, const TrkLane* __restrict__ lanes) {
    const int l = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d.cnt[d.n_lanes + l]) return;
    const int rs = lanes[l].rs;
    const size_t w = (size_t)l * d.cap + d.idx[((size_t)d.n_lanes + l) * d.cap + j];
    bool keep = true;
    if (rs >= 0) keep = d.rs_inl[d.rs_off[2 * rs] + j] != 0 && d.rs_inl[d.rs_off[2 * rs + 1] + j] != 0;
    d.flag[w] = keep ? 1 : 0;
    d.code[w] = trk_cell(d, d.c0[2 * w], d.c0[2 * w + 1]);
}

// step 6: the survivors' 7 x 7 blocks cleared in the lane's mask (k_mask_clear_sets with
// the occupied list read through the survivor list)
__global__ void __launch_bounds__(256) k_trk_mask_clear(TrkDev d, uint8_t* __restrict__ mask, int w, int h) {
    const int l = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int p = t / 7, r = t - 7 * p;
    if (p >= d.cnt[2 * d.n_lanes + l]) return;
    const size_t o = (size_t)l * d.cap + d.idx[((size_t)2 * d.n_lanes + l) * d.cap + p];
    mask_clear_row(d.c0[2 * o], d.c0[2 * o + 1], r, mask + (size_t)l * w * h, w, h);
}

// steps 7-9, one workgroup per lane: per cell the survivors and the new features (the
// first grid_min inliers in candidate order), then the prefixes over the cells in cell
// order; writes the next table's header and the lane's scalar outputs
__global__ void __launch_bounds__(TRK_THREADS) k_trk_cells(TrkDev d, const TrkLane* __restrict__ lanes, TrkOut o) {
    __shared__ int s_ns[MFE_GRID_MAX_CELLS], s_nn[MFE_GRID_MAX_CELLS];
    const int l = blockIdx.x, tid = threadIdx.x, k = d.grid_max;
    const TrkLane& L = lanes[l];
    const size_t base = (size_t)l * d.cap;
    const int n_sv = d.cnt[2 * d.n_lanes + l];
    const int* sv = d.idx + ((size_t)2 * d.n_lanes + l) * d.cap;
    for (int cell = tid; cell < d.cells; cell += TRK_THREADS) {
        int ns = 0, nn = 0;
        for (int j = 0; j < n_sv; ++j) ns += d.code[base + sv[j]] == cell ? 1 : 0;
        const int nc = min(k, d.g_cnt[(size_t)l * d.cells + cell]);
        const uint8_t* inl = d.cand_inl + ((size_t)l * d.cells + cell) * k;
        for (int q = 0; q < nc && nn < d.grid_min; ++q) nn += inl[q] ? 1 : 0;
        s_ns[cell] = ns;
        s_nn[cell] = nn;
    }
    __syncthreads();
    if (tid != 0) return;
    int n_new = 0, n_rows = 0;
    for (int cell = 0; cell < d.cells; ++cell) {
        d.new_off[(size_t)l * d.cells + cell] = n_new;
        d.out_off[(size_t)l * d.cells + cell] = n_rows;
        n_new += s_nn[cell];
        n_rows += min(s_ns[cell] + s_nn[cell], k);
    }
    const TrkHdr cur = d.hdr[(size_t)L.cur * d.n_lanes + L.lane];
    TrkHdr nxt;
    nxt.next_id = cur.next_id + n_new;
    nxt.n = n_rows;
    nxt.pad = 0;
    d.hdr[(size_t)(L.cur ^ 1) * d.n_lanes + L.lane] = nxt;
    o.n[l] = n_rows;
    o.next_id[l] = nxt.next_id;
    o.counters[4 * l] = cur.n;
    o.counters[4 * l + 1] = d.cnt[l];
    o.counters[4 * l + 2] = d.cnt[d.n_lanes + l];
    o.counters[4 * l + 3] = n_sv;
}

// steps 8-9, one workgroup per (lane, cell): the cell's rows gathered in LDS (survivors
// in previous-table order, then the new ones), ranked by counting the rows that precede
// in the stable sort by lifetime when the cell is over grid_max, and written to the next
// table.  s_src: a survivor's row, or -(1 + b) for candidate b.
__global__ void __launch_bounds__(TRK_THREADS) k_trk_assemble(TrkDev d, const TrkLane* __restrict__ lanes, TrkOut o) {
    __shared__ int s_src[RS_MAXN], s_life[RS_MAXN];
    __shared__ int s_wcnt[2][TRK_WAVES];
    __shared__ int s_nn;
    const int cell = blockIdx.x, l = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = d.grid_max;
    const TrkLane& L = lanes[l];
    const size_t base = (size_t)l * d.cap, tcur = ((size_t)L.cur * d.n_lanes + L.lane) * d.cap;
    const size_t tnxt = ((size_t)(L.cur ^ 1) * d.n_lanes + L.lane) * d.cap;
    const size_t obase = (size_t)(o.by_lane ? L.lane : l) * d.cap;
    const int n_sv = d.cnt[2 * d.n_lanes + l];
    const int* sv = d.idx + ((size_t)2 * d.n_lanes + l) * d.cap;
    int ns = 0;
    for (int c0 = 0, it = 0; c0 < n_sv; c0 += TRK_THREADS, ++it) {
        const int j = c0 + tid;
        int r = 0;
        bool keep = false;
        if (j < n_sv) {
            r = sv[j];
            keep = d.code[base + r] == cell;
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wcnt[it & 1][wave] = __popcll(bal);
        __syncthreads();
        int off = ns, tot = 0;
#pragma unroll
        for (int w = 0; w < TRK_WAVES; ++w) {
            const int cw = s_wcnt[it & 1][w];
            if (w < wave) off += cw;
            tot += cw;
        }
        if (keep) {
            const int p = off + __popcll(bal & ((1ull << lane) - 1ull));   // p <= j < cap <= RS_MAXN
            s_src[p] = r;
            s_life[p] = d.life[tcur + r] + 1;
        }
        ns += tot;
    }
    if (tid == 0) {
        const int nc = min(k, d.g_cnt[(size_t)l * d.cells + cell]);
        const uint8_t* inl = d.cand_inl + ((size_t)l * d.cells + cell) * k;
        int nn = 0;
        for (int q = 0; q < nc && nn < d.grid_min && ns + nn < RS_MAXN; ++q)
            if (inl[q]) {
                s_src[ns + nn] = -(1 + cell * k + q);
                s_life[ns + nn] = 1;
                ++nn;
            }
        s_nn = nn;
    }
    __syncthreads();
    const int m = ns + s_nn;
    const bool prune = m > k;
    const long long id0 = d.hdr[(size_t)L.cur * d.n_lanes + L.lane].next_id + d.new_off[(size_t)l * d.cells + cell];
    const int o0 = d.out_off[(size_t)l * d.cells + cell];
    for (int i = tid; i < m; i += TRK_THREADS) {
        int pos = i;
        const int life = s_life[i];
        if (prune) {
            pos = 0;
            for (int j = 0; j < m; ++j) pos += (s_life[j] > life || (s_life[j] == life && j < i)) ? 1 : 0;
            if (pos >= k) continue;
        }
        const size_t out = (size_t)o0 + pos;   // below cells grid_max <= cap
        if (out >= (size_t)d.cap) continue;
        const int src = s_src[i];
        long long id;
        float a0, a1, b0, b1;
        if (src >= 0) {
            id = d.ids[tcur + src];
            a0 = d.c0[2 * (base + src)]; a1 = d.c0[2 * (base + src) + 1];
            b0 = d.c1[2 * (base + src)]; b1 = d.c1[2 * (base + src) + 1];
        } else {
            const size_t g = (size_t)l * d.cells * k + (size_t)(-src - 1);
            id = id0 + (i - ns);
            a0 = d.g_xy[2 * g]; a1 = d.g_xy[2 * g + 1];
            b0 = d.cand_c1[2 * g]; b1 = d.cand_c1[2 * g + 1];
        }
        d.ids[tnxt + out] = id;
        d.life[tnxt + out] = life;
        d.cam0[2 * (tnxt + out)] = a0; d.cam0[2 * (tnxt + out) + 1] = a1;
        d.cam1[2 * (tnxt + out)] = b0; d.cam1[2 * (tnxt + out) + 1] = b1;
        o.ids[obase + out] = id;
    }
}

// step 9: the published coordinates of the next table's rows, fp64, one thread per row
__global__ void __launch_bounds__(256) k_trk_uv(TrkDev d, const TrkLane* __restrict__ lanes, TrkOut o) {
    const int l = blockIdx.y, r = blockIdx.x * 256 + threadIdx.x;
    const TrkLane& L = lanes[l];
    const size_t t = (size_t)(L.cur ^ 1) * d.n_lanes + L.lane;
    if (r >= min(d.hdr[t].n, d.cap)) return;
    const size_t row = t * d.cap + r;
    double* uv = o.uv + 4 * ((size_t)(o.by_lane ? L.lane : l) * d.cap + r);
    undistort_rect(L.pub0, (double)d.cam0[2 * row], (double)d.cam0[2 * row + 1], uv[0], uv[1]);
    undistort_rect(L.st.cam1, (double)d.cam1[2 * row], (double)d.cam1[2 * row + 1], uv[2], uv[3]);
}

}  // namespace

// ================================================================ C-ABI ====
struct mfe_ctx {
    int device = 0, W = 0, H = 0, nslot = 0, max_level = 0, max_points = 0;
    hipStream_t stream = nullptr;
    std::vector<Pyr> slots;
    std::vector<void*> allocs;
    int kp_cap = 0;           // rows of a set's raster keypoint list
    double* dpts = nullptr;   // mfe_distort: [2][max_points][2]
    // every other call with points: one device block and one pinned host block of the same
    // layout (inputs | work | outputs), grown to the largest call seen
    unsigned char* rs_dev = nullptr;
    unsigned char* rs_host = nullptr;
    size_t rs_cap = 0;
    // what the kernels read their sets from: the slots' Pyr descriptors and the slot
    // numbers 0 .. nslot - 1 on the device (d_slot + s is the slot list of the one image s),
    // and the detection's work areas for work_cap sets (one from mfe_create on)
    Pyr* d_pyr = nullptr;
    int32_t* d_slot = nullptr;
    GridWork work{};
    int work_cap = 0;
    // mfe_upload_many_eq's histograms and tables (msckf_equalize.h), grown to the largest call seen
    unsigned* eq_hist = nullptr;
    uint8_t* eq_lut = nullptr;
    size_t eq_hist_cap = 0, eq_lut_cap = 0;
    // the track tables (msckf_tracks.h), one block of the context's allocations; the host's
    // record of each lane's current table and its row count
    TrkDev trk{};
    std::vector<int> trk_cur, trk_n;
    // the lanes' messages (msckf_handoff.h), in the same block: ids [lane][cap], uv [lane][cap][4]; the
    // row count and the valid flag are the host's record
    long long* msg_ids = nullptr;
    double* msg_uv = nullptr;
    std::vector<int> msg_n;
    std::vector<unsigned char> msg_valid;
    // the lanes' motion records (msckf_standstill.h), in the same block: {n, d2} [lane]; the switch, its
    // quantile and the valid flags are the host's record
    msckf::MotionRec* mot = nullptr;
    std::vector<unsigned char> mot_valid;
    bool mot_on = false;
    double mot_q = 0.5;
};

// msckf_handoff_dev.h: the message tables as msckf_map_add_lost_tracks reads them
bool msckf::mfe_track_messages(const mfe_ctx* c, msckf::TrackMsgView& v) {
    if (!c || !c->trk.ids) return false;
    v.device = c->device;
    v.n_lanes = c->trk.n_lanes;
    v.cap = c->trk.cap;
    v.ids = reinterpret_cast<const int64_t*>(c->msg_ids);
    v.uv = c->msg_uv;
    v.n = c->msg_n.data();
    v.valid = c->msg_valid.data();
    return true;
}

// msckf_standstill_dev.h: the motion records as msckf_zupt_batch_cued reads them
bool msckf::mfe_track_motion(const mfe_ctx* c, msckf::TrackMotionView& v) {
    if (!c || !c->trk.ids) return false;
    v.device = c->device;
    v.n_lanes = c->trk.n_lanes;
    v.rec = c->mot;
    v.valid = c->mot_valid.data();
    return true;
}

namespace {

int dev_alloc(mfe_ctx* c, void** p, size_t bytes) {
    MFE_HIP(hipMalloc(p, bytes ? bytes : 16));
    c->allocs.push_back(*p);
    return 0;
}

int check_n(mfe_ctx* c, int n) {
    if (n < 0 || n > c->max_points) MFE_FAIL(-1, "n = %d outside [0, %d]", n, c->max_points);
    return 0;
}

int grow_scratch(mfe_ctx* c, size_t bytes) {
    if (bytes <= c->rs_cap) return 0;   // nothing is in flight: every call ends with a synchronisation
    if (c->rs_dev) (void)hipFree(c->rs_dev);
    if (c->rs_host) (void)hipHostFree(c->rs_host);
    c->rs_dev = c->rs_host = nullptr;
    c->rs_cap = 0;
    MFE_HIP(hipMalloc((void**)&c->rs_dev, bytes));
    MFE_HIP(hipHostMalloc((void**)&c->rs_host, bytes, hipHostMallocDefault));
    c->rs_cap = bytes;
    return 0;
}

void free_grid_work(mfe_ctx* c) {
    if (c->work.score) (void)hipFree(c->work.score);
    if (c->work.mask) (void)hipFree(c->work.mask);
    if (c->work.rows) (void)hipFree(c->work.rows);
    if (c->work.kp) (void)hipFree(c->work.kp);
    c->work = GridWork{};
    c->work_cap = 0;
}

// the detection's work areas for n_sets sets; their contents do not outlive a call (nothing
// is in flight: every call ends with a synchronisation)
int grow_grid_work(mfe_ctx* c, int n_sets) {
    if (n_sets <= c->work_cap) return 0;
    free_grid_work(c);
    const size_t S = (size_t)n_sets, px = (size_t)c->W * c->H;
    GridWork& g = c->work;
    MFE_HIP(hipMalloc((void**)&g.score, S * px * 2));
    MFE_HIP(hipMalloc((void**)&g.mask, S * px));
    MFE_HIP(hipMalloc((void**)&g.rows, S * 2 * c->H * sizeof(int)));
    MFE_HIP(hipMalloc((void**)&g.kp, S * 3 * c->kp_cap * sizeof(float)));
    g.w = c->W; g.h = c->H; g.kp_cap = c->kp_cap;
    c->work_cap = n_sets;
    return 0;
}

// set_off of a set call: [n_sets + 1], from 0, not decreasing, the total within max_points
int check_set_off(mfe_ctx* c, int n_sets, const int32_t* set_off, const char* name) {
    if (!set_off) MFE_FAIL(-1, "null %s", name);
    if (set_off[0] != 0) MFE_FAIL(-1, "%s[0] = %d, must be 0", name, set_off[0]);
    for (int s = 0; s < n_sets; ++s)
        if (set_off[s + 1] < set_off[s]) MFE_FAIL(-1, "%s is not monotone at set %d", name, s);
    if (set_off[n_sets] > c->max_points)
        MFE_FAIL(-1, "%d points in all sets, above the context's %d", set_off[n_sets], c->max_points);
    return 0;
}

int check_slots(mfe_ctx* c, int n, const int32_t* slots, const char* name) {
    if (!slots) MFE_FAIL(-1, "null %s", name);
    for (int s = 0; s < n; ++s)
        if (slots[s] < 0 || slots[s] >= c->nslot)
            MFE_FAIL(-1, "%s[%d] = %d outside [0, %d)", name, s, slots[s], c->nslot);
    return 0;
}

int check_lk_args(mfe_ctx* c, int win, int max_level, int max_iter) {
    if (win < 3 || win * win > 64 * LK_SLOTS) MFE_FAIL(-1, "window %d outside [3, 16]", win);
    if (max_level < 0 || max_level > c->max_level) MFE_FAIL(-1, "max_level %d outside [0, %d]", max_level, c->max_level);
    if (max_iter < 1) MFE_FAIL(-1, "max_iter must be positive");
    return 0;
}

int check_models(int n_sets, const int32_t* model, const char* name) {
    if (!model) MFE_FAIL(-1, "null %s", name);
    for (int s = 0; s < n_sets; ++s)
        if (model[s] != MFE_RADTAN && model[s] != MFE_EQUIDISTANT)
            MFE_FAIL(-1, "unknown distortion model %d (%s[%d])", model[s], name, s);
    return 0;
}

// byte offsets of a packed block's sections, each aligned to 16
struct Block {
    size_t size = 0;
    size_t add(size_t bytes) {
        const size_t o = size;
        size = (size + bytes + 15) & ~(size_t)15;
        return o;
    }
};

void fill_pt_set(int32_t* pt_set, int n_sets, const int32_t* set_off) {
    for (int s = 0; s < n_sets; ++s)
        for (int i = set_off[s]; i < set_off[s + 1]; ++i) pt_set[i] = s;
}

CamModel make_model(const double* intr, int model, const double* coeffs, const double* R, const double* nk) {
    CamModel m{};
    m.fx = intr[0]; m.fy = intr[1]; m.cx = intr[2]; m.cy = intr[3];
    for (int i = 0; i < 4; ++i) m.k[i] = coeffs ? coeffs[i] : 0.0;
    for (int i = 0; i < 9; ++i) m.R[i] = R ? R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    m.nfx = nk ? nk[0] : 1.0; m.nfy = nk ? nk[1] : 1.0; m.ncx = nk ? nk[2] : 0.0; m.ncy = nk ? nk[3] : 0.0;
    m.model = model;
    return m;
}

}  // namespace

extern "C" {

const char* mfe_last_error(void) { return g_err; }

int mfe_create(int hip_device, int width, int height, int nslot, int max_level, int max_points, mfe_ctx_t** out) {
    if (!out) MFE_FAIL(-1, "null out");
    *out = nullptr;
    if (width < 8 || height < 8 || width > 16384 || height > 16384) MFE_FAIL(-1, "bad image size %dx%d", width, height);
    if (nslot < 1 || nslot > MFE_MAX_SLOTS) MFE_FAIL(-1, "nslot %d outside [1, %d]", nslot, MFE_MAX_SLOTS);
    if (max_level < 0 || max_level >= MAXL) MFE_FAIL(-1, "max_level %d outside [0, %d]", max_level, MAXL - 1);
    if (max_points < 1) MFE_FAIL(-1, "max_points must be positive");
    MFE_HIP(hipSetDevice(hip_device));
    mfe_ctx* c = new mfe_ctx();
    c->device = hip_device; c->W = width; c->H = height; c->nslot = nslot; c->max_level = max_level;
    c->max_points = max_points;
    auto fail = [&](int rc) { mfe_destroy(c); return rc; };
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        set_err("hipStreamCreate failed");
        return fail(-2);
    }
    c->slots.resize(nslot);
    for (int s = 0; s < nslot; ++s) {
        int w = width, h = height;
        for (int l = 0; l < MAXL; ++l) {
            Level& L = c->slots[s].lv[l];
            L.w = w; L.h = h; L.img = nullptr; L.ix = L.iy = nullptr;
            if (l <= max_level) {
                void *a, *b, *d;
                if (dev_alloc(c, &a, (size_t)w * h) || dev_alloc(c, &b, (size_t)w * h * 2) ||
                    dev_alloc(c, &d, (size_t)w * h * 2))
                    return fail(-2);
                L.img = (uint8_t*)a; L.ix = (int16_t*)b; L.iy = (int16_t*)d;
            }
            w = (w + 1) / 2;
            h = (h + 1) / 2;
        }
    }
    std::vector<int32_t> ident(nslot);
    for (int s = 0; s < nslot; ++s) ident[s] = s;
    void *p, *q;
    if (dev_alloc(c, &p, nslot * sizeof(Pyr)) || dev_alloc(c, &q, nslot * sizeof(int32_t)) ||
        hipMemcpy(p, c->slots.data(), nslot * sizeof(Pyr), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(q, ident.data(), nslot * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        set_err("writing the slot tables failed");
        return fail(-2);
    }
    c->d_pyr = (Pyr*)p;
    c->d_slot = (int32_t*)q;
    c->kp_cap = 1 << 16;
    if (grow_grid_work(c, 1)) return fail(-2);
    if (dev_alloc(c, &p, 4 * (size_t)max_points * sizeof(double))) return fail(-2);
    c->dpts = (double*)p;
    *out = c;
    return 0;
}

int mfe_destroy(mfe_ctx_t* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->rs_dev) (void)hipFree(c->rs_dev);
    if (c->rs_host) (void)hipHostFree(c->rs_host);
    free_grid_work(c);
    if (c->eq_hist) (void)hipFree(c->eq_hist);
    if (c->eq_lut) (void)hipFree(c->eq_lut);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

// the pyramids and Scharr derivatives of the n images in the slots dslots (device) names
static void launch_pyramids(mfe_ctx_t* c, const int32_t* dslots, int n) {
    for (int l = 0; l <= c->max_level; ++l) {
        const Level& L = c->slots[0].lv[l];
        const dim3 grid((L.w + 15) / 16, (L.h + 15) / 16, n);
        if (l > 0) hipLaunchKernelGGL(k_pyrdown_sets, grid, dim3(256), 0, c->stream, (const Pyr*)c->d_pyr, dslots, l);
        hipLaunchKernelGGL(k_scharr_sets, grid, dim3(256), 0, c->stream, (const Pyr*)c->d_pyr, dslots, l);
    }
}

// The detection stages up to the raster keypoint lists of n_sets sets, in the work areas:
// the masks are the caller's; totals [n_sets] on the device.
static void launch_detect(mfe_ctx_t* c, const int32_t* dslots, int n_sets, int threshold, int max_kp, int* totals) {
    const GridWork& g = c->work;
    hipStream_t s = c->stream;
    hipLaunchKernelGGL(k_fast_sets, dim3((g.w + 15) / 16, (g.h + 15) / 16, n_sets), dim3(256), 0, s,
                       (const Pyr*)c->d_pyr, dslots, threshold < 0 ? 0 : (threshold > 255 ? 255 : threshold), g.score);
    hipLaunchKernelGGL(k_fast_rows_sets, dim3((g.h + 3) / 4, n_sets), dim3(256), 0, s, g, 0, 0);
    hipLaunchKernelGGL(k_row_scan_sets, dim3(n_sets), dim3(256), 0, s, g, totals);
    hipLaunchKernelGGL(k_fast_rows_sets, dim3((g.h + 3) / 4, n_sets), dim3(256), 0, s, g, 1, max_kp);
}

// The single-image calls: their own checks, then the set call with one set.
int mfe_upload(mfe_ctx_t* c, int slot, const uint8_t* image) {
    if (!c || !image) MFE_FAIL(-1, "null argument");
    const int32_t sl = slot;
    if (check_slots(c, 1, &sl, "slot")) return -1;
    MFE_HIP(hipSetDevice(c->device));
    // straight into level 0 of the slot: one image needs no packing and no scatter
    MFE_HIP(hipMemcpyAsync(c->slots[slot].lv[0].img, image, (size_t)c->W * c->H, hipMemcpyHostToDevice, c->stream));
    launch_pyramids(c, c->d_slot + slot, 1);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int mfe_fast(mfe_ctx_t* c, int slot, int threshold, const uint8_t* mask, int max_kp, float* xy_out,
             float* response_out, int* n_out) {
    if (!c || !n_out) MFE_FAIL(-1, "null argument");
    const int32_t sl = slot;
    if (check_slots(c, 1, &sl, "slot")) return -1;
    if (max_kp < 0 || (max_kp > 0 && (!xy_out || !response_out))) MFE_FAIL(-1, "bad keypoint output");
    MFE_HIP(hipSetDevice(c->device));
    if (int rc = grow_scratch(c, 16)) return rc;
    hipStream_t s = c->stream;
    const GridWork& g = c->work;   // set 0
    const size_t px = (size_t)g.w * g.h;
    // the mask of set 0 holds what the last detection left: all ones unless the caller has one
    if (mask) MFE_HIP(hipMemcpyAsync(g.mask, mask, px, hipMemcpyHostToDevice, s));
    else MFE_HIP(hipMemsetAsync(g.mask, 1, px, s));
    const int cap = std::min(max_kp, g.kp_cap);
    launch_detect(c, c->d_slot + slot, 1, threshold, cap, (int*)c->rs_dev);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(c->rs_host, c->rs_dev, sizeof(int), hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    const int tot = *(const int*)c->rs_host, nw = std::min(tot, cap);
    *n_out = tot;
    if (nw > 0) {
        MFE_HIP(hipMemcpyAsync(xy_out, g.kp, 2 * (size_t)nw * sizeof(float), hipMemcpyDeviceToHost, s));
        MFE_HIP(hipMemcpyAsync(response_out, g.kp + 2 * (size_t)g.kp_cap, (size_t)nw * sizeof(float),
                               hipMemcpyDeviceToHost, s));
        MFE_HIP(hipStreamSynchronize(s));
    }
    return 0;
}

int mfe_lk(mfe_ctx_t* c, int slot_prev, int slot_next, int n, const float* prev_pts, float* next_pts,
           uint8_t* status, int win, int max_level, int max_iter, double eps) {
    if (!c) MFE_FAIL(-1, "null context");
    if (check_n(c, n)) return -1;
    if (n == 0) return 0;
    const int32_t off[2] = {0, n}, sp = slot_prev, sn = slot_next;
    return mfe_lk_sets(c, 1, off, &sp, &sn, prev_pts, next_pts, status, win, max_level, max_iter, eps);
}

int mfe_undistort(mfe_ctx_t* c, int n, const double* pts_in, double* pts_out, const double* intrinsics, int model,
                  const double* coeffs, const double* R, const double* new_intrinsics) {
    if (!c) MFE_FAIL(-1, "null context");
    if (!intrinsics) MFE_FAIL(-1, "null intrinsics");
    if (check_n(c, n)) return -1;
    if (n == 0) return 0;
    static const double zero[4] = {0, 0, 0, 0}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, unit[4] = {1, 1, 0, 0};
    const int32_t off[2] = {0, n}, m = model;
    return mfe_undistort_sets(c, 1, off, pts_in, pts_out, intrinsics, &m, coeffs ? coeffs : zero, R ? R : eye,
                              new_intrinsics ? new_intrinsics : unit);
}

int mfe_distort(mfe_ctx_t* c, int n, const double* pts_in, double* pts_out, const double* intrinsics, int model,
                const double* coeffs) {
    if (!c) MFE_FAIL(-1, "null context");
    if (!intrinsics) MFE_FAIL(-1, "null intrinsics");
    if (check_n(c, n)) return -1;
    if (n == 0) return 0;
    if (!pts_in || !pts_out) MFE_FAIL(-1, "null point array");
    const int32_t m = model;
    if (check_models(1, &m, "model")) return -1;
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    double* din = c->dpts;
    double* dout = c->dpts + 2 * (size_t)c->max_points;
    MFE_HIP(hipMemcpyAsync(din, pts_in, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_distort, dim3((n + 255) / 256), dim3(256), 0, s,
                       make_model(intrinsics, model, coeffs, nullptr, nullptr), n, din, dout);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(pts_out, dout, 2 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    return 0;
}

int mfe_two_point_ransac(mfe_ctx_t* c, int n_sets, const int32_t* set_off, const double* pts_prev,
                         const double* pts_curr, const double* R_p_c, const double* intrinsics, const int32_t* model,
                         const double* coeffs, double inlier_error, int n_hyp, const uint32_t* draws,
                         uint8_t* inlier_out, double* info_out) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0) MFE_FAIL(-1, "n_sets = %d is negative", n_sets);
    if (n_sets == 0) return 0;
    if (!set_off) MFE_FAIL(-1, "null set_off");
    if (set_off[0] != 0) MFE_FAIL(-1, "set_off[0] = %d, must be 0", set_off[0]);
    for (int s = 0; s < n_sets; ++s) {
        const long long ns = (long long)set_off[s + 1] - set_off[s];
        if (ns < 0) MFE_FAIL(-1, "set_off is not monotone at set %d", s);
        if (ns > MFE_RANSAC_MAX_SET_POINTS)
            MFE_FAIL(-1, "set %d has %lld points, above the cap of %d", s, ns, MFE_RANSAC_MAX_SET_POINTS);
    }
    const size_t T = (size_t)set_off[n_sets], S = (size_t)n_sets;
    if (T == 0) return 0;
    if (!pts_prev || !pts_curr || !R_p_c || !intrinsics || !model || !coeffs || !draws || !inlier_out || !info_out)
        MFE_FAIL(-1, "null argument");
    if (n_hyp < 1 || n_hyp > MFE_RANSAC_MAX_HYP) MFE_FAIL(-1, "n_hyp %d outside [1, %d]", n_hyp, MFE_RANSAC_MAX_HYP);
    if (check_models(n_sets, model, "model")) return -1;
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // inputs | work | info, inlier: what comes back
    const size_t H = (size_t)n_hyp, info_bytes = 8 * MFE_RANSAC_INFO_LEN * S;
    Block b;
    const size_t o_prev = b.add(16 * T), o_curr = b.add(16 * T), o_R = b.add(72 * S), o_intr = b.add(32 * S),
                 o_coef = b.add(32 * S), o_off = b.add(4 * (S + 1)), o_model = b.add(4 * S), o_draw = b.add(8 * S * H),
                 in_bytes = b.size, o_work = b.add(32 * T), o_info = b.add(info_bytes), o_inl = b.add(T);
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    memcpy(h + o_prev, pts_prev, 16 * T);
    memcpy(h + o_curr, pts_curr, 16 * T);
    memcpy(h + o_R, R_p_c, 72 * S);
    memcpy(h + o_intr, intrinsics, 32 * S);
    memcpy(h + o_coef, coeffs, 32 * S);
    memcpy(h + o_off, set_off, 4 * (S + 1));
    memcpy(h + o_model, model, 4 * S);
    memcpy(h + o_draw, draws, 8 * S * H);
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st));
    RansacArgs a;
    a.set_off = (const int32_t*)(d + o_off);
    a.pts_prev = (const double*)(d + o_prev);
    a.pts_curr = (const double*)(d + o_curr);
    a.R = (const double*)(d + o_R);
    a.intr = (const double*)(d + o_intr);
    a.coeffs = (const double*)(d + o_coef);
    a.model = (const int32_t*)(d + o_model);
    a.draws = (const uint32_t*)(d + o_draw);
    a.work = (double*)(d + o_work);
    a.info = (double*)(d + o_info);
    a.inlier = d + o_inl;
    a.inlier_error = inlier_error;
    a.n_hyp = n_hyp;
    hipLaunchKernelGGL(k_two_point_ransac, dim3(n_sets), dim3(RS_THREADS), 0, st, a);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_info, d + o_info, b.size - o_info, hipMemcpyDeviceToHost, st));
    MFE_HIP(hipStreamSynchronize(st));
    memcpy(info_out, h + o_info, info_bytes);
    memcpy(inlier_out, h + o_inl, T);
    return 0;
}

int mfe_stereo_match(mfe_ctx_t* c, int slot_cam0, int slot_cam1, int n, const double* cam0_pts,
                     const double* intrinsics0, int model0, const double* coeffs0, const double* intrinsics1,
                     int model1, const double* coeffs1, const double* R_guess, const double* E, int win,
                     int max_level, int max_iter, double eps, double stereo_threshold, float* cam1_pts,
                     uint8_t* inlier, uint8_t* reason) {
    if (!c) MFE_FAIL(-1, "null context");
    if (check_n(c, n)) return -1;
    if (n == 0) return 0;
    const int32_t off[2] = {0, n}, s0 = slot_cam0, s1 = slot_cam1, m0 = model0, m1 = model1;
    return mfe_stereo_match_sets(c, 1, off, &s0, &s1, cam0_pts, intrinsics0, &m0, coeffs0, intrinsics1, &m1, coeffs1,
                                 R_guess, E, &stereo_threshold, win, max_level, max_iter, eps, cam1_pts, inlier, reason);
}

int mfe_fast_grid(mfe_ctx_t* c, int slot, int threshold, int n_occ, const float* occupied, int grid_row,
                  int grid_col, int k, int max_kp, float* xy_out, float* response_out, int32_t* cell_count,
                  int* n_total) {
    const int32_t off[2] = {0, n_occ}, sl = slot;
    return mfe_fast_grid_sets(c, 1, &sl, off, occupied, threshold, grid_row, grid_col, k, max_kp, xy_out,
                              response_out, cell_count, n_total);
}

// ------------------------------------------------- set calls (msckf_lanes.h) --
int mfe_upload_many(mfe_ctx_t* c, int n, const int32_t* slots, const uint8_t* images) {
    if (!c || !images) MFE_FAIL(-1, "null argument");
    if (n < 1 || n > c->nslot) MFE_FAIL(-1, "n = %d outside [1, %d]", n, c->nslot);
    if (check_slots(c, n, slots, "slots")) return -1;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (slots[i] == slots[j]) MFE_FAIL(-1, "slot %d is named twice (images %d and %d)", slots[i], j, i);
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t px = (size_t)c->W * c->H;
    Block b;
    const size_t o_slots = b.add(4 * (size_t)n), o_img = b.add(px * n);
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *hin = c->rs_host, *d = c->rs_dev;
    memcpy(hin + o_slots, slots, 4 * (size_t)n);
    memcpy(hin + o_img, images, px * n);
    MFE_HIP(hipMemcpyAsync(d, hin, b.size, hipMemcpyHostToDevice, s));
    const int32_t* dslots = (const int32_t*)(d + o_slots);
    const int vec = px % 16 == 0 ? 1 : 0;
    const size_t items = vec ? px / 16 : px;
    hipLaunchKernelGGL(k_image_scatter_sets, dim3((unsigned)((items + 255) / 256), 1, n), dim3(256), 0, s,
                       (const Pyr*)c->d_pyr, dslots, (const uint8_t*)(d + o_img), px, vec);
    launch_pyramids(c, dslots, n);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipStreamSynchronize(s));
    return 0;
}

// ------------------------------------------- equalisation (msckf_equalize.h) --
int mfe_upload_many_eq(mfe_ctx_t* c, int n, const int32_t* slots, const uint8_t* images, const int32_t* mode,
                       const float* clip_limit, int tiles_x, int tiles_y) {
    if (!c || !images || !mode) MFE_FAIL(-1, "null argument");
    if (n < 1 || n > c->nslot) MFE_FAIL(-1, "n = %d outside [1, %d]", n, c->nslot);
    if (check_slots(c, n, slots, "slots")) return -1;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (slots[i] == slots[j]) MFE_FAIL(-1, "slot %d is named twice (images %d and %d)", slots[i], j, i);
    if (tiles_x < 1 || tiles_x > MFE_EQ_MAX_TILES) MFE_FAIL(-1, "tiles_x = %d outside [1, %d]", tiles_x, MFE_EQ_MAX_TILES);
    if (tiles_y < 1 || tiles_y > MFE_EQ_MAX_TILES) MFE_FAIL(-1, "tiles_y = %d outside [1, %d]", tiles_y, MFE_EQ_MAX_TILES);
    if (c->W < tiles_x) MFE_FAIL(-1, "tiles_x = %d above the image width %d", tiles_x, c->W);
    if (c->H < tiles_y) MFE_FAIL(-1, "tiles_y = %d above the image height %d", tiles_y, c->H);
    // the tile of the padded image (clahe.cpp: both sides are padded as soon as one does not divide)
    int Wp = c->W, Hp = c->H;
    if (c->W % tiles_x || c->H % tiles_y) {
        Wp += tiles_x - c->W % tiles_x;
        Hp += tiles_y - c->H % tiles_y;
    }
    const int tw = Wp / tiles_x, th = Hp / tiles_y, tiles = tiles_x * tiles_y;
    const double area = (double)tw * th;
    std::vector<int32_t> clip(n, 0);
    for (int i = 0; i < n; ++i) {
        if (mode[i] != MFE_EQ_NONE && mode[i] != MFE_EQ_HIST && mode[i] != MFE_EQ_CLAHE)
            MFE_FAIL(-1, "unknown equalisation mode %d (mode[%d])", mode[i], i);
        if (mode[i] != MFE_EQ_CLAHE) continue;
        if (!clip_limit) MFE_FAIL(-1, "null clip_limit with a CLAHE image (mode[%d])", i);
        if (std::isnan(clip_limit[i])) MFE_FAIL(-1, "clip_limit[%d] is NaN", i);
        if (clip_limit[i] > 0) {   // no bin holds more than area: a limit above it cuts nothing
            const double cl = std::min((double)clip_limit[i] * area / 256.0, area);
            clip[i] = std::max((int32_t)cl, 1);
        }
    }
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t px = (size_t)c->W * c->H;
    const int units = std::max(tiles, EQ_HCH);
    const size_t hist_bytes = (size_t)n * units * 256 * sizeof(unsigned), lut_bytes = (size_t)n * tiles * 256;
    if (hist_bytes > c->eq_hist_cap) {   // nothing is in flight: every call ends with a synchronisation
        if (c->eq_hist) (void)hipFree(c->eq_hist);
        c->eq_hist = nullptr;
        c->eq_hist_cap = 0;
        MFE_HIP(hipMalloc((void**)&c->eq_hist, hist_bytes));
        c->eq_hist_cap = hist_bytes;
    }
    if (lut_bytes > c->eq_lut_cap) {
        if (c->eq_lut) (void)hipFree(c->eq_lut);
        c->eq_lut = nullptr;
        c->eq_lut_cap = 0;
        MFE_HIP(hipMalloc((void**)&c->eq_lut, lut_bytes));
        c->eq_lut_cap = lut_bytes;
    }
    Block b;
    const size_t o_slots = b.add(4 * (size_t)n), o_mode = b.add(4 * (size_t)n), o_clip = b.add(4 * (size_t)n),
                 o_img = b.add(px * n);
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *hin = c->rs_host, *d = c->rs_dev;
    memcpy(hin + o_slots, slots, 4 * (size_t)n);
    memcpy(hin + o_mode, mode, 4 * (size_t)n);
    memcpy(hin + o_clip, clip.data(), 4 * (size_t)n);
    memcpy(hin + o_img, images, px * n);
    MFE_HIP(hipMemcpyAsync(d, hin, b.size, hipMemcpyHostToDevice, s));
    const int32_t* dslots = (const int32_t*)(d + o_slots);
    EqArgs a{};
    a.tab = c->d_pyr; a.slots = dslots; a.mode = (const int32_t*)(d + o_mode); a.clip = (const int32_t*)(d + o_clip);
    a.images = d + o_img; a.hist = c->eq_hist; a.lut = c->eq_lut;
    a.W = c->W; a.H = c->H; a.tiles_x = tiles_x; a.tiles_y = tiles_y; a.tw = tw; a.th = th; a.units = units;
    hipLaunchKernelGGL(k_eq_hist_sets, dim3(units, 1, n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_eq_lut_sets, dim3(tiles, 1, n), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_eq_apply_sets, dim3((tiles_x + 1) * (tiles_y + 1), 1, n), dim3(256), 0, s, a);
    launch_pyramids(c, dslots, n);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipStreamSynchronize(s));
    return 0;
}

int mfe_download(mfe_ctx_t* c, int slot, int level, uint8_t* out) {
    if (!c || !out) MFE_FAIL(-1, "null argument");
    const int32_t sl = slot;
    if (check_slots(c, 1, &sl, "slot")) return -1;
    if (level < 0 || level > c->max_level) MFE_FAIL(-1, "level %d outside [0, %d]", level, c->max_level);
    MFE_HIP(hipSetDevice(c->device));
    const Level& L = c->slots[slot].lv[level];
    MFE_HIP(hipMemcpyAsync(out, L.img, (size_t)L.w * L.h, hipMemcpyDeviceToHost, c->stream));
    MFE_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int mfe_download_deriv(mfe_ctx_t* c, int slot, int level, int16_t* ix, int16_t* iy) {
    if (!c || !ix || !iy) MFE_FAIL(-1, "null argument");
    const int32_t sl = slot;
    if (check_slots(c, 1, &sl, "slot")) return -1;
    if (level < 0 || level > c->max_level) MFE_FAIL(-1, "level %d outside [0, %d]", level, c->max_level);
    MFE_HIP(hipSetDevice(c->device));
    const Level& L = c->slots[slot].lv[level];
    const size_t bytes = (size_t)L.w * L.h * sizeof(int16_t);
    MFE_HIP(hipMemcpyAsync(ix, L.ix, bytes, hipMemcpyDeviceToHost, c->stream));
    MFE_HIP(hipMemcpyAsync(iy, L.iy, bytes, hipMemcpyDeviceToHost, c->stream));
    MFE_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int mfe_lk_sets(mfe_ctx_t* c, int n_sets, const int32_t* set_off, const int32_t* slot_prev,
                const int32_t* slot_next, const float* prev_pts, float* next_pts, uint8_t* status, int win,
                int max_level, int max_iter, double eps) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0 || n_sets > MFE_MAX_SETS) MFE_FAIL(-1, "n_sets = %d outside [0, %d]", n_sets, MFE_MAX_SETS);
    if (n_sets == 0) return 0;
    if (check_set_off(c, n_sets, set_off, "set_off") || check_slots(c, n_sets, slot_prev, "slot_prev") ||
        check_slots(c, n_sets, slot_next, "slot_next") || check_lk_args(c, win, max_level, max_iter))
        return -1;
    const size_t T = (size_t)set_off[n_sets], S = (size_t)n_sets;
    if (T == 0) return 0;
    if (!prev_pts || !next_pts || !status) MFE_FAIL(-1, "null point array");
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    // prev | pt_set | slots | next | status: next ends what goes in and starts what comes back
    Block b;
    const size_t o_prev = b.add(8 * T), o_set = b.add(4 * T), o_slots = b.add(8 * S), o_next = b.add(8 * T),
                 in_bytes = b.size, o_st = b.add(T), out_bytes = b.size - o_next;
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    memcpy(h + o_prev, prev_pts, 8 * T);
    fill_pt_set((int32_t*)(h + o_set), n_sets, set_off);
    for (size_t i = 0; i < S; ++i) {
        ((int32_t*)(h + o_slots))[2 * i] = slot_prev[i];
        ((int32_t*)(h + o_slots))[2 * i + 1] = slot_next[i];
    }
    memcpy(h + o_next, next_pts, 8 * T);
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    LkSetsArgs a;
    a.tab = c->d_pyr;
    a.pt_set = (const int32_t*)(d + o_set);
    a.set_slots = (const int32_t*)(d + o_slots);
    a.prev_pts = (const float*)(d + o_prev);
    a.next_pts = (float*)(d + o_next);
    a.status = d + o_st;
    a.eps = eps;
    a.n = (int)T; a.win = win; a.max_level = max_level; a.max_iter = max_iter;
    hipLaunchKernelGGL(k_lk_sets, dim3((unsigned)T), dim3(64), 0, s, a);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_next, d + o_next, out_bytes, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    memcpy(next_pts, h + o_next, 8 * T);
    memcpy(status, h + o_st, T);
    return 0;
}

int mfe_stereo_match_sets(mfe_ctx_t* c, int n_sets, const int32_t* set_off, const int32_t* slot_cam0,
                          const int32_t* slot_cam1, const double* cam0_pts, const double* intrinsics0,
                          const int32_t* model0, const double* coeffs0, const double* intrinsics1,
                          const int32_t* model1, const double* coeffs1, const double* R_guess, const double* E,
                          const double* stereo_threshold, int win, int max_level, int max_iter, double eps,
                          float* cam1_pts, uint8_t* inlier, uint8_t* reason) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0 || n_sets > MFE_MAX_SETS) MFE_FAIL(-1, "n_sets = %d outside [0, %d]", n_sets, MFE_MAX_SETS);
    if (n_sets == 0) return 0;
    if (check_set_off(c, n_sets, set_off, "set_off") || check_slots(c, n_sets, slot_cam0, "slot_cam0") ||
        check_slots(c, n_sets, slot_cam1, "slot_cam1") || check_lk_args(c, win, max_level, max_iter))
        return -1;
    if (!intrinsics0 || !coeffs0 || !intrinsics1 || !coeffs1 || !R_guess || !E || !stereo_threshold)
        MFE_FAIL(-1, "null camera argument");
    if (check_models(n_sets, model0, "model0") || check_models(n_sets, model1, "model1")) return -1;
    const size_t T = (size_t)set_off[n_sets], S = (size_t)n_sets;
    if (T == 0) return 0;
    if (!cam0_pts || !cam1_pts || !inlier || !reason) MFE_FAIL(-1, "null point array");
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Block b;
    const size_t o_pts = b.add(16 * T), o_tab = b.add(sizeof(StereoSet) * S), o_set = b.add(4 * T), in_bytes = b.size,
                 o_c1 = b.add(8 * T), o_inl = b.add(T), o_rsn = b.add(T), out_bytes = b.size - o_c1;
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    memcpy(h + o_pts, cam0_pts, 16 * T);
    StereoSet* tab = (StereoSet*)(h + o_tab);
    for (size_t i = 0; i < S; ++i) {
        const double *K0 = intrinsics0 + 4 * i, *K1 = intrinsics1 + 4 * i;
        tab[i].cam0 = make_model(K0, model0[i], coeffs0 + 4 * i, R_guess + 9 * i, nullptr);
        tab[i].cam1 = make_model(K1, model1[i], coeffs1 + 4 * i, nullptr, nullptr);
        for (int j = 0; j < 9; ++j) tab[i].E[j] = E[9 * i + j];
        tab[i].epi_thr = stereo_threshold[i] * (4.0 / (K0[0] + K0[1] + K1[0] + K1[1]));
        tab[i].slot0 = slot_cam0[i];
        tab[i].slot1 = slot_cam1[i];
    }
    fill_pt_set((int32_t*)(h + o_set), n_sets, set_off);
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    StereoSetsArgs a;
    a.tab = c->d_pyr;
    a.sets = (const StereoSet*)(d + o_tab);
    a.pt_set = (const int32_t*)(d + o_set);
    a.pts = (const double*)(d + o_pts);
    a.cam1_pts = (float*)(d + o_c1);
    a.inlier = d + o_inl;
    a.reason = d + o_rsn;
    a.eps = eps;
    a.n = (int)T; a.win = win; a.max_level = max_level; a.max_iter = max_iter;
    hipLaunchKernelGGL(k_stereo_match_sets, dim3((unsigned)T), dim3(64), 0, s, a);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_c1, d + o_c1, out_bytes, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    memcpy(cam1_pts, h + o_c1, 8 * T);
    memcpy(inlier, h + o_inl, T);
    memcpy(reason, h + o_rsn, T);
    return 0;
}

int mfe_fast_grid_sets(mfe_ctx_t* c, int n_sets, const int32_t* slots, const int32_t* occ_off,
                       const float* occupied, int threshold, int grid_row, int grid_col, int k, int max_kp,
                       float* xy_out, float* response_out, int32_t* cell_count, int32_t* n_total) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0 || n_sets > MFE_MAX_SETS) MFE_FAIL(-1, "n_sets = %d outside [0, %d]", n_sets, MFE_MAX_SETS);
    if (n_sets == 0) return 0;
    if (!xy_out || !response_out || !cell_count || !n_total) MFE_FAIL(-1, "null argument");
    if (check_slots(c, n_sets, slots, "slots") || check_set_off(c, n_sets, occ_off, "occ_off")) return -1;
    const size_t T = (size_t)occ_off[n_sets], S = (size_t)n_sets;
    if (T > 0 && !occupied) MFE_FAIL(-1, "null occupied points");
    if (c->W < 16 || c->H < 16) MFE_FAIL(-1, "image %dx%d is smaller than 16x16", c->W, c->H);
    if (k < 1 || k > MFE_GRID_MAX_K) MFE_FAIL(-1, "k = %d outside [1, %d]", k, MFE_GRID_MAX_K);
    if (grid_row < 1 || grid_col < 1 || (long long)grid_row * grid_col > MFE_GRID_MAX_CELLS)
        MFE_FAIL(-1, "grid %dx%d outside [1, %d] cells", grid_row, grid_col, MFE_GRID_MAX_CELLS);
    if (max_kp < 1 || max_kp > c->kp_cap) MFE_FAIL(-1, "max_kp = %d outside [1, %d]", max_kp, c->kp_cap);
    MFE_HIP(hipSetDevice(c->device));
    if (int rc = grow_grid_work(c, n_sets)) return rc;
    hipStream_t s = c->stream;
    const int W = c->W, H = c->H;
    const size_t cells = (size_t)grid_row * grid_col, K = (size_t)k;
    Block b;
    const size_t o_occ = b.add(8 * T), o_oset = b.add(4 * T), o_slots = b.add(4 * S), in_bytes = b.size,
                 o_tot = b.add(4 * S), o_cnt = b.add(4 * S * cells), o_resp = b.add(4 * S * cells * K),
                 o_xy = b.add(8 * S * cells * K), out_bytes = b.size - o_tot;
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    if (T > 0) memcpy(h + o_occ, occupied, 8 * T);
    fill_pt_set((int32_t*)(h + o_oset), n_sets, occ_off);
    memcpy(h + o_slots, slots, 4 * S);
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    const GridWork& g = c->work;
    MFE_HIP(hipMemsetAsync(g.mask, 1, S * W * H, s));
    if (T > 0)
        hipLaunchKernelGGL(k_mask_clear_sets, dim3((unsigned)((7 * T + 255) / 256)), dim3(256), 0, s,
                           (const float*)(d + o_occ), (const int32_t*)(d + o_oset), (int)T, g.mask, W, H);
    launch_detect(c, (const int32_t*)(d + o_slots), n_sets, threshold, max_kp, (int*)(d + o_tot));
    GridArgs a;
    a.xy = g.kp; a.resp = g.kp + 2 * (size_t)g.kp_cap; a.total = (const int*)(d + o_tot);
    a.out_xy = (float*)(d + o_xy); a.out_resp = (float*)(d + o_resp); a.cell_count = (int*)(d + o_cnt);
    a.cap = max_kp; a.gh = (H + grid_row - 1) / grid_row; a.gw = (W + grid_col - 1) / grid_col;
    a.grid_col = grid_col; a.k = k;
    hipLaunchKernelGGL(k_grid_select_sets, dim3((unsigned)cells, n_sets), dim3(256), 0, s, a, g.kp_cap);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_tot, d + o_tot, out_bytes, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    const int32_t* tot = (const int32_t*)(h + o_tot);
    int over = -1;
    for (size_t i = 0; i < S; ++i) {
        n_total[i] = tot[i];
        if (tot[i] > max_kp && over < 0) over = (int)i;
    }
    if (over >= 0) MFE_FAIL(-3, "set %d: %d keypoints exceed the capacity of %d", over, tot[over], max_kp);
    const int32_t* cnt = (const int32_t*)(h + o_cnt);
    const float* resp = (const float*)(h + o_resp);
    const float* xy = (const float*)(h + o_xy);
    for (size_t i = 0; i < S; ++i) {
        size_t w = i * cells * K;
        for (size_t cell = 0; cell < cells; ++cell) {
            const size_t q = i * cells + cell, kept = std::min((size_t)cnt[q], K);
            cell_count[q] = cnt[q];
            for (size_t r = 0; r < kept; ++r, ++w) {
                xy_out[2 * w] = xy[2 * (q * K + r)];
                xy_out[2 * w + 1] = xy[2 * (q * K + r) + 1];
                response_out[w] = resp[q * K + r];
            }
        }
    }
    return 0;
}

int mfe_undistort_sets(mfe_ctx_t* c, int n_sets, const int32_t* set_off, const double* pts_in, double* pts_out,
                       const double* intrinsics, const int32_t* model, const double* coeffs, const double* R,
                       const double* new_intrinsics) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0 || n_sets > MFE_MAX_SETS) MFE_FAIL(-1, "n_sets = %d outside [0, %d]", n_sets, MFE_MAX_SETS);
    if (n_sets == 0) return 0;
    if (check_set_off(c, n_sets, set_off, "set_off")) return -1;
    if (!intrinsics || !coeffs || !R || !new_intrinsics) MFE_FAIL(-1, "null camera argument");
    if (check_models(n_sets, model, "model")) return -1;
    const size_t T = (size_t)set_off[n_sets], S = (size_t)n_sets;
    if (T == 0) return 0;
    if (!pts_in || !pts_out) MFE_FAIL(-1, "null point array");
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Block b;
    const size_t o_pts = b.add(16 * T), o_tab = b.add(sizeof(CamModel) * S), o_set = b.add(4 * T), in_bytes = b.size,
                 o_out = b.add(16 * T);
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    memcpy(h + o_pts, pts_in, 16 * T);
    CamModel* tab = (CamModel*)(h + o_tab);
    for (size_t i = 0; i < S; ++i)
        tab[i] = make_model(intrinsics + 4 * i, model[i], coeffs + 4 * i, R + 9 * i, new_intrinsics + 4 * i);
    fill_pt_set((int32_t*)(h + o_set), n_sets, set_off);
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_undistort_sets, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s,
                       (const CamModel*)(d + o_tab), (const int32_t*)(d + o_set), (int)T, (const double*)(d + o_pts),
                       (double*)(d + o_out));
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_out, d + o_out, 16 * T, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    memcpy(pts_out, h + o_out, 16 * T);
    return 0;
}

// ------------------------------------------ device-side tracks (msckf_tracks.h) --
int mfe_tracks_create(mfe_ctx_t* c, int n_lanes, int cap, int grid_row, int grid_col, int grid_min, int grid_max) {
    if (!c) MFE_FAIL(-1, "null context");
    if (c->trk.ids) MFE_FAIL(-1, "the context has its track tables already");
    if (n_lanes < 1 || 3 * (long long)n_lanes > c->nslot)
        MFE_FAIL(-1, "n_lanes = %d outside [1, %d] (three slots per lane)", n_lanes, c->nslot / 3);
    if (grid_row < 1 || grid_col < 1 || (long long)grid_row * grid_col > MFE_GRID_MAX_CELLS)
        MFE_FAIL(-1, "grid %dx%d outside [1, %d] cells", grid_row, grid_col, MFE_GRID_MAX_CELLS);
    if (grid_max < 1 || grid_max > MFE_GRID_MAX_K) MFE_FAIL(-1, "grid_max = %d outside [1, %d]", grid_max, MFE_GRID_MAX_K);
    if (grid_min < 0) MFE_FAIL(-1, "grid_min = %d is negative", grid_min);
    const long long cells = (long long)grid_row * grid_col;
    if (cap > MFE_RANSAC_MAX_SET_POINTS || cap < cells * ((long long)grid_min + grid_max))
        MFE_FAIL(-1, "cap = %d outside [%lld, %d]", cap, cells * ((long long)grid_min + grid_max),
                 MFE_RANSAC_MAX_SET_POINTS);
    MFE_HIP(hipSetDevice(c->device));
    const size_t NL = (size_t)n_lanes, C = (size_t)cap, CK = (size_t)cells * grid_max;
    Block b;
    const size_t o_ids = b.add(8 * 2 * NL * C), o_life = b.add(4 * 2 * NL * C), o_cam0 = b.add(8 * 2 * NL * C),
                 o_cam1 = b.add(8 * 2 * NL * C), o_hdr = b.add(sizeof(TrkHdr) * 2 * NL), o_c0 = b.add(8 * NL * C),
                 o_c1 = b.add(8 * NL * C), o_flag = b.add(NL * C), o_code = b.add(4 * NL * C),
                 o_idx = b.add(4 * 3 * NL * C), o_cnt = b.add(4 * 3 * NL), o_gcnt = b.add(4 * NL * cells),
                 o_gresp = b.add(4 * NL * CK), o_gxy = b.add(8 * NL * CK), o_cc1 = b.add(8 * NL * CK),
                 o_cinl = b.add(NL * CK), o_noff = b.add(4 * NL * cells), o_ooff = b.add(4 * NL * cells),
                 o_rsoff = b.add(4 * (2 * NL + 1)), o_rsprev = b.add(16 * 2 * NL * C), o_rscurr = b.add(16 * 2 * NL * C),
                 o_rswork = b.add(32 * 2 * NL * C), o_rsinfo = b.add(8 * MFE_RANSAC_INFO_LEN * 2 * NL),
                 o_rsinl = b.add(2 * NL * C), o_mids = b.add(8 * NL * C), o_muv = b.add(32 * NL * C),
                 o_mot = b.add(sizeof(msckf::MotionRec) * NL);
    void* p;
    if (int rc = dev_alloc(c, &p, b.size)) return rc;
    MFE_HIP(hipMemset(p, 0, b.size));   // every lane empty, next_id = 0
    unsigned char* m = (unsigned char*)p;
    TrkDev& d = c->trk;
    d.ids = (long long*)(m + o_ids); d.life = (int*)(m + o_life);
    d.cam0 = (float*)(m + o_cam0); d.cam1 = (float*)(m + o_cam1); d.hdr = (TrkHdr*)(m + o_hdr);
    d.c0 = (float*)(m + o_c0); d.c1 = (float*)(m + o_c1); d.flag = m + o_flag; d.code = (int*)(m + o_code);
    d.idx = (int*)(m + o_idx); d.cnt = (int*)(m + o_cnt);
    d.g_cnt = (int*)(m + o_gcnt); d.g_resp = (float*)(m + o_gresp); d.g_xy = (float*)(m + o_gxy);
    d.cand_c1 = (float*)(m + o_cc1); d.cand_inl = m + o_cinl;
    d.new_off = (int*)(m + o_noff); d.out_off = (int*)(m + o_ooff);
    d.rs_off = (int*)(m + o_rsoff); d.rs_prev = (double*)(m + o_rsprev); d.rs_curr = (double*)(m + o_rscurr);
    d.rs_work = (double*)(m + o_rswork); d.rs_info = (double*)(m + o_rsinfo); d.rs_inl = m + o_rsinl;
    d.n_lanes = n_lanes; d.cap = cap; d.cells = (int)cells; d.grid_col = grid_col;
    d.grid_min = grid_min; d.grid_max = grid_max;
    d.gh = (c->H + grid_row - 1) / grid_row; d.gw = (c->W + grid_col - 1) / grid_col;
    c->trk_cur.assign(n_lanes, 0);
    c->trk_n.assign(n_lanes, 0);
    c->msg_ids = (long long*)(m + o_mids);
    c->msg_uv = (double*)(m + o_muv);
    c->msg_n.assign(n_lanes, 0);
    c->msg_valid.assign(n_lanes, 0);
    c->mot = (msckf::MotionRec*)(m + o_mot);
    c->mot_valid.assign(n_lanes, 0);
    return 0;
}

static int check_trk_lane(mfe_ctx_t* c, int lane) {
    if (!c) MFE_FAIL(-1, "null context");
    if (!c->trk.ids) MFE_FAIL(-1, "the context has no track tables (mfe_tracks_create)");
    if (lane < 0 || lane >= c->trk.n_lanes) MFE_FAIL(-1, "lane %d outside [0, %d)", lane, c->trk.n_lanes);
    return 0;
}

int mfe_tracks_put(mfe_ctx_t* c, int lane, int n, const int64_t* ids, const int32_t* lifetimes, const float* cam0,
                   const float* cam1, int64_t next_id) {
    if (check_trk_lane(c, lane)) return -1;
    const TrkDev& d = c->trk;
    if (n < 0 || (long long)n + (long long)d.cells * d.grid_min > d.cap)
        MFE_FAIL(-1, "n = %d outside [0, %lld] (cap %d less grid_min per cell)", n,
                 (long long)d.cap - (long long)d.cells * d.grid_min, d.cap);
    if (n > 0 && (!ids || !lifetimes || !cam0 || !cam1)) MFE_FAIL(-1, "null table array");
    c->msg_valid[lane] = 0;   // the lane's message described the table this call replaces
    c->mot_valid[lane] = 0;   // and so did its motion record (msckf_standstill.h)
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t t = (size_t)c->trk_cur[lane] * d.n_lanes + lane, row = t * d.cap, N = (size_t)n;
    TrkHdr hdr;
    hdr.next_id = next_id; hdr.n = n; hdr.pad = 0;
    if (n > 0) {
        MFE_HIP(hipMemcpyAsync(d.ids + row, ids, 8 * N, hipMemcpyHostToDevice, s));
        MFE_HIP(hipMemcpyAsync(d.life + row, lifetimes, 4 * N, hipMemcpyHostToDevice, s));
        MFE_HIP(hipMemcpyAsync(d.cam0 + 2 * row, cam0, 8 * N, hipMemcpyHostToDevice, s));
        MFE_HIP(hipMemcpyAsync(d.cam1 + 2 * row, cam1, 8 * N, hipMemcpyHostToDevice, s));
    }
    MFE_HIP(hipMemcpyAsync(d.hdr + t, &hdr, sizeof(hdr), hipMemcpyHostToDevice, s));
    MFE_HIP(hipStreamSynchronize(s));
    c->trk_n[lane] = n;
    return 0;
}

int mfe_tracks_get(mfe_ctx_t* c, int lane, int32_t* n, int64_t* ids, int32_t* lifetimes, float* cam0, float* cam1,
                   int64_t* next_id) {
    if (check_trk_lane(c, lane)) return -1;
    if (!n || !ids || !lifetimes || !cam0 || !cam1 || !next_id) MFE_FAIL(-1, "null output");
    const TrkDev& d = c->trk;
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t t = (size_t)c->trk_cur[lane] * d.n_lanes + lane, row = t * d.cap;
    TrkHdr hdr;
    MFE_HIP(hipMemcpyAsync(&hdr, d.hdr + t, sizeof(hdr), hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    if (hdr.n < 0 || hdr.n > d.cap) MFE_FAIL(-2, "lane %d: the device table holds n = %d", lane, hdr.n);
    const size_t N = (size_t)hdr.n;
    if (N > 0) {
        MFE_HIP(hipMemcpyAsync(ids, d.ids + row, 8 * N, hipMemcpyDeviceToHost, s));
        MFE_HIP(hipMemcpyAsync(lifetimes, d.life + row, 4 * N, hipMemcpyDeviceToHost, s));
        MFE_HIP(hipMemcpyAsync(cam0, d.cam0 + 2 * row, 8 * N, hipMemcpyDeviceToHost, s));
        MFE_HIP(hipMemcpyAsync(cam1, d.cam1 + 2 * row, 8 * N, hipMemcpyDeviceToHost, s));
        MFE_HIP(hipStreamSynchronize(s));
    }
    *n = hdr.n;
    *next_id = hdr.next_id;
    return 0;
}

// The one tracking body of mfe_tracks_step and mfe_tracks_step_msg (to_msg: ids and uv go to the
// named lanes' message tables instead of the call's block and ids_out / uv_out, which are not read).
static int tracks_step_body(mfe_ctx_t* c, bool to_msg, int n_lanes, const int32_t* lanes, const int32_t* slot_prev,
                            const int32_t* slot_c0, const int32_t* slot_c1, const double* Hpred,
                            const double* intrinsics0, const int32_t* model0, const double* coeffs0,
                            const double* intrinsics1, const int32_t* model1, const double* coeffs1,
                            const double* R_guess, const double* E, const double* stereo_threshold,
                            const int32_t* ransac, const double* R0, const double* R1, const uint32_t* draws, int win,
                            int max_level, int max_iter, double eps, int threshold, int max_kp, double inlier_error,
                            int n_hyp, int32_t* n_out, int64_t* ids_out, double* uv_out, int32_t* counters,
                            int32_t* n_total, int64_t* next_id_out) {
    if (!c) MFE_FAIL(-1, "null context");
    if (!c->trk.ids) MFE_FAIL(-1, "the context has no track tables (mfe_tracks_create)");
    TrkDev d = c->trk;
    if (n_lanes < 0 || n_lanes > d.n_lanes) MFE_FAIL(-1, "n_lanes = %d outside [0, %d]", n_lanes, d.n_lanes);
    if (n_lanes == 0) return 0;
    if (!lanes || !Hpred || !ransac) MFE_FAIL(-1, "null lane argument");
    if (!n_out || !counters || !n_total || !next_id_out || (!to_msg && (!ids_out || !uv_out)))
        MFE_FAIL(-1, "null output");
    int n_rs = 0;
    for (int l = 0; l < n_lanes; ++l) {
        if (lanes[l] < 0 || lanes[l] >= d.n_lanes) MFE_FAIL(-1, "lanes[%d] = %d outside [0, %d)", l, lanes[l], d.n_lanes);
        for (int j = 0; j < l; ++j)
            if (lanes[j] == lanes[l]) MFE_FAIL(-1, "lane %d is named twice (entries %d and %d)", lanes[l], j, l);
        if ((long long)c->trk_n[lanes[l]] + (long long)d.cells * d.grid_min > d.cap)
            MFE_FAIL(-1, "lane %d: %d rows leave no room for %d new ones (cap %d)", lanes[l], c->trk_n[lanes[l]],
                     d.cells * d.grid_min, d.cap);
        n_rs += ransac[l] ? 1 : 0;
    }
    if (check_slots(c, n_lanes, slot_prev, "slot_prev") || check_slots(c, n_lanes, slot_c0, "slot_c0") ||
        check_slots(c, n_lanes, slot_c1, "slot_c1") || check_lk_args(c, win, max_level, max_iter))
        return -1;
    if (!intrinsics0 || !coeffs0 || !intrinsics1 || !coeffs1 || !R_guess || !E || !stereo_threshold)
        MFE_FAIL(-1, "null camera argument");
    if (check_models(n_lanes, model0, "model0") || check_models(n_lanes, model1, "model1")) return -1;
    if (n_rs > 0) {
        if (!R0 || !R1 || !draws) MFE_FAIL(-1, "null RANSAC argument");
        if (n_hyp < 1 || n_hyp > MFE_RANSAC_MAX_HYP) MFE_FAIL(-1, "n_hyp %d outside [1, %d]", n_hyp, MFE_RANSAC_MAX_HYP);
    }
    if (c->W < 16 || c->H < 16) MFE_FAIL(-1, "image %dx%d is smaller than 16x16", c->W, c->H);
    if (max_kp < 1 || max_kp > c->kp_cap) MFE_FAIL(-1, "max_kp = %d outside [1, %d]", max_kp, c->kp_cap);
    // a lane's message describes its current table, which this call replaces (msckf_handoff.h)
    for (int l = 0; l < n_lanes; ++l) c->msg_valid[lanes[l]] = 0, c->mot_valid[lanes[l]] = 0;
    MFE_HIP(hipSetDevice(c->device));
    if (int rc = grow_grid_work(c, n_lanes)) return rc;
    hipStream_t s = c->stream;
    const int W = c->W, H = c->H;
    const size_t NL = (size_t)n_lanes, NR = (size_t)n_rs, C = (size_t)d.cap, HY = (size_t)(n_rs ? n_hyp : 0);
    Block b;
    const size_t o_lanes = b.add(sizeof(TrkLane) * NL), o_slots = b.add(4 * NL), o_rsl = b.add(4 * NR),
                 o_rsR = b.add(72 * 2 * NR), o_rsK = b.add(32 * 2 * NR), o_rsk = b.add(32 * 2 * NR),
                 o_rsm = b.add(4 * 2 * NR), o_draw = b.add(8 * 2 * NR * HY), in_bytes = b.size,
                 o_n = b.add(4 * NL), o_ctr = b.add(16 * NL), o_tot = b.add(4 * NL), o_next = b.add(8 * NL),
                 head_bytes = b.size - o_n, o_ids = b.add(to_msg ? 0 : 8 * NL * C),
                 o_uv = b.add(to_msg ? 0 : 32 * NL * C), out_bytes = to_msg ? head_bytes : b.size - o_n;
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *dv = c->rs_dev;
    TrkLane* tl = (TrkLane*)(h + o_lanes);
    int32_t* rsl = (int32_t*)(h + o_rsl);
    for (size_t i = 0, r = 0; i < NL; ++i) {
        const double *K0 = intrinsics0 + 4 * i, *K1 = intrinsics1 + 4 * i;
        TrkLane& L = tl[i];
        L.st.cam0 = make_model(K0, model0[i], coeffs0 + 4 * i, R_guess + 9 * i, nullptr);
        L.st.cam1 = make_model(K1, model1[i], coeffs1 + 4 * i, nullptr, nullptr);
        for (int j = 0; j < 9; ++j) L.st.E[j] = E[9 * i + j];
        L.st.epi_thr = stereo_threshold[i] * (4.0 / (K0[0] + K0[1] + K1[0] + K1[1]));
        L.st.slot0 = slot_c0[i];
        L.st.slot1 = slot_c1[i];
        L.pub0 = make_model(K0, model0[i], coeffs0 + 4 * i, nullptr, nullptr);
        for (int j = 0; j < 9; ++j) L.H[j] = Hpred[9 * i + j];
        L.lane = lanes[i];
        L.cur = c->trk_cur[lanes[i]];
        L.slot_prev = slot_prev[i];
        L.rs = -1;
        ((int32_t*)(h + o_slots))[i] = slot_c0[i];
        if (ransac[i]) {   // sets 2 r (cam0, R0, draws[0]) and 2 r + 1 (cam1, R1, draws[1])
            L.rs = (int)r;
            rsl[r] = (int32_t)i;
            memcpy(h + o_rsR + 72 * (2 * r), R0 + 9 * i, 72);
            memcpy(h + o_rsR + 72 * (2 * r + 1), R1 + 9 * i, 72);
            memcpy(h + o_rsK + 32 * (2 * r), K0, 32);
            memcpy(h + o_rsK + 32 * (2 * r + 1), K1, 32);
            memcpy(h + o_rsk + 32 * (2 * r), coeffs0 + 4 * i, 32);
            memcpy(h + o_rsk + 32 * (2 * r + 1), coeffs1 + 4 * i, 32);
            ((int32_t*)(h + o_rsm))[2 * r] = model0[i];
            ((int32_t*)(h + o_rsm))[2 * r + 1] = model1[i];
            memcpy(h + o_draw + 8 * (2 * r) * HY, draws + 4 * i * HY, 16 * HY);
            ++r;
        }
    }
    MFE_HIP(hipMemcpyAsync(dv, h, in_bytes, hipMemcpyHostToDevice, s));
    const TrkLane* dl = (const TrkLane*)(dv + o_lanes);
    const int32_t* drsl = (const int32_t*)(dv + o_rsl);
    const Pyr* tab = c->d_pyr;
    TrkOut o;
    o.n = (int*)(dv + o_n); o.counters = (int*)(dv + o_ctr); o.n_total = (int*)(dv + o_tot);
    o.next_id = (long long*)(dv + o_next);
    o.ids = to_msg ? c->msg_ids : (long long*)(dv + o_ids);
    o.uv = to_msg ? c->msg_uv : (double*)(dv + o_uv);
    o.by_lane = to_msg ? 1 : 0;
    const dim3 rows(d.cap, n_lanes), per256((d.cap + 255) / 256, n_lanes);
    // steps 1-3
    hipLaunchKernelGGL(k_trk_lk, rows, dim3(64), 0, s, d, dl, tab, win, max_level, max_iter, eps);
    hipLaunchKernelGGL(k_trk_compact, dim3(n_lanes), dim3(TRK_THREADS), 0, s, d, dl, 0);
    hipLaunchKernelGGL(k_trk_stereo, rows, dim3(64), 0, s, d, dl, tab, win, max_level, max_iter, eps);
    hipLaunchKernelGGL(k_trk_compact, dim3(n_lanes), dim3(TRK_THREADS), 0, s, d, dl, 1);
    // step 4
    if (n_rs > 0) {
        hipLaunchKernelGGL(k_trk_rs_off, dim3(1), dim3(64), 0, s, d, drsl, n_rs);
        hipLaunchKernelGGL(k_trk_rs_pack, dim3((d.cap + 255) / 256, 2 * n_rs), dim3(256), 0, s, d, dl, drsl);
        RansacArgs a;
        a.set_off = d.rs_off;
        a.pts_prev = d.rs_prev; a.pts_curr = d.rs_curr;
        a.R = (const double*)(dv + o_rsR); a.intr = (const double*)(dv + o_rsK);
        a.coeffs = (const double*)(dv + o_rsk); a.model = (const int32_t*)(dv + o_rsm);
        a.draws = (const uint32_t*)(dv + o_draw);
        a.work = d.rs_work; a.inlier = d.rs_inl; a.info = d.rs_info;
        a.inlier_error = inlier_error; a.n_hyp = n_hyp;
        hipLaunchKernelGGL(k_two_point_ransac, dim3(2 * n_rs), dim3(RS_THREADS), 0, s, a);
    }
    hipLaunchKernelGGL(k_trk_rs_flag, per256, dim3(256), 0, s, d, dl);
    hipLaunchKernelGGL(k_trk_compact, dim3(n_lanes), dim3(TRK_THREADS), 0, s, d, dl, 2);
    if (c->mot_on)   // the motion statistic of step 4's survivors (msckf_standstill.h)
        hipLaunchKernelGGL(k_trk_motion, dim3(n_lanes), dim3(MOT_THREADS), 0, s, d, dl, c->mot_q, c->mot);
    // step 6: the stages of mfe_fast_grid_sets
    const GridWork& g = c->work;
    MFE_HIP(hipMemsetAsync(g.mask, 1, NL * W * H, s));
    hipLaunchKernelGGL(k_trk_mask_clear, dim3((7 * d.cap + 255) / 256, n_lanes), dim3(256), 0, s, d, g.mask, W, H);
    launch_detect(c, (const int32_t*)(dv + o_slots), n_lanes, threshold, max_kp, o.n_total);
    GridArgs ga;
    ga.xy = g.kp; ga.resp = g.kp + 2 * (size_t)g.kp_cap; ga.total = o.n_total;
    ga.out_xy = d.g_xy; ga.out_resp = d.g_resp; ga.cell_count = d.g_cnt;
    ga.cap = max_kp; ga.gh = d.gh; ga.gw = d.gw; ga.grid_col = d.grid_col; ga.k = d.grid_max;
    hipLaunchKernelGGL(k_grid_select_sets, dim3(d.cells, n_lanes), dim3(256), 0, s, ga, g.kp_cap);
    // steps 7-9
    hipLaunchKernelGGL(k_trk_stereo_new, dim3(d.cells * d.grid_max, n_lanes), dim3(64), 0, s, d, dl, tab, win,
                       max_level, max_iter, eps);
    hipLaunchKernelGGL(k_trk_cells, dim3(n_lanes), dim3(TRK_THREADS), 0, s, d, dl, o);
    hipLaunchKernelGGL(k_trk_assemble, dim3(d.cells, n_lanes), dim3(TRK_THREADS), 0, s, d, dl, o);
    hipLaunchKernelGGL(k_trk_uv, per256, dim3(256), 0, s, d, dl, o);
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_n, dv + o_n, out_bytes, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    const int32_t* tot = (const int32_t*)(h + o_tot);
    int over = -1;
    for (size_t i = 0; i < NL; ++i) {
        n_total[i] = tot[i];
        if (tot[i] > max_kp && over < 0) over = (int)i;
    }
    if (over >= 0)   // the next tables hold a truncated frame: they stay the next ones
        MFE_FAIL(-3, "lane %d: %d keypoints exceed the capacity of %d", lanes[over], tot[over], max_kp);
    const int32_t* hn = (const int32_t*)(h + o_n);
    for (size_t i = 0; i < NL; ++i)
        if (hn[i] < 0 || (long long)hn[i] + (long long)d.cells * d.grid_min > d.cap)
            MFE_FAIL(-2, "lane %d: the step left n = %d", lanes[i], hn[i]);
    for (size_t i = 0; i < NL; ++i) {
        const size_t N = (size_t)hn[i];
        n_out[i] = hn[i];
        next_id_out[i] = ((const int64_t*)(h + o_next))[i];
        memcpy(counters + 4 * i, h + o_ctr + 16 * i, 16);
        if (to_msg) {
            c->msg_n[lanes[i]] = hn[i];
            c->msg_valid[lanes[i]] = 1;
        } else {
            memcpy(ids_out + i * C, h + o_ids + 8 * i * C, 8 * N);
            memcpy(uv_out + 4 * i * C, h + o_uv + 32 * i * C, 32 * N);
        }
        c->trk_cur[lanes[i]] ^= 1;
        c->trk_n[lanes[i]] = hn[i];
        if (c->mot_on) c->mot_valid[lanes[i]] = 1;
    }
    return 0;
}

int mfe_tracks_step(mfe_ctx_t* c, int n_lanes, const int32_t* lanes, const int32_t* slot_prev, const int32_t* slot_c0,
                    const int32_t* slot_c1, const double* Hpred, const double* intrinsics0, const int32_t* model0,
                    const double* coeffs0, const double* intrinsics1, const int32_t* model1, const double* coeffs1,
                    const double* R_guess, const double* E, const double* stereo_threshold, const int32_t* ransac,
                    const double* R0, const double* R1, const uint32_t* draws, int win, int max_level, int max_iter,
                    double eps, int threshold, int max_kp, double inlier_error, int n_hyp, int32_t* n_out,
                    int64_t* ids_out, double* uv_out, int32_t* counters, int32_t* n_total, int64_t* next_id_out) {
    return tracks_step_body(c, false, n_lanes, lanes, slot_prev, slot_c0, slot_c1, Hpred, intrinsics0, model0, coeffs0,
                            intrinsics1, model1, coeffs1, R_guess, E, stereo_threshold, ransac, R0, R1, draws, win,
                            max_level, max_iter, eps, threshold, max_kp, inlier_error, n_hyp, n_out, ids_out, uv_out,
                            counters, n_total, next_id_out);
}

// ------------------------------------------ the lanes' messages (msckf_handoff.h) --
int mfe_tracks_step_msg(mfe_ctx_t* c, int n_lanes, const int32_t* lanes, const int32_t* slot_prev,
                        const int32_t* slot_c0, const int32_t* slot_c1, const double* Hpred,
                        const double* intrinsics0, const int32_t* model0, const double* coeffs0,
                        const double* intrinsics1, const int32_t* model1, const double* coeffs1, const double* R_guess,
                        const double* E, const double* stereo_threshold, const int32_t* ransac, const double* R0,
                        const double* R1, const uint32_t* draws, int win, int max_level, int max_iter, double eps,
                        int threshold, int max_kp, double inlier_error, int n_hyp, int32_t* n_out, int32_t* counters,
                        int32_t* n_total, int64_t* next_id_out) {
    return tracks_step_body(c, true, n_lanes, lanes, slot_prev, slot_c0, slot_c1, Hpred, intrinsics0, model0, coeffs0,
                            intrinsics1, model1, coeffs1, R_guess, E, stereo_threshold, ransac, R0, R1, draws, win,
                            max_level, max_iter, eps, threshold, max_kp, inlier_error, n_hyp, n_out, nullptr, nullptr,
                            counters, n_total, next_id_out);
}

int mfe_tracks_msg_put(mfe_ctx_t* c, int lane, int n, const int64_t* ids, const double* uv) {
    if (check_trk_lane(c, lane)) return -1;
    const TrkDev& d = c->trk;
    if (n < 0 || n > d.cap) MFE_FAIL(-1, "n = %d outside [0, %d]", n, d.cap);
    if (n > 0 && (!ids || !uv)) MFE_FAIL(-1, "null message array");
    {
        std::vector<int64_t> srt(ids, ids + n);
        std::sort(srt.begin(), srt.end());
        if (std::adjacent_find(srt.begin(), srt.end()) != srt.end())
            MFE_FAIL(-1, "lane %d: an id is repeated within the message", lane);
    }
    c->msg_valid[lane] = 0;
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t row = (size_t)lane * d.cap;
    if (n > 0) {
        MFE_HIP(hipMemcpyAsync(c->msg_ids + row, ids, 8 * (size_t)n, hipMemcpyHostToDevice, s));
        MFE_HIP(hipMemcpyAsync(c->msg_uv + 4 * row, uv, 32 * (size_t)n, hipMemcpyHostToDevice, s));
    }
    MFE_HIP(hipStreamSynchronize(s));
    c->msg_n[lane] = n;
    c->msg_valid[lane] = 1;
    return 0;
}

int mfe_tracks_msg_get(mfe_ctx_t* c, int lane, int32_t* valid, int32_t* n, int64_t* ids, double* uv) {
    if (check_trk_lane(c, lane)) return -1;
    if (!valid || !n) MFE_FAIL(-1, "null output");
    *valid = c->msg_valid[lane] ? 1 : 0;
    *n = *valid ? c->msg_n[lane] : 0;
    if (*n == 0) return 0;
    if (!ids || !uv) MFE_FAIL(-1, "null output");
    const TrkDev& d = c->trk;
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t row = (size_t)lane * d.cap, N = (size_t)*n;
    MFE_HIP(hipMemcpyAsync(ids, c->msg_ids + row, 8 * N, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipMemcpyAsync(uv, c->msg_uv + 4 * row, 32 * N, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    return 0;
}

// ------------------------------------- the motion statistic (msckf_standstill.h) --
int mfe_motion_sets(mfe_ctx_t* c, int n_sets, const int32_t* set_off, const float* prev, const float* curr, double q,
                    int32_t* n_out, float* d2_out) {
    if (!c) MFE_FAIL(-1, "null context");
    if (n_sets < 0 || n_sets > MFE_MAX_SETS) MFE_FAIL(-1, "n_sets = %d outside [0, %d]", n_sets, MFE_MAX_SETS);
    if (!(q >= 0.0 && q <= 1.0)) MFE_FAIL(-1, "q = %g outside [0, 1]", q);
    if (n_sets == 0) return 0;
    if (check_set_off(c, n_sets, set_off, "set_off")) return -1;
    if (!n_out || !d2_out) MFE_FAIL(-1, "null output");
    const size_t T = (size_t)set_off[n_sets], S = (size_t)n_sets;
    if (T > 0 && (!prev || !curr)) MFE_FAIL(-1, "null point array");
    for (int s = 0; s < n_sets; ++s)
        if (set_off[s + 1] - set_off[s] > MFE_RANSAC_MAX_SET_POINTS)
            MFE_FAIL(-1, "set %d: %d pairs, above %d", s, set_off[s + 1] - set_off[s], MFE_RANSAC_MAX_SET_POINTS);
    for (size_t i = 0; i < 2 * T; ++i)
        if (!std::isfinite(prev[i]) || !std::isfinite(curr[i]))
            MFE_FAIL(-1, "pair %zu: a coordinate is not finite", i / 2);
    MFE_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    Block b;
    const size_t o_off = b.add(4 * (S + 1)), o_prev = b.add(8 * T), o_curr = b.add(8 * T), in_bytes = b.size,
                 o_n = b.add(4 * S), o_d2 = b.add(4 * S), out_bytes = b.size - o_n;
    if (int rc = grow_scratch(c, b.size)) return rc;
    unsigned char *h = c->rs_host, *d = c->rs_dev;
    memcpy(h + o_off, set_off, 4 * (S + 1));
    if (T > 0) {
        memcpy(h + o_prev, prev, 8 * T);
        memcpy(h + o_curr, curr, 8 * T);
    }
    MFE_HIP(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_motion_sets, dim3(n_sets), dim3(MOT_THREADS), 0, s, (const int32_t*)(d + o_off),
                       (const float*)(d + o_prev), (const float*)(d + o_curr), q, (int32_t*)(d + o_n),
                       (float*)(d + o_d2));
    MFE_HIP(hipGetLastError());
    MFE_HIP(hipMemcpyAsync(h + o_n, d + o_n, out_bytes, hipMemcpyDeviceToHost, s));
    MFE_HIP(hipStreamSynchronize(s));
    memcpy(n_out, h + o_n, 4 * S);
    memcpy(d2_out, h + o_d2, 4 * S);
    return 0;
}

int mfe_tracks_motion_enable(mfe_ctx_t* c, int on, double q) {
    if (!c) MFE_FAIL(-1, "null context");
    if (!c->trk.ids) MFE_FAIL(-1, "the context has no track tables (mfe_tracks_create)");
    if (!(q >= 0.0 && q <= 1.0)) MFE_FAIL(-1, "q = %g outside [0, 1]", q);
    c->mot_on = on != 0;
    c->mot_q = q;
    return 0;
}

int mfe_tracks_motion_get(mfe_ctx_t* c, int lane, int32_t* valid, int32_t* n, float* d2) {
    if (check_trk_lane(c, lane)) return -1;
    if (!valid || !n || !d2) MFE_FAIL(-1, "null output");
    *valid = c->mot_valid[lane] ? 1 : 0;
    *n = 0;
    *d2 = std::nanf("");
    MFE_HIP(hipSetDevice(c->device));
    if (!*valid) {
        MFE_HIP(hipStreamSynchronize(c->stream));
        return 0;
    }
    msckf::MotionRec r;
    MFE_HIP(hipMemcpyAsync(&r, c->mot + lane, sizeof(r), hipMemcpyDeviceToHost, c->stream));
    MFE_HIP(hipStreamSynchronize(c->stream));
    *n = r.n;
    *d2 = r.d2;
    return 0;
}

}  // extern "C"
