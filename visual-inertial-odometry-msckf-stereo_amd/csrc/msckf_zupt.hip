// msckf_zupt.hip -- the zero-velocity update (include/msckf_zupt.h is the
// specification): a dense rank-m (m = 3, 6, 9) update of the whole covariance,
// batched over filter slots, in two launches.
//
//   k_zupt_gain   one workgroup per listed filter.  H touches columns 0:12 of P
//                 only; by symmetry P H^T = (H P[0:12, :])^T is read from the
//                 contiguous ROWS 0:12.  Forms P H^T (D x m), S, chol(S), the gate,
//                 W = P H^T L^-T (workspace), dx = W L^-1 r, the record and the
//                 state correction.  Reads P, writes none of it.
//   k_zupt_apply  one workgroup per 32 x 32 tile of the lower triangle and listed
//                 filter: P_ij <- T(double(P_ij) - sum_k W_ik W_jk), k ascending,
//                 mirrored into the upper triangle through LDS
//                 (msckf_rank_apply.h, shared with the aiding fixes).
// The gain reads rows 0:12 of P, which the rank-m update rewrites: with more than
// one workgroup per filter they have to be separate launches.  All arithmetic is
// fp64 whatever T; no atomics, no data-dependent order.
//
// k_zupt_gain<T, true> is the cued form (include/msckf_standstill.h): the same
// kernel with the vision cue's status in the decision and three more record words;
// <T, false> is msckf_zupt_batch's: the same body and arithmetic as before the cue, with
// one more kernel argument, placed last and never read, and three more pointers in ZuptDev.
#include "../../include/msckf_standstill.h"
#include "../../include/msckf_zupt.h"
#include "msckf_common.h"
#include "msckf_correct.h"
#include "msckf_rank_apply.h"
#include "msckf_zupt_dev.h"

namespace msckf {

constexpr int ZG_NT = 256;                                   // k_zupt_gain's workgroup
constexpr int ZG_DMAX = 21 + 6 * 128;                        // the largest window (msckf_create)
constexpr int ZG_ROWS = (ZG_DMAX + ZG_NT - 1) / ZG_NT;       // rows of P H^T per thread

template <typename T, bool CUED>
__global__ void __launch_bounds__(ZG_NT) k_zupt_gain(DevState<T> st, ZuptDev z, ZuptArgs a, const int* filters,
                                                      const double* means, ZuptCueArgs q) {
    const int w = blockIdx.x, b = filters[w], tid = threadIdx.x;
    const int D = 21 + 6 * st.ncams[b], ld = st.Dmax, m = a.m;
    const T* P = st.P + (size_t)b * ld * ld;
    const T* imu = st.imu + (size_t)b * IMU_STRIDE;
    __shared__ double Hc[ZUPT_M][12];       // H's columns 0:12
    __shared__ double r[ZUPT_M], nz[ZUPT_M], y[ZUPT_M];
    __shared__ double PH[12][ZUPT_M];       // rows 0:12 of P H^T
    __shared__ double S[ZUPT_M][ZUPT_M];    // S, then its Cholesky factor (lower)
    __shared__ double dxs[ZG_DMAX];
    __shared__ double s_speed;
    __shared__ int s_app;

    for (int e = tid; e < ZUPT_M * 12; e += ZG_NT) (&Hc[0][0])[e] = 0.0;
    __syncthreads();
    if (tid == 0) {   // the measurement: rows VEL, GYRO, ACC, the masked groups dropped
        double q[4], R[9], g[3], Rg[3], v[3];
        for (int i = 0; i < 4; ++i) q[i] = (double)imu[I_Q + i];
        for (int i = 0; i < 3; ++i) g[i] = (double)imu[I_G + i], v[i] = (double)imu[I_V + i];
        quat_to_rot(q, R);
        mat3_vec(R, g, Rg);
        int k = 0;
        if (a.rows & MSCKF_ZUPT_VEL) {
            for (int i = 0; i < 3; ++i) Hc[k + i][6 + i] = 1.0, r[k + i] = -v[i], nz[k + i] = a.noise[0];
            k += 3;
        }
        if (a.rows & MSCKF_ZUPT_GYRO) {
            for (int i = 0; i < 3; ++i) {
                Hc[k + i][3 + i] = 1.0;
                r[k + i] = means[6 * w + i] - (double)imu[I_BG + i];
                nz[k + i] = a.noise[1];
            }
            k += 3;
        }
        if (a.rows & MSCKF_ZUPT_ACC) {
            double Sk[9];
            skew3(Rg, Sk);
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) Hc[k + i][j] = -Sk[3 * i + j];
                Hc[k + i][9 + i] = 1.0;
                r[k + i] = means[6 * w + 3 + i] - (double)imu[I_BA + i] + Rg[i];
                nz[k + i] = a.noise[2];
            }
        }
        s_speed = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    }
    __syncthreads();
    // P H^T: row i is H's mix of P[0:12, i]; a thread's reads of one row of P are coalesced over i
    double ph[ZG_ROWS][ZUPT_M];
#pragma unroll
    for (int rr = 0; rr < ZG_ROWS; ++rr) {
        const int i = tid + rr * ZG_NT;
        if (i < D) {
            double p[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) p[c] = (double)P[(size_t)c * ld + i];
#pragma unroll
            for (int k = 0; k < ZUPT_M; ++k) {
                double s = 0.0;
                if (k < m) {
#pragma unroll
                    for (int c = 0; c < 12; ++c) s += Hc[k][c] * p[c];
                }
                ph[rr][k] = s;
            }
            if (i < 12) {
#pragma unroll
                for (int k = 0; k < ZUPT_M; ++k) PH[i][k] = ph[rr][k];
            }
        }
    }
    __syncthreads();
    if (tid < m * m) {   // S = H (P H^T)[0:12] + diag(noise), lower triangle
        const int k = tid / m, l = tid - k * m;
        if (l <= k) {
            double s = 0.0;
            for (int c = 0; c < 12; ++c) s += Hc[k][c] * PH[c][l];
            S[k][l] = s + (k == l ? nz[k] : 0.0);
        }
    }
    __syncthreads();
    if (tid == 0) {   // chol(S) in place, the gate, the record
        bool pd = true;
        for (int j = 0; j < m && pd; ++j) {
            double d = S[j][j];
            for (int k = 0; k < j; ++k) d -= S[j][k] * S[j][k];
            if (!(d > 0.0)) {
                pd = false;
                break;
            }
            const double l = sqrt(d);
            S[j][j] = l;
            for (int i = j + 1; i < m; ++i) {
                double s = S[i][j];
                for (int k = 0; k < j; ++k) s -= S[i][k] * S[j][k];
                S[i][j] = s / l;
            }
        }
        double gamma = __builtin_nan("");
        if (pd) {
            gamma = 0.0;
            for (int i = 0; i < m; ++i) {   // y = L^-1 r
                double s = r[i];
                for (int k = 0; k < i; ++k) s -= S[i][k] * y[k];
                y[i] = s / S[i][i];
                gamma += y[i] * y[i];
            }
        }
        int app = (pd && gamma < a.chi2 && s_speed <= a.max_speed) ? 1 : 0;
        if constexpr (CUED) {   // the cue's status and the decision rules of msckf_standstill.h
            int cn = -1;
            float cd = __builtin_nanf("");
            if (q.rec) {
                const int ln = q.lane[w];
                if (ln >= 0) cn = q.rec[ln].n, cd = q.rec[ln].d2;
            } else if (q.n[w] >= 0) {
                cn = q.n[w], cd = q.d2[w];
            }
            const int status = (cn < 0 || cn < q.min_tracks) ? MSCKF_CUE_UNKNOWN
                               : ((double)cd <= q.max_px2)   ? MSCKF_CUE_STILL
                                                             : MSCKF_CUE_MOVING;
            const bool imu_ok = app != 0, still = status == MSCKF_CUE_STILL, unk = status == MSCKF_CUE_UNKNOWN;
            const bool fall = q.unknown == MSCKF_CUE_UNKNOWN_IMU;
            if (q.mode == MSCKF_CUE_MODE_VETO)
                app = (imu_ok && (still || (unk && fall))) ? 1 : 0;
            else
                app = ((pd && still) || (imu_ok && (!unk || fall))) ? 1 : 0;
            z.cue[b] = status;
            z.cue_n[b] = cn;
            z.cue_d2[b] = cd;
        }
        z.applied[b] = app;
        z.gamma[b] = gamma;
        if (app) z.count[b] += 1;
        s_app = app;
    }
    __syncthreads();
    if (!s_app) return;   // not applied: no byte of the state or of P is written
    double* W = z.W + (size_t)b * ld * ZUPT_M;
#pragma unroll
    for (int rr = 0; rr < ZG_ROWS; ++rr) {
        const int i = tid + rr * ZG_NT;
        if (i < D) {   // row i of W = P H^T L^-T, and dx_i = W_i . y
            double wr[ZUPT_M], dx = 0.0;
#pragma unroll
            for (int k = 0; k < ZUPT_M; ++k) {
                double s = 0.0;
                if (k < m) {
                    s = ph[rr][k];
#pragma unroll
                    for (int j = 0; j < k; ++j) s -= wr[j] * S[k][j];
                    s /= S[k][k];
                    dx += s * y[k];
                }
                wr[k] = s;
                W[(size_t)i * ZUPT_M + k] = s;
            }
            dxs[i] = dx;
        }
    }
    __syncthreads();
    correct_state(st, b, dxs);
    if (tid == 0) {   // quirk Q5: aliased nulls are the corrected velocity and position
        T* im = st.imu + (size_t)b * IMU_STRIDE;
        if (im[I_ALIAS] != T(0))
            for (int i = 0; i < 3; ++i) im[I_VN + i] = im[I_V + i], im[I_PN + i] = im[I_P + i];
    }
}

// Tile bk.x of the lower triangle of listed filter bk.y (msckf_rank_apply.h).
template <typename T>
__global__ void __launch_bounds__(256) k_zupt_apply(DevState<T> st, ZuptDev z, int m, const int* filters) {
    const Blk3 bk = xcd_blk3();
    const int b = filters[bk.y];
    if (!z.applied[b]) return;
    rank_apply_tile<T, ZUPT_M>(st, b, z.W + (size_t)b * st.Dmax * ZUPT_M, m, bk.x);
}

template <typename T>
void launch_zupt_gain(hipStream_t s, const DevState<T>& st, const ZuptDev& z, const ZuptArgs& a, int nfilt,
                      const int* filters, const double* means) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL((k_zupt_gain<T, false>), dim3(nfilt), dim3(ZG_NT), 0, s, st, z, a, filters, means,
                       ZuptCueArgs{});
}
template <typename T>
void launch_zupt_gain_cued(hipStream_t s, const DevState<T>& st, const ZuptDev& z, const ZuptArgs& a,
                           const ZuptCueArgs& q, int nfilt, const int* filters, const double* means) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL((k_zupt_gain<T, true>), dim3(nfilt), dim3(ZG_NT), 0, s, st, z, a, filters, means, q);
}
template <typename T>
void launch_zupt_apply(hipStream_t s, const DevState<T>& st, const ZuptDev& z, int m, int nfilt, const int* filters,
                       int maxD) {
    if (nfilt <= 0) return;
    const int nt = (maxD + ZUPT_TS - 1) / ZUPT_TS;
    hipLaunchKernelGGL(k_zupt_apply<T>, dim3(nt * (nt + 1) / 2, nfilt), dim3(256), 0, s, st, z, m, filters);
}

#define INSTANTIATE(T)                                                                                           \
    template void launch_zupt_gain<T>(hipStream_t, const DevState<T>&, const ZuptDev&, const ZuptArgs&, int,     \
                                      const int*, const double*);                                                \
    template void launch_zupt_gain_cued<T>(hipStream_t, const DevState<T>&, const ZuptDev&, const ZuptArgs&,     \
                                           const ZuptCueArgs&, int, const int*, const double*);                  \
    template void launch_zupt_apply<T>(hipStream_t, const DevState<T>&, const ZuptDev&, int, int, const int*, int);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace msckf
