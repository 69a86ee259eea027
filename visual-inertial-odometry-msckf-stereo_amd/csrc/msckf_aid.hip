// msckf_aid.hip -- aiding fixes (include/msckf_aid.h is the specification): a
// dense rank-m (1 <= m <= 12, per filter) update of the whole covariance, batched
// over filter slots, in two launches.
//
//   k_aid_gain   one workgroup per listed filter.  H touches columns 0:3, 6:9 and
//                12:15 of P only; by symmetry P H^T is read from those contiguous
//                ROWS.  Builds the kept rows of H, r and the noise from the
//                filter's own fix, forms P H^T (D x m), S, chol(S), the gate, W =
//                P H^T L^-T (workspace), dx = W L^-1 r, the record and the state
//                correction.  Reads P, writes none of it.
//   k_aid_apply  one workgroup per 32 x 32 tile of the lower triangle and listed
//                filter, m from the filter's record (msckf_rank_apply.h).
// The gain reads rows of P that the rank-m update rewrites: with more than one
// workgroup per filter they have to be separate launches.  All arithmetic is fp64
// whatever T; no atomics, no data-dependent order.
#include "../../include/msckf_aid.h"
#include "msckf_aid_dev.h"
#include "msckf_common.h"
#include "msckf_correct.h"
#include "msckf_rank_apply.h"

namespace msckf {

constexpr int AG_NT = 256;                                   // k_aid_gain's workgroup
constexpr int AG_DMAX = 21 + 6 * 128;                        // the largest window (msckf_create)
constexpr int AG_ROWS = (AG_DMAX + AG_NT - 1) / AG_NT;       // rows of P H^T per thread

// column c of the nine H touches -> column of P: 0:3, 6:9, 12:15
__device__ __forceinline__ int aid_col(int c) { return c + 3 * (c / 3); }

template <typename T>
__global__ void __launch_bounds__(AG_NT) k_aid_gain(DevState<T> st, AidDev z, msckf_aid_params_t a, const int* filters,
                                                     const msckf_aid_fix_t* fixes) {
    const int w = blockIdx.x, b = filters[w], tid = threadIdx.x;
    const int D = 21 + 6 * st.ncams[b], ld = st.Dmax;
    const msckf_aid_fix_t& fx = fixes[w];
    const int rows = fx.rows & 0xfff, m = __popc(rows);
    const T* P = st.P + (size_t)b * ld * ld;
    const T* imu = st.imu + (size_t)b * IMU_STRIDE;
    __shared__ double Hf[AID_M][AID_C], hf[AID_M];   // all twelve rows of H (its nine columns) and of h(x)
    __shared__ double Hc[AID_M][AID_C];              // the kept rows, packed
    __shared__ double r[AID_M], nz[AID_M], y[AID_M];
    __shared__ double PH[AID_C][AID_M];              // rows 0:3, 6:9, 12:15 of P H^T
    __shared__ double S[AID_M][AID_M];               // S, then its Cholesky factor (lower)
    __shared__ double dxs[AG_DMAX];
    __shared__ int s_app;

    for (int e = tid; e < AID_M * AID_C; e += AG_NT) (&Hf[0][0])[e] = 0.0, (&Hc[0][0])[e] = 0.0;
    __syncthreads();
    if (tid == 0) {   // the measurement model: rows POS, VEL, BVEL, DIR; columns theta (0:3), v (3:6), p (6:9)
        double q[4], R[9], p[3], v[3], Rtl[3], Rv[3], Rd[3], Sk[9], M[9];
        for (int i = 0; i < 4; ++i) q[i] = (double)imu[I_Q + i];
        for (int i = 0; i < 3; ++i) p[i] = (double)imu[I_P + i], v[i] = (double)imu[I_V + i];
        quat_to_rot(q, R);
        mat3T_vec(R, a.lever, Rtl);
        mat3_vec(R, v, Rv);
        mat3_vec(R, a.dir_w, Rd);
        const double dt = fx.dt;
        // POS: h = p + R^T l - dt v;  -R^T [l]x, -dt I, I
        skew3(a.lever, Sk);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j)
                Hf[i][j] = -(R[i] * Sk[j] + R[3 + i] * Sk[3 + j] + R[6 + i] * Sk[6 + j]);
            Hf[i][3 + i] = -dt;
            Hf[i][6 + i] = 1.0;
            hf[i] = p[i] + Rtl[i] - dt * v[i];
        }
        // VEL: h = v;  I
        for (int i = 0; i < 3; ++i) Hf[3 + i][3 + i] = 1.0, hf[3 + i] = v[i];
        // BVEL: h = R_body R v;  R_body [R v]x, R_body R
        skew3(Rv, Sk);
        mat3_mul(a.R_body, Sk, M);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Hf[6 + i][j] = M[3 * i + j];
        mat3_mul(a.R_body, R, M);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Hf[6 + i][3 + j] = M[3 * i + j];
        mat3_vec(a.R_body, Rv, hf + 6);
        // DIR: h = R d_w;  [R d_w]x
        skew3(Rd, Sk);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) Hf[9 + i][j] = Sk[3 * i + j];
            hf[9 + i] = Rd[i];
        }
    }
    __syncthreads();
    if (tid < AID_M * AID_C) {   // pack the kept rows: row g goes to the count of kept rows below it
        const int g = tid / AID_C, c = tid - g * AID_C;
        if ((rows >> g) & 1) {
            const int k = __popc(rows & ((1 << g) - 1));
            Hc[k][c] = Hf[g][c];
            if (c == 0) r[k] = fx.z[g] - hf[g], nz[k] = fx.var[g];
        }
    }
    __syncthreads();
    // P H^T: row i is H's mix of P[{0:3, 6:9, 12:15}, i]; a thread's reads of one row of P are coalesced over i
    double ph[AG_ROWS][AID_M];
#pragma unroll
    for (int rr = 0; rr < AG_ROWS; ++rr) {
        const int i = tid + rr * AG_NT;
        if (i < D) {
            double p[AID_C];
#pragma unroll
            for (int c = 0; c < AID_C; ++c) p[c] = (double)P[(size_t)aid_col(c) * ld + i];
#pragma unroll
            for (int k = 0; k < AID_M; ++k) {
                double s = 0.0;
                if (k < m) {
#pragma unroll
                    for (int c = 0; c < AID_C; ++c) s += Hc[k][c] * p[c];
                }
                ph[rr][k] = s;
            }
            if (i < 15 && i % 6 < 3) {   // one of the nine rows S needs
                const int c = i - 3 * (i / 6);
#pragma unroll
                for (int k = 0; k < AID_M; ++k) PH[c][k] = ph[rr][k];
            }
        }
    }
    __syncthreads();
    if (tid < m * m) {   // S = H (P H^T)[the nine rows] + diag(noise), lower triangle
        const int k = tid / m, l = tid - k * m;
        if (l <= k) {
            double s = 0.0;
            for (int c = 0; c < AID_C; ++c) s += Hc[k][c] * PH[c][l];
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
        const int app = (pd && gamma < a.chi2[m - 1]) ? 1 : 0;
        z.applied[b] = app;
        z.gamma[b] = gamma;
        z.rows[b] = rows;
        if (app) z.count[b] += 1;
        s_app = app;
    }
    __syncthreads();
    if (!s_app) return;   // not applied: no byte of the state or of P is written
    double* W = z.W + (size_t)b * ld * AID_M;
#pragma unroll
    for (int rr = 0; rr < AG_ROWS; ++rr) {
        const int i = tid + rr * AG_NT;
        if (i < D) {   // row i of W = P H^T L^-T, and dx_i = W_i . y
            double wr[AID_M], dx = 0.0;
#pragma unroll
            for (int k = 0; k < AID_M; ++k) {
                double s = 0.0;
                if (k < m) {
                    s = ph[rr][k];
#pragma unroll
                    for (int j = 0; j < k; ++j) s -= wr[j] * S[k][j];
                    s /= S[k][k];
                    dx += s * y[k];
                }
                wr[k] = s;
                W[(size_t)i * AID_M + k] = s;
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

// m is per filter: the popcount of the mask the gain left in the record.
template <typename T>
__global__ void __launch_bounds__(256) k_aid_apply(DevState<T> st, AidDev z, const int* filters) {
    const Blk3 bk = xcd_blk3();
    const int b = filters[bk.y];
    if (!z.applied[b]) return;
    rank_apply_tile<T, AID_M>(st, b, z.W + (size_t)b * st.Dmax * AID_M, __popc(z.rows[b]), bk.x);
}

template <typename T>
void launch_aid_gain(hipStream_t s, const DevState<T>& st, const AidDev& z, const msckf_aid_params_t& a, int nfilt,
                     const int* filters, const msckf_aid_fix_t* fixes) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL(k_aid_gain<T>, dim3(nfilt), dim3(AG_NT), 0, s, st, z, a, filters, fixes);
}
template <typename T>
void launch_aid_apply(hipStream_t s, const DevState<T>& st, const AidDev& z, int nfilt, const int* filters, int maxD) {
    if (nfilt <= 0) return;
    const int nt = (maxD + RANK_TS - 1) / RANK_TS;
    hipLaunchKernelGGL(k_aid_apply<T>, dim3(nt * (nt + 1) / 2, nfilt), dim3(256), 0, s, st, z, filters);
}

#define INSTANTIATE(T)                                                                                              \
    template void launch_aid_gain<T>(hipStream_t, const DevState<T>&, const AidDev&, const msckf_aid_params_t&, int, \
                                     const int*, const msckf_aid_fix_t*);                                           \
    template void launch_aid_apply<T>(hipStream_t, const DevState<T>&, const AidDev&, int, const int*, int);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace msckf
