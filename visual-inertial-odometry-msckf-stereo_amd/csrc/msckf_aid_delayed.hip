// msckf_aid_delayed.hip -- delayed aiding fixes (include/msckf_aid_delayed.h is
// the specification): a fix at a past instant measured on the pose interpolated
// between two cam-state clones, a dense rank-m (1 <= m <= 6, per filter) update
// of the whole covariance, batched over filter slots, in two launches.
//
//   k_aid_delayed_gain   one workgroup per listed filter.  H touches columns
//                        15:21 and the six or twelve of clones s (, s + 1) of P
//                        only; by symmetry P H^T is read from those contiguous
//                        ROWS.  One lane checks the slot pair against the live
//                        window, interpolates (Log / Exp / J_l in double) and
//                        builds the rows of H; then as k_aid_gain: P H^T (D x m),
//                        S, chol(S), the gate, W = P H^T L^-T (workspace), dx = W
//                        L^-1 r, the record and the state correction.  Reads P,
//                        writes none of it.
//   k_aid_delayed_apply  one workgroup per 32 x 32 tile of the lower triangle and
//                        listed filter, m from the filter's record
//                        (msckf_rank_apply.h).
// The gain reads rows of P that the rank-m update rewrites: with more than one
// workgroup per filter they have to be separate launches.  All arithmetic is fp64
// whatever T; no atomics, no data-dependent order.
#include "../../include/msckf_aid_delayed.h"
#include "msckf_aid_delayed_dev.h"
#include "msckf_common.h"
#include "msckf_correct.h"
#include "msckf_rank_apply.h"

namespace msckf {

constexpr int DG_NT = 256;                                   // k_aid_delayed_gain's workgroup
constexpr int DG_DMAX = 21 + 6 * 128;                        // the largest window (msckf_create)
constexpr int DG_ROWS = (DG_DMAX + DG_NT - 1) / DG_NT;       // rows of P H^T per thread
constexpr double DG_SMALL = 1e-4;                            // below this angle: the series forms

// column c of the eighteen H touches -> column of P: 15:21, then clones s and s + 1
__device__ __forceinline__ int adl_col(int c, int s) { return c < 6 ? 15 + c : 15 + 6 * s + c; }

// sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3
__device__ __forceinline__ void so3_abc(double th, double& a, double& b, double& c) {
    if (th < DG_SMALL) {
        const double t2 = th * th;
        a = 1.0 - t2 / 6.0, b = 0.5 - t2 / 24.0, c = 1.0 / 6.0 - t2 / 120.0;
    } else {
        a = sin(th) / th, b = (1.0 - cos(th)) / (th * th), c = (th - sin(th)) / (th * th * th);
    }
}

// M = I + x [phi]x + y [phi]x^2
__device__ __forceinline__ void so3_poly(const double* phi, double x, double y, double* M) {
    double K[9], K2[9];
    skew3(phi, K);
    mat3_mul(K, K, K2);
    for (int e = 0; e < 9; ++e) M[e] = (e % 4 == 0 ? 1.0 : 0.0) + x * K[e] + y * K2[e];
}

__device__ __forceinline__ double norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

template <typename T>
__global__ void __launch_bounds__(DG_NT) k_aid_delayed_gain(DevState<T> st, AidDelayedDev z, msckf_aid_params_t a,
                                                             const int* filters,
                                                             const msckf_aid_delayed_fix_t* fixes) {
    const int w = blockIdx.x, b = filters[w], tid = threadIdx.x;
    const int n = st.ncams[b], D = 21 + 6 * n, ld = st.Dmax;
    const msckf_aid_delayed_fix_t& fx = fixes[w];
    const int rows = fx.rows & 0x3f, m = __popc(rows), s = fx.slot;
    const double lam = fx.lambda;
    const bool two = lam != 0.0;
    if (!(s >= 0 && s < n && (!two || s + 1 < n))) {   // not inside the live window: the record and nothing else
        if (tid == 0) {
            z.applied[b] = 0;
            z.gamma[b] = __builtin_nan("");
            z.rows[b] = rows;
            z.status[b] = MSCKF_AID_DELAYED_BAD_SLOT;
        }
        return;
    }
    const int nc = two ? ADL_C : ADL_C - 6;   // columns of P in play
    const T* P = st.P + (size_t)b * ld * ld;
    const T* imu = st.imu + (size_t)b * IMU_STRIDE;
    __shared__ double Hf[ADL_M][ADL_C], hf[ADL_M];   // all six rows of H (its eighteen columns) and of h(x)
    __shared__ double Hc[ADL_M][ADL_C];              // the kept rows, packed
    __shared__ double r[ADL_M], nz[ADL_M], y[ADL_M];
    __shared__ double PH[ADL_C][ADL_M];              // rows 15:21 and the clones' of P H^T
    __shared__ double S[ADL_M][ADL_M];               // S, then its Cholesky factor (lower)
    __shared__ double dxs[DG_DMAX];
    __shared__ int s_app;

    for (int e = tid; e < ADL_M * ADL_C; e += DG_NT) (&Hf[0][0])[e] = 0.0, (&Hc[0][0])[e] = 0.0;
    __syncthreads();
    if (tid == 0) {   // the measurement model; columns: theta_ext (0:3), t_ci (3:6), clone s (6:12), clone s + 1 (12:18)
        const T* c0 = st.cams + ((size_t)b * st.Nmax + s) * CAM_STRIDE;
        double q[4], R0[9], p0[3], Ric[9], tci[3], Rc[9], pc[3], A0[9], A1[9];
        for (int i = 0; i < 4; ++i) q[i] = (double)c0[C_Q + i];
        for (int i = 0; i < 3; ++i) p0[i] = (double)c0[C_P + i], tci[i] = (double)imu[I_TCI + i];
        for (int i = 0; i < 9; ++i) Ric[i] = (double)imu[I_RIC + i];
        quat_to_rot(q, R0);
        for (int e = 0; e < 9; ++e) Rc[e] = R0[e], A0[e] = (e % 4 == 0 ? 1.0 : 0.0), A1[e] = 0.0;
        for (int i = 0; i < 3; ++i) pc[i] = p0[i];
        if (two) {   // phi = Log(R1 R0^T), R_c = Exp(lam phi) R0, dtheta_c = A0 dtheta_s + A1 dtheta_s+1
            const T* c1 = c0 + CAM_STRIDE;
            double R1[9], M[9], v[3], phi[3], lphi[3], E[9], Jl[9], Ji[9], JiT[9], X[9], Y[9];
            for (int i = 0; i < 4; ++i) q[i] = (double)c1[C_Q + i];
            quat_to_rot(q, R1);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    M[3 * i + j] = R1[3 * i] * R0[3 * j] + R1[3 * i + 1] * R0[3 * j + 1] + R1[3 * i + 2] * R0[3 * j + 2];
            v[0] = 0.5 * (M[7] - M[5]), v[1] = 0.5 * (M[2] - M[6]), v[2] = 0.5 * (M[3] - M[1]);
            const double sn = norm3(v);
            const double k = sn < DG_SMALL ? 1.0 + sn * sn / 6.0 : atan2(sn, 0.5 * (M[0] + M[4] + M[8] - 1.0)) / sn;
            for (int i = 0; i < 3; ++i) phi[i] = k * v[i], lphi[i] = lam * phi[i];
            double ca, cb, cc;
            so3_abc(norm3(lphi), ca, cb, cc);
            so3_poly(lphi, ca, cb, E);
            so3_poly(lphi, cb, cc, Jl);
            const double th = norm3(phi);
            const double cd = th < DG_SMALL ? 1.0 / 12.0 + th * th / 720.0
                                            : 1.0 / (th * th) - (1.0 + cos(th)) / (2.0 * th * sin(th));
            so3_poly(phi, -0.5, cd, Ji);
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) JiT[3 * i + j] = Ji[3 * j + i];
            mat3_mul(Jl, Ji, X);
            mat3_mul(Jl, JiT, Y);
            for (int e = 0; e < 9; ++e) A1[e] = lam * X[e], A0[e] = E[e] - lam * Y[e];
            mat3_mul(E, R0, Rc);
            for (int i = 0; i < 3; ++i) pc[i] = (1.0 - lam) * p0[i] + lam * (double)c1[C_P + i];
        }
        double lt[3], mc[3], u[3], Rtm[3], Sk[9], Gp[9], Gd[9], G0[9], G1[9], RtR[9];
        for (int i = 0; i < 3; ++i) lt[i] = a.lever[i] - tci[i];
        mat3_vec(Ric, lt, mc);
        mat3_vec(Rc, a.dir_w, u);
        mat3T_vec(Rc, mc, Rtm);
        // POS: h = p_c + R_c^T m_c;  Gp = -R_c^T [m_c]x w.r.t. dtheta_c, -Gp at theta_ext, -R_c^T R_ic at t_ci
        skew3(mc, Sk);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                Gp[3 * i + j] = -(Rc[i] * Sk[j] + Rc[3 + i] * Sk[3 + j] + Rc[6 + i] * Sk[6 + j]);
                RtR[3 * i + j] = Rc[i] * Ric[j] + Rc[3 + i] * Ric[3 + j] + Rc[6 + i] * Ric[6 + j];
            }
        mat3_mul(Gp, A0, G0);
        mat3_mul(Gp, A1, G1);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) {
                Hf[i][j] = -Gp[3 * i + j];
                Hf[i][3 + j] = -RtR[3 * i + j];
                Hf[i][6 + j] = G0[3 * i + j];
                Hf[i][12 + j] = G1[3 * i + j];
            }
            Hf[i][9 + i] = 1.0 - lam;
            Hf[i][15 + i] = lam;
            hf[i] = pc[i] + Rtm[i];
        }
        // DIR: h = R_ic^T u, u = R_c d_w;  Gd = R_ic^T [u]x w.r.t. dtheta_c, -Gd at theta_ext
        skew3(u, Sk);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Gd[3 * i + j] = Ric[i] * Sk[j] + Ric[3 + i] * Sk[3 + j] + Ric[6 + i] * Sk[6 + j];
        mat3_mul(Gd, A0, G0);
        mat3_mul(Gd, A1, G1);
        mat3T_vec(Ric, u, hf + 3);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                Hf[3 + i][j] = -Gd[3 * i + j];
                Hf[3 + i][6 + j] = G0[3 * i + j];
                Hf[3 + i][12 + j] = G1[3 * i + j];
            }
    }
    __syncthreads();
    if (tid < ADL_M * ADL_C) {   // pack the kept rows: row g goes to the count of kept rows below it
        const int g = tid / ADL_C, c = tid - g * ADL_C;
        if ((rows >> g) & 1) {
            const int k = __popc(rows & ((1 << g) - 1));
            Hc[k][c] = Hf[g][c];
            if (c == 0) r[k] = fx.z[g] - hf[g], nz[k] = fx.var[g];
        }
    }
    __syncthreads();
    // P H^T: row i is H's mix of P[cols, i]; a thread's reads of one row of P are coalesced over i.  With lam == 0
    // the last six columns are not read (clone s + 1 need not exist) and their H entries are 0.
    const int i0 = 21 + 6 * s;
    double ph[DG_ROWS][ADL_M];
#pragma unroll
    for (int rr = 0; rr < DG_ROWS; ++rr) {
        const int i = tid + rr * DG_NT;
        if (i < D) {
            double p[ADL_C];
#pragma unroll
            for (int c = 0; c < ADL_C; ++c) p[c] = c < nc ? (double)P[(size_t)adl_col(c, s) * ld + i] : 0.0;
#pragma unroll
            for (int k = 0; k < ADL_M; ++k) {
                double sum = 0.0;
                if (k < m) {
#pragma unroll
                    for (int c = 0; c < ADL_C; ++c) sum += Hc[k][c] * p[c];
                }
                ph[rr][k] = sum;
            }
            const int c = (i >= 15 && i < 21) ? i - 15 : (i >= i0 && i < i0 + nc - 6) ? 6 + i - i0 : -1;
            if (c >= 0) {   // one of the rows S needs
#pragma unroll
                for (int k = 0; k < ADL_M; ++k) PH[c][k] = ph[rr][k];
            }
        }
    }
    __syncthreads();
    if (tid < m * m) {   // S = H (P H^T)[its rows] + diag(noise), lower triangle
        const int k = tid / m, l = tid - k * m;
        if (l <= k) {
            double sum = 0.0;
            for (int c = 0; c < nc; ++c) sum += Hc[k][c] * PH[c][l];
            S[k][l] = sum + (k == l ? nz[k] : 0.0);
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
                double sum = S[i][j];
                for (int k = 0; k < j; ++k) sum -= S[i][k] * S[j][k];
                S[i][j] = sum / l;
            }
        }
        double gamma = __builtin_nan("");
        if (pd) {
            gamma = 0.0;
            for (int i = 0; i < m; ++i) {   // y = L^-1 r
                double sum = r[i];
                for (int k = 0; k < i; ++k) sum -= S[i][k] * y[k];
                y[i] = sum / S[i][i];
                gamma += y[i] * y[i];
            }
        }
        const int app = (pd && gamma < a.chi2[m - 1]) ? 1 : 0;
        z.applied[b] = app;
        z.gamma[b] = gamma;
        z.rows[b] = rows;
        z.status[b] = app ? MSCKF_AID_DELAYED_APPLIED : pd ? MSCKF_AID_DELAYED_GATED : MSCKF_AID_DELAYED_NOT_PD;
        if (app) z.count[b] += 1;
        s_app = app;
    }
    __syncthreads();
    if (!s_app) return;   // not applied: no byte of the state or of P is written
    double* W = z.W + (size_t)b * ld * ADL_WS;
#pragma unroll
    for (int rr = 0; rr < DG_ROWS; ++rr) {
        const int i = tid + rr * DG_NT;
        if (i < D) {   // row i of W = P H^T L^-T, and dx_i = W_i . y
            double wr[ADL_M], dx = 0.0;
#pragma unroll
            for (int k = 0; k < ADL_M; ++k) {
                double sum = 0.0;
                if (k < m) {
                    sum = ph[rr][k];
#pragma unroll
                    for (int j = 0; j < k; ++j) sum -= wr[j] * S[k][j];
                    sum /= S[k][k];
                    dx += sum * y[k];
                }
                wr[k] = sum;
                W[(size_t)i * ADL_WS + k] = sum;
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
__global__ void __launch_bounds__(256) k_aid_delayed_apply(DevState<T> st, AidDelayedDev z, const int* filters) {
    const Blk3 bk = xcd_blk3();
    const int b = filters[bk.y];
    if (!z.applied[b]) return;
    rank_apply_tile<T, ADL_WS>(st, b, z.W + (size_t)b * st.Dmax * ADL_WS, __popc(z.rows[b]), bk.x);
}

template <typename T>
void launch_aid_delayed_gain(hipStream_t s, const DevState<T>& st, const AidDelayedDev& z, const msckf_aid_params_t& a,
                             int nfilt, const int* filters, const msckf_aid_delayed_fix_t* fixes) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL(k_aid_delayed_gain<T>, dim3(nfilt), dim3(DG_NT), 0, s, st, z, a, filters, fixes);
}
template <typename T>
void launch_aid_delayed_apply(hipStream_t s, const DevState<T>& st, const AidDelayedDev& z, int nfilt,
                              const int* filters, int maxD) {
    if (nfilt <= 0) return;
    const int nt = (maxD + RANK_TS - 1) / RANK_TS;
    hipLaunchKernelGGL(k_aid_delayed_apply<T>, dim3(nt * (nt + 1) / 2, nfilt), dim3(256), 0, s, st, z, filters);
}

#define INSTANTIATE(T)                                                                                             \
    template void launch_aid_delayed_gain<T>(hipStream_t, const DevState<T>&, const AidDelayedDev&,                \
                                             const msckf_aid_params_t&, int, const int*,                           \
                                             const msckf_aid_delayed_fix_t*);                                      \
    template void launch_aid_delayed_apply<T>(hipStream_t, const DevState<T>&, const AidDelayedDev&, int, const int*, int);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace msckf
