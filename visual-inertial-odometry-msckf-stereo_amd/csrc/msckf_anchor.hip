// msckf_anchor.hip -- anchor fixes (include/msckf_anchor.h is the specification):
// stereo observations of points with known world positions, gated per anchor,
// stacked, compressed to at most twelve rows and applied as a dense rank-m update
// of the whole covariance, batched over filter slots, in two launches.
//
//   k_anchor_gain   one workgroup per listed filter.  H_l touches columns 0:3 and
//                   12:21 of P only.  One wave takes one anchor per lane (gate,
//                   status, whitened rows), the used ones are compacted in list
//                   order, the Householder QR of the <= 256 x 12 stack runs in
//                   LDS with one thread per row; then as k_aid_gain: P H'^T from
//                   the twelve contiguous ROWS of P, S, chol(S), W = P H'^T L^-T
//                   (workspace), dx = W L^-1 r', the records and the state
//                   correction.  Reads P, writes none of it.
//   k_anchor_apply  one workgroup per 32 x 32 tile of the lower triangle and
//                   listed filter, m from the filter's record (msckf_rank_apply.h).
// The gain reads rows of P that the rank-m update rewrites: with more than one
// workgroup per filter they have to be separate launches.  All arithmetic is fp64
// whatever T; no atomics, no data-dependent order (every reduction has a fixed
// shape), so a repeat gives the same bits.
#include "../../include/msckf_anchor.h"
#include "msckf_anchor_dev.h"
#include "msckf_common.h"
#include "msckf_correct.h"
#include "msckf_rank_apply.h"

namespace msckf {

constexpr int NG_NT = 256;                                   // k_anchor_gain's workgroup; rows of the stack
constexpr int NG_DMAX = 21 + 6 * 128;                        // the largest window (msckf_create)
constexpr int NG_ROWS = (NG_DMAX + NG_NT - 1) / NG_NT;       // rows of P H^T per thread
constexpr int NG_LD = ANC_C + 1;                             // a stacked row: twelve columns of H~ and r~
static_assert(4 * ANC_K == NG_NT, "one thread per stacked row");

// column c of the twelve H touches -> column of P: 0:3, 12:21
__device__ __forceinline__ int anc_col(int c) { return c < 3 ? c : c + 9; }

// Lower Cholesky factor of the 4 x 4 M (its lower triangle) in place; false at a pivot <= 0 or a NaN.
__device__ __forceinline__ bool chol4(double (&M)[4][4]) {
    bool pd = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= M[j][k] * M[j][k];
        if (!(d > 0.0)) pd = false;
        const double l = sqrt(d);
        M[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double s = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= M[i][k] * M[j][k];
            M[i][j] = s / l;
        }
    }
    return pd;
}

template <typename T>
__global__ void __launch_bounds__(NG_NT) k_anchor_gain(DevState<T> st, AnchorDev z, AnchorPrm a, const int* filters,
                                                        const int* off, const msckf_anchor_t* anchors) {
    const int w = blockIdx.x, b = filters[w], tid = threadIdx.x;
    const int D = 21 + 6 * st.ncams[b], ld = st.Dmax;
    const int k0 = off[w], K = off[w + 1] - k0;
    const T* P = st.P + (size_t)b * ld * ld;
    const T* imu = st.imu + (size_t)b * IMU_STRIDE;
    __shared__ double Pcc[ANC_C][ANC_C];             // P[C, C]
    __shared__ double gR[9], gR0[9], gR1[9], gRic[9], gMt[9], gt0[3], gt1[3];   // the geometry; gMt = -R^T [t_ci]x
    __shared__ double A[NG_NT][NG_LD];               // the stack [H~[:, C] | r~]; after the QR its first rows are [H' | r']
    __shared__ double red[NG_NT / 64][NG_LD], piv[NG_LD];
    __shared__ double PH[ANC_C][ANC_M];              // rows C of P H'^T
    __shared__ double S[ANC_M][ANC_M];               // S, then its Cholesky factor (lower)
    __shared__ double y[ANC_M], rd[ANC_M];           // L^-1 r' and the reciprocals of L's diagonal
    __shared__ double dxs[NG_DMAX];
    __shared__ int s_used, s_app;

    if (tid < ANC_C * ANC_C) {
        const int i = tid / ANC_C, j = tid - i * ANC_C;
        Pcc[i][j] = (double)P[(size_t)anc_col(i) * ld + anc_col(j)];
    }
    if (tid == NG_NT - 1) {   // cam0: R0 = R_ic R, t0 = p + R^T t_ci; cam1: R1 = R_cc R0, t1 = t0 - R1^T t_cc
        double q[4], p[3], tci[3], Sk[9], v[3];
        for (int i = 0; i < 4; ++i) q[i] = (double)imu[I_Q + i];
        for (int i = 0; i < 3; ++i) p[i] = (double)imu[I_P + i], tci[i] = (double)imu[I_TCI + i];
        for (int i = 0; i < 9; ++i) gRic[i] = (double)imu[I_RIC + i];
        quat_to_rot(q, gR);
        mat3_mul(gRic, gR, gR0);
        mat3_mul(a.R_cc, gR0, gR1);
        mat3T_vec(gR, tci, v);
        for (int i = 0; i < 3; ++i) gt0[i] = p[i] + v[i];
        mat3T_vec(gR1, a.t_cc, v);
        for (int i = 0; i < 3; ++i) gt1[i] = gt0[i] - v[i];
        skew3(tci, Sk);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) gMt[3 * i + j] = -(gR[i] * Sk[j] + gR[3 + i] * Sk[3 + j] + gR[6 + i] * Sk[6 + j]);
    }
    __syncthreads();

    if (tid < 64) {   // one anchor per lane: the gate, the status and the whitened rows
        int status = MSCKF_ANCHOR_DEPTH;
        double gam = __builtin_nan("");
        double Hw[4][ANC_C], rw[4];
        bool use = false;
        if (tid < K) {
            const msckf_anchor_t& an = anchors[k0 + tid];
            double d[3], pa[3], pb[3];
            for (int i = 0; i < 3; ++i) d[i] = an.p_w[i] - gt0[i];
            mat3_vec(gR0, d, pa);
            for (int i = 0; i < 3; ++i) d[i] = an.p_w[i] - gt1[i];
            mat3_vec(gR1, d, pb);
            if (pa[2] > a.min_depth && pb[2] > a.min_depth) {
                const double ia = 1.0 / pa[2], ib = 1.0 / pb[2];
                const double dz[4][3] = {{ia, 0.0, -pa[0] * ia * ia}, {0.0, ia, -pa[1] * ia * ia},
                                         {ib, 0.0, -pb[0] * ib * ib}, {0.0, ib, -pb[1] * ib * ib}};
                double r[4] = {an.z[0] - pa[0] * ia, an.z[1] - pa[1] * ia, an.z[2] - pb[0] * ib, an.z[3] - pb[1] * ib};
                double X[9], Y[9];
                skew3(pa, X);
                mat3_mul(a.R_cc, X, Y);
                // Hx = [Hth | Hp]: rows 0, 1 through cam0 (dz0 [a]x, -dz0 R0), rows 2, 3 through cam1 (dz1 R_cc [a]x, -dz1 R1)
                double Hth[4][3], Hp[4][3], H[4][ANC_C];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        double s = 0.0, t = 0.0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            s += dz[i][k] * (i < 2 ? X[3 * k + j] : Y[3 * k + j]);
                            t += dz[i][k] * (i < 2 ? gR0[3 * k + j] : gR1[3 * k + j]);
                        }
                        Hth[i][j] = s;
                        Hp[i][j] = -t;
                    }
                // H_l = Hx J in the columns C: theta | p | theta_ext | t_ci
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        double s = 0.0, t = 0.0;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            s += Hth[i][k] * gRic[3 * k + j] + Hp[i][k] * gMt[3 * k + j];
                            t += Hp[i][k] * gR[3 * j + k];
                        }
                        H[i][j] = s;
                        H[i][3 + j] = Hp[i][j];
                        H[i][6 + j] = Hth[i][j];
                        H[i][9 + j] = t;
                    }
                // N_l = obs_var I + Hf Sigma Hf^T (Hf = -Hp), S_l = H_l P H_l^T + N_l: lower triangles
                const double Sg[3][3] = {{an.cov[0], an.cov[1], an.cov[2]}, {an.cov[1], an.cov[3], an.cov[4]},
                                         {an.cov[2], an.cov[4], an.cov[5]}};
                double N[4][4], Sl[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double hs[3], hp[ANC_C];
#pragma unroll
                    for (int j = 0; j < 3; ++j) hs[j] = Hp[i][0] * Sg[0][j] + Hp[i][1] * Sg[1][j] + Hp[i][2] * Sg[2][j];
#pragma unroll
                    for (int c = 0; c < ANC_C; ++c) {
                        double s = 0.0;
#pragma unroll
                        for (int e = 0; e < ANC_C; ++e) s += H[i][e] * Pcc[e][c];
                        hp[c] = s;
                    }
#pragma unroll
                    for (int j = 0; j <= i; ++j) {
                        double s = 0.0;
#pragma unroll
                        for (int c = 0; c < ANC_C; ++c) s += hp[c] * H[j][c];
                        N[i][j] = hs[0] * Hp[j][0] + hs[1] * Hp[j][1] + hs[2] * Hp[j][2] + (i == j ? a.obs_var : 0.0);
                        Sl[i][j] = s + N[i][j];
                    }
                }
                const bool pdn = chol4(N);
                const bool pds = chol4(Sl);
                if (pdn && pds) {
                    double yl[4];
                    gam = 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {   // y = L^-1 r
                        double s = r[i];
#pragma unroll
                        for (int k = 0; k < i; ++k) s -= Sl[i][k] * yl[k];
                        yl[i] = s / Sl[i][i];
                        gam += yl[i] * yl[i];
                    }
                    use = gam < a.chi2;
                    status = use ? MSCKF_ANCHOR_USED : MSCKF_ANCHOR_GATED;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {   // the rows whitened with N_l = C C^T: C^-1 H_l, C^-1 r
                        const double ic = 1.0 / N[i][i];
#pragma unroll
                        for (int c = 0; c < ANC_C; ++c) {
                            double s = H[i][c];
#pragma unroll
                            for (int k = 0; k < i; ++k) s -= N[i][k] * Hw[k][c];
                            Hw[i][c] = s * ic;
                        }
                        double s = r[i];
#pragma unroll
                        for (int k = 0; k < i; ++k) s -= N[i][k] * rw[k];
                        rw[i] = s * ic;
                    }
                } else {
                    status = MSCKF_ANCHOR_NOT_PD;
                }
            }
            z.status[(size_t)b * ANC_K + tid] = (uint8_t)status;
            z.gamma[(size_t)b * ANC_K + tid] = gam;
        }
        // the used anchors in list order: an anchor's place is the count of used lanes below it
        const unsigned long long mask = __ballot(use);
        if (use) {
            const int pos = __popcll(mask & ((1ull << tid) - 1ull));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int c = 0; c < ANC_C; ++c) A[4 * pos + i][c] = Hw[i][c];
                A[4 * pos + i][ANC_C] = rw[i];
            }
        }
        if (tid == 0) s_used = __popcll(mask);
    }
    __syncthreads();
    const int used = s_used, nrows = 4 * used, m = nrows < ANC_M ? nrows : ANC_M;
    if (used == 0 || used < a.min_anchors) {   // nothing to apply: the record only
        if (tid == 0) z.applied[b] = 0, z.used[b] = used, z.rows[b] = m, z.n[b] = K;
        return;
    }

    if (nrows > ANC_M) {   // Householder thin QR of A[0:nrows, 0:12], the reflections applied to r~ too; thread = row
        const int lane = tid & 63, wv = tid >> 6;
        for (int j = 0; j < ANC_C; ++j) {
            const bool act = tid >= j && tid < nrows;
            const double x = act ? A[tid][j] : 0.0;
            if (tid >= j && tid < NG_LD) piv[tid] = A[j][tid];   // row j before its thread rewrites it
            // x^T A[:, k] for k >= j (k = j: |x|^2): thirteen independent butterflies per wave (the columns below j
            // ride along as zeros, so that the trip count is fixed and the chains interleave), then four partials
            double part[NG_LD];
#pragma unroll
            for (int k = 0; k < NG_LD; ++k) part[k] = (act && k >= j) ? x * A[tid][k] : 0.0;
#pragma unroll
            for (int k = 0; k < NG_LD; ++k) part[k] = wave_sum(part[k]);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k < NG_LD; ++k) red[wv][k] = part[k];
            }
            __syncthreads();
            const double nrm = sqrt(((red[0][j] + red[1][j]) + red[2][j]) + red[3][j]);
            if (act && nrm > 0.0) {   // v = x - alpha e_j, alpha = -sign(x_j) |x|; A <- A - beta v (v^T A), beta = 2 / v^T v
                const double x0 = piv[j], alpha = x0 >= 0.0 ? -nrm : nrm;
                const double beta = 1.0 / (nrm * (nrm + fabs(x0)));
                const double vt = tid == j ? x0 - alpha : x;
#pragma unroll
                for (int k = 0; k < NG_LD; ++k) {   // a fixed trip count: the LDS reads of all columns go out together
                    const double sk = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
                    if (k > j) A[tid][k] -= vt * ((sk - alpha * piv[k]) * beta);
                }
                A[tid][j] = tid == j ? alpha : 0.0;
            }
            __syncthreads();
        }
    }

    // P H'^T: row i is H''s mix of P[C, i]; a thread's reads of one row of P are coalesced over i
    double ph[NG_ROWS][ANC_M];
#pragma unroll
    for (int rr = 0; rr < NG_ROWS; ++rr) {
        const int i = tid + rr * NG_NT;
        if (i < D) {
            double p[ANC_C];
#pragma unroll
            for (int c = 0; c < ANC_C; ++c) p[c] = (double)P[(size_t)anc_col(c) * ld + i];
#pragma unroll
            for (int k = 0; k < ANC_M; ++k) {
                double s = 0.0;
                if (k < m) {
#pragma unroll
                    for (int c = 0; c < ANC_C; ++c) s += A[k][c] * p[c];
                }
                ph[rr][k] = s;
            }
            if (i < 3 || (i >= 12 && i < 21)) {   // one of the twelve rows S needs
                const int c = i < 3 ? i : i - 9;
#pragma unroll
                for (int k = 0; k < ANC_M; ++k) PH[c][k] = ph[rr][k];
            }
        }
    }
    __syncthreads();
    if (tid < m * m) {   // S = H' (P H'^T)[C] + I, lower triangle
        const int k = tid / m, l = tid - k * m;
        if (l <= k) {
            double s = 0.0;
            for (int c = 0; c < ANC_C; ++c) s += A[k][c] * PH[c][l];
            S[k][l] = s + (k == l ? 1.0 : 0.0);
        }
    }
    __syncthreads();
    if (tid < 64) {   // chol(S), y = L^-1 r' and the record.  Lane i holds row i in registers; the rows and columns from m on
                      // are the identity's, so that the twelve steps are unrolled for every m.  Column j: lane j's
                      // s is the pivot, the lanes below it finish L[i][j]; y_j follows at once (forward substitution
                      // by columns).  One thread walking S in LDS took 19 of the kernel's 70 us per launch here.
        const int i = tid, ii = i < ANC_M ? i : 0;
        double row[ANC_M];
#pragma unroll
        for (int k = 0; k < ANC_M; ++k) row[k] = (i < m && k <= i) ? S[ii][k] : (i == k ? 1.0 : 0.0);
        double t = i < m ? A[ii][ANC_C] : 0.0;   // r'_i less the columns done
        bool pd = true;
#pragma unroll
        for (int j = 0; j < ANC_M; ++j) {
            double s = row[j];
#pragma unroll
            for (int k = 0; k < j; ++k) s -= row[k] * lane_bcast(row[k], j);
            const double d = lane_bcast(s, j);
            if (!(d > 0.0)) pd = false;
            const double l = sqrt(d), il = 1.0 / l;
            row[j] = i == j ? l : (i > j ? s * il : 0.0);
            const double yj = lane_bcast(t, j) * il;
            if (i > j) t -= row[j] * yj;
            if (i == j) y[j] = yj, rd[j] = il;
        }
        if (i < m) {
#pragma unroll
            for (int k = 0; k < ANC_M; ++k)
                if (k <= i) S[i][k] = row[k];
        }
        if (tid == 0) {
            const int app = pd ? 1 : 0;
            z.applied[b] = app;
            z.used[b] = used;
            z.rows[b] = m;
            z.n[b] = K;
            if (app) z.count[b] += 1;
            s_app = app;
        }
    }
    __syncthreads();
    if (!s_app) return;   // not applied: no byte of the state or of P is written
    double* W = z.W + (size_t)b * ld * ANC_M;
#pragma unroll
    for (int rr = 0; rr < NG_ROWS; ++rr) {
        const int i = tid + rr * NG_NT;
        if (i < D) {   // row i of W = P H'^T L^-T, and dx_i = W_i . y
            double wr[ANC_M], dx = 0.0;
#pragma unroll
            for (int k = 0; k < ANC_M; ++k) {
                double s = 0.0;
                if (k < m) {
                    s = ph[rr][k];
#pragma unroll
                    for (int j = 0; j < k; ++j) s -= wr[j] * S[k][j];
                    s *= rd[k];
                    dx += s * y[k];
                }
                wr[k] = s;
                W[(size_t)i * ANC_M + k] = s;
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

// m is per filter: the row count the gain left in the record.
template <typename T>
__global__ void __launch_bounds__(256) k_anchor_apply(DevState<T> st, AnchorDev z, const int* filters) {
    const Blk3 bk = xcd_blk3();
    const int b = filters[bk.y];
    if (!z.applied[b]) return;
    rank_apply_tile<T, ANC_M>(st, b, z.W + (size_t)b * st.Dmax * ANC_M, z.rows[b], bk.x);
}

template <typename T>
void launch_anchor_gain(hipStream_t s, const DevState<T>& st, const AnchorDev& z, const AnchorPrm& a, int nfilt,
                        const int* filters, const int* off, const msckf_anchor_t* anchors) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL(k_anchor_gain<T>, dim3(nfilt), dim3(NG_NT), 0, s, st, z, a, filters, off, anchors);
}
template <typename T>
void launch_anchor_apply(hipStream_t s, const DevState<T>& st, const AnchorDev& z, int nfilt, const int* filters,
                         int maxD) {
    if (nfilt <= 0) return;
    const int nt = (maxD + RANK_TS - 1) / RANK_TS;
    hipLaunchKernelGGL(k_anchor_apply<T>, dim3(nt * (nt + 1) / 2, nfilt), dim3(256), 0, s, st, z, filters);
}

#define INSTANTIATE(T)                                                                                                \
    template void launch_anchor_gain<T>(hipStream_t, const DevState<T>&, const AnchorDev&, const AnchorPrm&, int,     \
                                        const int*, const int*, const msckf_anchor_t*);                              \
    template void launch_anchor_apply<T>(hipStream_t, const DevState<T>&, const AnchorDev&, int, const int*, int);
INSTANTIATE(float)
INSTANTIATE(double)

}  // namespace msckf
