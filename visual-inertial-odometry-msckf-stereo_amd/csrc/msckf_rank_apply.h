// msckf_rank_apply.h -- one 32 x 32 tile of the dense rank-m covariance update
// P <- P - W W^T, device code shared by its two callers: k_zupt_apply
// (msckf_zupt.hip) and k_aid_apply (msckf_aid.hip).
#pragma once
#include "msckf_common.h"

namespace msckf {

constexpr int RANK_TS = 32;  // the tile edge; the workgroup is 256 threads

// Tile t of the lower triangle (column-major enumeration, colmajor_col) of filter
// b: P_ij <- T(double(P_ij) - sum_k W_ik W_jk), k ascending over m, mirrored into
// the upper triangle through LDS.  W is the filter's [D][MS] block, MS the stride
// of a row of W (m <= MS).  Every value is computed before the workgroup's first
// store: a diagonal tile reads P[max(i,j)][min(i,j)] for both (i,j) and (j,i), so
// both get the same bits, and those are entries other threads of the tile write.
template <typename T, int MS>
__device__ __forceinline__ void rank_apply_tile(const DevState<T>& st, int b, const double* W, int m, int t) {
    const int D = 21 + 6 * st.ncams[b], ld = st.Dmax, nt = (D + RANK_TS - 1) / RANK_TS;
    if (t >= nt * (nt + 1) / 2) return;
    const int tj = colmajor_col(t, nt), ti = tj + t - (tj * nt - tj * (tj - 1) / 2);
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    __shared__ double Wi[RANK_TS][MS], Wj[RANK_TS][MS];
    __shared__ T tile[RANK_TS][RANK_TS + 1];
    for (int e = tid; e < RANK_TS * MS; e += 256) {
        const int row = e / MS, k = e - row * MS;
        const int gi = RANK_TS * ti + row, gj = RANK_TS * tj + row;
        Wi[row][k] = (gi < D && k < m) ? W[(size_t)gi * MS + k] : 0.0;
        Wj[row][k] = (gj < D && k < m) ? W[(size_t)gj * MS + k] : 0.0;
    }
    __syncthreads();
    T* P = st.P + (size_t)b * ld * ld;
    const bool diag = ti == tj;
    const int j = RANK_TS * tj + tx;
    T v[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int li = ty + 8 * rr, i = RANK_TS * ti + li;
        v[rr] = T(0);
        if (i < D && j < D) {
            const int hi = (diag && j > i) ? j : i, lo = (diag && j > i) ? i : j;
            double s = 0.0;
            for (int k = 0; k < m; ++k) s += Wi[li][k] * Wj[tx][k];
            v[rr] = (T)((double)P[(size_t)hi * ld + lo] - s);
        }
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int li = ty + 8 * rr, i = RANK_TS * ti + li;
        if (i < D && j < D) P[(size_t)i * ld + j] = v[rr];
        tile[li][tx] = v[rr];
    }
    if (diag) return;
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {   // the mirror: row (tj, lj) of the upper triangle, contiguous over tx
        const int lj = ty + 8 * rr, jj = RANK_TS * tj + lj, ii = RANK_TS * ti + tx;
        if (jj < D && ii < D) P[(size_t)jj * ld + ii] = tile[tx][lj];
    }
}

}  // namespace msckf
