// msckf_map.hip -- the filter's feature map kept on the device
// (include/msckf_map.h is the specification, tests/feature_map_ref.py its
// numpy restatement), and the keyframe choice fused into the prune select
// (include/msckf_keyframes.h, tests/keyframe_ref.py), and the landmark archive filled from a lost-form batch
// (include/msckf_odometry.h, tests/landmarks_ref.py).  One workgroup of 256 threads (four wavefronts) per named
// filter; a call reads a filter's current table and writes its other one.
//
// Rules (those of the front-end's k_trk_* kernels): fixed-stride [filter][cap]
// tables, row counts read from the call's header on the device, order-preserving
// compactions by ballot rank with the wave counts through LDS in wave order, the
// id match against the table's ids staged in LDS, no atomics and no
// data-dependent ordering -- a repeat gives the same bits.
#include <hip/hip_runtime.h>

#include "msckf_common.h"
#include "msckf_map_dev.h"

namespace msckf {

namespace {

constexpr int MAP_BLOCK = 256, MAP_WAVES = MAP_BLOCK / 64;

// Exclusive rank of `flag` among the workgroup's threads in thread order and
// the workgroup's total.  Every thread calls it (the callers' loops have
// uniform trip counts).
__device__ inline int block_rank(bool flag, int* s_wcnt, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int k = 0; k < MAP_WAVES; ++k) {
        const int cnt = s_wcnt[k];
        if (k < wave) base += cnt;
        total += cnt;
    }
    __syncthreads();
    return base + __popcll(bal & ((1ull << lane) - 1ull));
}

__device__ inline bool bit_of(unsigned long long m0, unsigned long long m1, int slot) {
    return (((slot < 64 ? m0 : m1) >> (slot & 63)) & 1ull) != 0;
}
// number of set bits of (r0, r1) below `slot`
__device__ inline int bits_below(unsigned long long r0, unsigned long long r1, int slot) {
    if (slot < 64) return __popcll(r0 & ((1ull << slot) - 1ull));
    return __popcll(r0) + __popcll(r1 & ((1ull << (slot - 64)) - 1ull));
}

struct MapLds {
    long long* ids;   // [cap]
    int* hit;         // [cap]  add_lost: 1 + message row of the row's new observation (0: none)
    int* dst;         // [cap]  row of the next table (-1: dropped); commit: entry of a row (-1: none)
    int* wcnt;        // [MAP_WAVES]
};
__device__ inline MapLds map_lds(unsigned char* raw, int cap) {
    MapLds l;
    l.ids = reinterpret_cast<long long*>(raw);
    l.hit = reinterpret_cast<int*>(raw + (size_t)cap * 8);
    l.dst = l.hit + cap;
    l.wcnt = l.dst + cap;
    return l;
}

// msckf_map_add_lost, steps 1-6 of the header.
__global__ void __launch_bounds__(MAP_BLOCK)
k_map_add_lost(MapDev m, const int* __restrict__ hdr, const int64_t* __restrict__ msg_ids,
               const double* __restrict__ msg_z, int* __restrict__ out, int64_t* __restrict__ desc_id,
               int* __restrict__ desc_info) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const MapLds L = map_lds(s_raw, m.cap);
    const int w = blockIdx.x, tid = threadIdx.x, cap = m.cap, N4 = m.Nmax * 4;
    const int* h = hdr + w * MAP_HDR;
    const int f = h[0], n = h[1], cur = h[2], snew = h[3], m0 = h[4], nm = h[5] - h[4], ds = h[6];
    const MapTab src = m.t[cur], dstt = m.t[cur ^ 1];
    const size_t fb = (size_t)f * cap;
    for (int i = tid; i < cap; i += MAP_BLOCK) {
        L.ids[i] = i < n ? src.ids[fb + i] : 0;
        L.hit[i] = 0;
        L.dst[i] = -1;
    }
    __syncthreads();
    // 1-2: match the message against the table, new ids ranked in message order
    int nnew = 0;
    for (int j0 = 0; j0 < nm; j0 += MAP_BLOCK) {
        const int j = j0 + tid;
        const bool active = j < nm;
        int r = -1;
        if (active) {
            const long long id = msg_ids[m0 + j];
            for (int i = 0; i < n; ++i)
                if (L.ids[i] == id) {
                    r = i;
                    break;
                }
            if (r >= 0) L.hit[r] = j + 1;   // ids of a message and of a table are distinct: one writer
        }
        int tot;
        const int rank = block_rank(active && r < 0, L.wcnt, tot);
        if (active && r < 0) {
            const int pos = n + nnew + rank;
            if (pos < cap) {
                L.hit[pos] = j + 1;
                L.ids[pos] = msg_ids[m0 + j];
            }
        }
        nnew += tot;
    }
    __syncthreads();
    const int tracked = nm - nnew, ntot = n + nnew;
    if (ntot > cap) {   // overflow: nothing of the next table is meaningful, the host does not swap
        if (tid == 0) {
            out[w * MAP_OUT + 0] = tracked;
            out[w * MAP_OUT + 1] = ntot;
            out[w * MAP_OUT + 2] = 0;
            out[w * MAP_OUT + 3] = 1;
        }
        return;
    }
    // 3-5: classify, rank the rows that stay and the candidates, write the rows that stay
    int nkeep = 0, ncand = 0;
    for (int i0 = 0; i0 < ntot; i0 += MAP_BLOCK) {
        const int i = i0 + tid;
        const bool active = i < ntot, old = i < n;
        unsigned long long k0 = 0, k1 = 0;
        bool keep = false, cand = false;
        int M = 0;
        if (active) {
            if (old) {
                k0 = src.mask[(fb + i) * 2];
                k1 = src.mask[(fb + i) * 2 + 1];
                M = __popcll(k0) + __popcll(k1);
                keep = L.hit[i] != 0 || bit_of(k0, k1, snew);
                cand = !keep && M >= 3;
            } else {
                keep = true;
            }
        }
        int tot;
        const int rk = block_rank(keep, L.wcnt, tot);
        if (keep) {
            const int d = nkeep + rk;   // d <= i < cap
            L.dst[i] = d;
            if (snew < 64) k0 |= 1ull << snew; else k1 |= 1ull << (snew - 64);
            dstt.ids[fb + d] = L.ids[i];
            dstt.mask[(fb + d) * 2] = k0;
            dstt.mask[(fb + d) * 2 + 1] = k1;
            for (int c = 0; c < 3; ++c) dstt.pw[(fb + d) * 3 + c] = old ? src.pw[(fb + i) * 3 + c] : 0.0;
            dstt.init[fb + d] = old ? src.init[fb + i] : 0;
            const int mj = L.hit[i];
            if (mj)
                for (int c = 0; c < 4; ++c)
                    dstt.z[(fb + d) * N4 + snew * 4 + c] = msg_z[(size_t)(m0 + mj - 1) * 4 + c];
        }
        nkeep += tot;
        const int rc = block_rank(cand, L.wcnt, tot);
        if (cand) {
            const int p = ncand + rc;   // p <= i < n <= ds
            desc_id[(size_t)w * ds + p] = L.ids[i];
            int* di = desc_info + ((size_t)w * ds + p) * MAP_INFO;
            di[0] = M;
            di[1] = 0;
            di[2] = src.init[fb + i] ? 1 : 0;
            di[3] = i;
        }
        ncand += tot;
    }
    __syncthreads();
    // 6: the kept rows' earlier observations
    for (int e = tid; e < n * N4; e += MAP_BLOCK) {
        const int i = e / N4, k = e - i * N4, slot = k >> 2, d = L.dst[i];
        if (d < 0) continue;
        if (slot == snew && L.hit[i]) continue;   // written from the message above
        if (bit_of(src.mask[(fb + i) * 2], src.mask[(fb + i) * 2 + 1], slot))
            dstt.z[(fb + d) * N4 + k] = src.z[(fb + i) * N4 + k];
    }
    if (tid == 0) {
        out[w * MAP_OUT + 0] = tracked;
        out[w * MAP_OUT + 1] = nkeep;
        out[w * MAP_OUT + 2] = ncand;
        out[w * MAP_OUT + 3] = 0;
    }
}

// The body of a prune select, shared by msckf_map_prune_select and
// msckf_keyframe_select: the rows of the table read into the other one with the
// single involved observations dropped, the involved rows into the descriptor;
// (r0, r1) = the removed slots.  No row moves.  Every thread of the workgroup
// calls it; returns the number of involved rows.
__device__ inline int select_body(const MapDev& m, const int* __restrict__ h, int w, unsigned long long r0,
                                  unsigned long long r1, int* s_wcnt, int64_t* __restrict__ desc_id,
                                  int* __restrict__ desc_info) {
    const int tid = threadIdx.x, cap = m.cap, N4 = m.Nmax * 4;
    const int f = h[0], n = h[1], cur = h[2], ds = h[6];
    const MapTab src = m.t[cur], dstt = m.t[cur ^ 1];
    const size_t fb = (size_t)f * cap;
    int ninv = 0;
    for (int i0 = 0; i0 < n; i0 += MAP_BLOCK) {
        const int i = i0 + tid;
        const bool active = i < n;
        bool involved = false;
        int M = 0, k = 0;
        if (active) {
            unsigned long long k0 = src.mask[(fb + i) * 2], k1 = src.mask[(fb + i) * 2 + 1];
            M = __popcll(k0) + __popcll(k1);
            k = __popcll(k0 & r0) + __popcll(k1 & r1);
            involved = k >= 2;
            if (k == 1) {
                k0 &= ~r0;
                k1 &= ~r1;
            }
            dstt.ids[fb + i] = src.ids[fb + i];
            dstt.mask[(fb + i) * 2] = k0;
            dstt.mask[(fb + i) * 2 + 1] = k1;
            for (int c = 0; c < 3; ++c) dstt.pw[(fb + i) * 3 + c] = src.pw[(fb + i) * 3 + c];
            dstt.init[fb + i] = src.init[fb + i];
        }
        int tot;
        const int rk = block_rank(involved, s_wcnt, tot);
        if (involved) {
            const int p = ninv + rk;   // p <= i < n <= ds
            desc_id[(size_t)w * ds + p] = src.ids[fb + i];
            int* di = desc_info + ((size_t)w * ds + p) * MAP_INFO;
            di[0] = M;
            di[1] = k;
            di[2] = src.init[fb + i] ? 1 : 0;
            di[3] = i;
        }
        ninv += tot;
    }
    for (int e = tid; e < n * N4; e += MAP_BLOCK) {
        const int i = e / N4, kk = e - i * N4, slot = kk >> 2;
        unsigned long long k0 = src.mask[(fb + i) * 2], k1 = src.mask[(fb + i) * 2 + 1];
        if (__popcll(k0 & r0) + __popcll(k1 & r1) == 1) {
            k0 &= ~r0;
            k1 &= ~r1;
        }
        if (bit_of(k0, k1, slot)) dstt.z[(fb + i) * N4 + kk] = src.z[(fb + i) * N4 + kk];
    }
    return ninv;
}

// msckf_map_prune_select
__global__ void __launch_bounds__(MAP_BLOCK)
k_map_prune_select(MapDev m, const int* __restrict__ hdr, const unsigned long long* __restrict__ rm,
                   int* __restrict__ out, int64_t* __restrict__ desc_id, int* __restrict__ desc_info) {
    __shared__ int s_wcnt[MAP_WAVES];
    const int w = blockIdx.x;
    const int* h = hdr + w * MAP_HDR;
    const int ninv = select_body(m, h, w, rm[2 * w], rm[2 * w + 1], s_wcnt, desc_id, desc_info);
    if (threadIdx.x == 0) {
        out[w * MAP_OUT + 0] = ninv;
        out[w * MAP_OUT + 1] = h[1];
        out[w * MAP_OUT + 2] = 0;
        out[w * MAP_OUT + 3] = 0;
    }
}

// to_rotation of q / |q| (geometry.py; JPL [x y z w]), row-major
__device__ inline void kf_rotation(const double* q, double* R) {
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double x = q[0] / nq, y = q[1] / nq, z = q[2] / nq, w = q[3] / nq;
    const double d = 2.0 * w * w - 1.0;
    R[0] = d + 2.0 * x * x;
    R[1] = 2.0 * w * z + 2.0 * x * y;
    R[2] = -2.0 * w * y + 2.0 * x * z;
    R[3] = -2.0 * w * z + 2.0 * y * x;
    R[4] = d + 2.0 * y * y;
    R[5] = 2.0 * w * x + 2.0 * y * z;
    R[6] = 2.0 * w * y + 2.0 * z * x;
    R[7] = -2.0 * w * x + 2.0 * z * y;
    R[8] = d + 2.0 * z * z;
}

// The rotation angle between cam records c and key: 2 acos of the last component
// of to_quaternion(R_c R_key^T), the four branches of geometry.to_quaternion.
__device__ inline double kf_angle(const double* Rc, const double* Rk) {
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[i * 3 + j] = Rc[i * 3] * Rk[j * 3] + Rc[i * 3 + 1] * Rk[j * 3 + 1] + Rc[i * 3 + 2] * Rk[j * 3 + 2];
    double u0, u1, u2, u3;
    if (M[8] < 0.0) {
        if (M[0] > M[4]) {
            u0 = 1.0 + M[0] - M[4] - M[8], u1 = M[1] + M[3], u2 = M[6] + M[2], u3 = M[5] - M[7];
        } else {
            u0 = M[1] + M[3], u1 = 1.0 - M[0] + M[4] - M[8], u2 = M[7] + M[5], u3 = M[6] - M[2];
        }
    } else if (M[0] < -M[4]) {
        u0 = M[2] + M[6], u1 = M[7] + M[5], u2 = 1.0 - M[0] - M[4] + M[8], u3 = M[1] - M[3];
    } else {
        u0 = M[5] - M[7], u1 = M[6] - M[2], u2 = M[1] - M[3], u3 = 1.0 + M[0] + M[4] + M[8];
    }
    return 2.0 * acos(u3 / sqrt(u0 * u0 + u1 * u1 + u2 * u2 + u3 * u3));
}

// msckf_keyframe_select: lane 0 chooses the two cam slots (include/msckf_keyframes.h)
// from the filter's cam records, the workgroup then runs the select body with them.
template <typename T>
__global__ void __launch_bounds__(MAP_BLOCK)
k_map_keyframe_select(MapDev m, const int* __restrict__ hdr, const double* __restrict__ rate, double rot_thr,
                      double trans_thr, double rate_thr, const T* __restrict__ cams, int* __restrict__ out,
                      int64_t* __restrict__ desc_id, int* __restrict__ desc_info) {
    __shared__ int s_wcnt[MAP_WAVES];
    __shared__ unsigned long long s_rm[2];
    __shared__ int s_slot[2];
    const int w = blockIdx.x;
    const int* h = hdr + w * MAP_HDR;
    if (threadIdx.x == 0) {
        const int nc = h[3];   // 4 <= nc <= Nmax, checked on the host
        const T* rec = cams + (size_t)h[0] * m.Nmax * CAM_STRIDE;
        const T* kr = rec + (size_t)(nc - 4) * CAM_STRIDE;
        double q[4], Rk[9], Rc[9];
#pragma unroll
        for (int c = 0; c < 4; ++c) q[c] = (double)kr[c];
        kf_rotation(q, Rk);
        const double kp0 = (double)kr[4], kp1 = (double)kr[5], kp2 = (double)kr[6];
        const bool rate_ok = rate[w] > rate_thr;
        int first = 0, slot[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const T* cr = rec + (size_t)(nc - 3 + j) * CAM_STRIDE;
#pragma unroll
            for (int c = 0; c < 4; ++c) q[c] = (double)cr[c];
            kf_rotation(q, Rc);
            const double d0 = (double)cr[4] - kp0, d1 = (double)cr[5] - kp1, d2 = (double)cr[6] - kp2;
            const double dist = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
            const double ang = kf_angle(Rc, Rk);
            slot[j] = (ang < rot_thr && dist < trans_thr && rate_ok) ? nc - 3 + j : first++;
        }
        const int a = min(slot[0], slot[1]), b = max(slot[0], slot[1]);   // distinct: first <= 1 < nc - 3 + j
        unsigned long long r0 = 0, r1 = 0;
        if (a < 64) r0 |= 1ull << a; else r1 |= 1ull << (a - 64);
        if (b < 64) r0 |= 1ull << b; else r1 |= 1ull << (b - 64);
        s_rm[0] = r0;
        s_rm[1] = r1;
        s_slot[0] = a;
        s_slot[1] = b;
    }
    __syncthreads();
    const int ninv = select_body(m, h, w, s_rm[0], s_rm[1], s_wcnt, desc_id, desc_info);
    if (threadIdx.x == 0) {
        out[w * MAP_OUT + 0] = ninv;
        out[w * MAP_OUT + 1] = h[1];
        out[w * MAP_OUT + 2] = s_slot[0];
        out[w * MAP_OUT + 3] = s_slot[1];
    }
}

// msckf_map_prune_commit: the triangulation results into their rows, then every
// row's observations moved to the cam slots that remain.
__global__ void __launch_bounds__(MAP_BLOCK)
k_map_prune_commit(MapDev m, const int* __restrict__ hdr, const unsigned long long* __restrict__ rm,
                   const int* __restrict__ ent_row, const int* __restrict__ ent_valid,
                   const double* __restrict__ ent_pw) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    const MapLds L = map_lds(s_raw, m.cap);
    const int w = blockIdx.x, tid = threadIdx.x, cap = m.cap, Nmax = m.Nmax, N4 = Nmax * 4;
    const int* h = hdr + w * MAP_HDR;
    const int f = h[0], n = h[1], cur = h[2], e0 = h[4], e1 = h[5];
    const unsigned long long r0 = rm[2 * w], r1 = rm[2 * w + 1];
    const MapTab src = m.t[cur], dstt = m.t[cur ^ 1];
    const size_t fb = (size_t)f * cap;
    for (int i = tid; i < cap; i += MAP_BLOCK) L.dst[i] = -1;
    __syncthreads();
    for (int e = e0 + tid; e < e1; e += MAP_BLOCK) {
        const int r = ent_row[e];
        if (r >= 0 && r < n) L.dst[r] = e;   // rows of a filter's entries are distinct (checked on the host)
    }
    __syncthreads();
    for (int i = tid; i < n; i += MAP_BLOCK) {
        const unsigned long long k0 = src.mask[(fb + i) * 2] & ~r0, k1 = src.mask[(fb + i) * 2 + 1] & ~r1;
        unsigned long long o0 = 0, o1 = 0;
        for (int slot = 0; slot < Nmax; ++slot)
            if (bit_of(k0, k1, slot)) {
                const int ns = slot - bits_below(r0, r1, slot);
                if (ns < 64) o0 |= 1ull << ns; else o1 |= 1ull << (ns - 64);
            }
        const int e = L.dst[i];
        dstt.ids[fb + i] = src.ids[fb + i];
        dstt.mask[(fb + i) * 2] = o0;
        dstt.mask[(fb + i) * 2 + 1] = o1;
        for (int c = 0; c < 3; ++c) dstt.pw[(fb + i) * 3 + c] = e >= 0 ? ent_pw[(size_t)e * 3 + c] : src.pw[(fb + i) * 3 + c];
        dstt.init[fb + i] = e >= 0 ? (ent_valid[e] ? 1 : 0) : src.init[fb + i];
    }
    for (int e = tid; e < n * N4; e += MAP_BLOCK) {
        const int i = e / N4, kk = e - i * N4, slot = kk >> 2;
        const unsigned long long k0 = src.mask[(fb + i) * 2] & ~r0, k1 = src.mask[(fb + i) * 2 + 1] & ~r1;
        if (bit_of(k0, k1, slot)) {
            const int ns = slot - bits_below(r0, r1, slot);   // ns <= slot < Nmax
            dstt.z[(fb + i) * N4 + ns * 4 + (kk & 3)] = src.z[(fb + i) * N4 + kk];
        }
    }
}

// The fill of msckf_map_load: what msckf_batch_load copies from the host's
// arrays, gathered from the tables; one thread per feature.
template <typename T>
__global__ void __launch_bounds__(MAP_BLOCK)
k_map_gather(MapDev m, int mode, int nf, const int* __restrict__ feat_filter, const int* __restrict__ obs_off,
             const int* __restrict__ frow, const int* __restrict__ sel, const unsigned long long* __restrict__ rm,
             const double* __restrict__ host_pw, const double* __restrict__ chi2_tab, T big,
             int* __restrict__ obs_cam, T* __restrict__ obs_z, T* __restrict__ chi2, uint8_t* __restrict__ valid,
             T* __restrict__ p_w) {
    const int f = blockIdx.x * MAP_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const int b = feat_filter[f], r = frow[f], N4 = m.Nmax * 4;
    const MapTab tab = m.t[sel[b]];
    const size_t row = (size_t)b * m.cap + r;
    unsigned long long k0 = tab.mask[row * 2], k1 = tab.mask[row * 2 + 1];
    if (mode == 2) {
        k0 &= rm[2 * b];
        k1 &= rm[2 * b + 1];
    }
    const int o0 = obs_off[f], cnt = obs_off[f + 1] - o0;
    int k = 0;
    for (int slot = 0; slot < m.Nmax && k < cnt; ++slot)
        if (bit_of(k0, k1, slot)) {
            obs_cam[o0 + k] = slot;
            for (int c = 0; c < 4; ++c) obs_z[(size_t)(o0 + k) * 4 + c] = (T)tab.z[row * N4 + slot * 4 + c];
            ++k;
        }
    for (; k < cnt; ++k) {   // a count that is not the descriptor's: defined contents, never out of bounds
        obs_cam[o0 + k] = 0;
        for (int c = 0; c < 4; ++c) obs_z[(size_t)(o0 + k) * 4 + c] = (T)0;
    }
    if (mode == 1) {
        chi2[f] = big;
        valid[f] = 0;
        return;
    }
    const int dof = mode == 0 ? cnt - 1 : cnt;   // 1..99, checked on the host
    chi2[f] = (T)chi2_tab[dof - 1];
    double p[3];
    bool have = mode == 2 || tab.init[row] != 0;
    for (int c = 0; c < 3; ++c) p[c] = tab.pw[row * 3 + c];
    if (mode == 2 && host_pw) {
        const double* hp = host_pw + (size_t)f * 3;
        if (isfinite(hp[0]) && isfinite(hp[1]) && isfinite(hp[2]))
            for (int c = 0; c < 3; ++c) p[c] = hp[c];
    }
    if (!have)
        for (int c = 0; c < 3; ++c) p[c] = __builtin_nan("");
    for (int c = 0; c < 3; ++c) p_w[(size_t)f * 3 + c] = (T)p[c];
    valid[f] = (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) ? 2 : 0;
}

// msckf_landmarks_archive (include/msckf_odometry.h): the accepted features of
// the filter's part of the loaded batch, in batch order, appended to its ring.
// The host guarantees count <= ring cap (no slot is written twice in a call) and
// every frow inside the lost table.
template <typename T>
__global__ void __launch_bounds__(MAP_BLOCK)
k_lm_archive(MapDev m, LmDev L, const int* __restrict__ hdr, const int* __restrict__ frow,
             const uint8_t* __restrict__ include, const T* __restrict__ p_w, const T* __restrict__ gamma) {
    __shared__ int s_wcnt[MAP_WAVES];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int* h = hdr + w * LM_HDR;
    const int f = h[0], a0 = h[2], n = h[3], stamp = h[4];
    const MapTab tab = m.t[h[1]];
    const size_t fb = (size_t)f * m.cap, rb = (size_t)f * L.cap;
    const long long seq0 = L.seq[f];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += MAP_BLOCK) {
        const int i = i0 + tid;
        const bool take = i < n && include[a0 + i] != 0;
        int tot;
        const int rk = block_rank(take, s_wcnt, tot);
        if (take) {
            const size_t row = fb + frow[a0 + i];
            const size_t d = rb + (size_t)((seq0 + base + rk) % L.cap);
            L.ids[d] = tab.ids[row];
            for (int c = 0; c < 3; ++c) L.pw[d * 3 + c] = (double)p_w[(size_t)(a0 + i) * 3 + c];
            L.gamma[d] = (double)gamma[a0 + i];
            L.nobs[d] = __popcll(tab.mask[row * 2]) + __popcll(tab.mask[row * 2 + 1]);
            L.stamp[d] = stamp;
        }
        base += tot;
    }
    __syncthreads();   // every thread's last use of seq0 lies before the one store to seq
    if (tid == 0 && base) L.seq[f] = seq0 + base;
}

}  // namespace

template <typename T>
void launch_lm_archive(hipStream_t s, const MapDev& m, const LmDev& L, int nfilt, const int* hdr, const int* frow,
                       const uint8_t* include, const T* p_w, const T* gamma) {
    if (nfilt <= 0) return;
    hipLaunchKernelGGL(k_lm_archive<T>, dim3(nfilt), dim3(MAP_BLOCK), 0, s, m, L, hdr, frow, include, p_w, gamma);
}
template void launch_lm_archive<float>(hipStream_t, const MapDev&, const LmDev&, int, const int*, const int*,
                                       const uint8_t*, const float*, const float*);
template void launch_lm_archive<double>(hipStream_t, const MapDev&, const LmDev&, int, const int*, const int*,
                                        const uint8_t*, const double*, const double*);

size_t map_lds_bytes(int cap) { return (size_t)cap * 16 + MAP_WAVES * sizeof(int); }

void launch_map_add_lost(hipStream_t s, const MapDev& m, int nfilt, const int* hdr, const int64_t* msg_ids,
                         const double* msg_z, int* out, int64_t* desc_id, int* desc_info) {
    hipLaunchKernelGGL(k_map_add_lost, dim3(nfilt), dim3(MAP_BLOCK), map_lds_bytes(m.cap), s, m, hdr, msg_ids, msg_z,
                       out, desc_id, desc_info);
}

void launch_map_prune_select(hipStream_t s, const MapDev& m, int nfilt, const int* hdr, const unsigned long long* rm,
                             int* out, int64_t* desc_id, int* desc_info) {
    hipLaunchKernelGGL(k_map_prune_select, dim3(nfilt), dim3(MAP_BLOCK), 0, s, m, hdr, rm, out, desc_id, desc_info);
}

template <typename T>
void launch_map_keyframe_select(hipStream_t s, const MapDev& m, int nfilt, const int* hdr, const double* rate,
                                double rot_thr, double trans_thr, double rate_thr, const T* cams, int* out,
                                int64_t* desc_id, int* desc_info) {
    hipLaunchKernelGGL(k_map_keyframe_select<T>, dim3(nfilt), dim3(MAP_BLOCK), 0, s, m, hdr, rate, rot_thr, trans_thr,
                       rate_thr, cams, out, desc_id, desc_info);
}
template void launch_map_keyframe_select<float>(hipStream_t, const MapDev&, int, const int*, const double*, double,
                                                double, double, const float*, int*, int64_t*, int*);
template void launch_map_keyframe_select<double>(hipStream_t, const MapDev&, int, const int*, const double*, double,
                                                 double, double, const double*, int*, int64_t*, int*);

void launch_map_prune_commit(hipStream_t s, const MapDev& m, int nfilt, const int* hdr, const unsigned long long* rm,
                             const int* ent_row, const int* ent_valid, const double* ent_pw) {
    hipLaunchKernelGGL(k_map_prune_commit, dim3(nfilt), dim3(MAP_BLOCK), map_lds_bytes(m.cap), s, m, hdr, rm, ent_row,
                       ent_valid, ent_pw);
}

template <typename T>
void launch_map_gather(hipStream_t s, const MapDev& m, int mode, int nf, const int* feat_filter, const int* obs_off,
                       const int* frow, const int* sel, const unsigned long long* rm, const double* host_pw,
                       const double* chi2_tab, T big, int* obs_cam, T* obs_z, T* chi2, uint8_t* valid, T* p_w) {
    if (nf <= 0) return;
    hipLaunchKernelGGL(k_map_gather<T>, dim3((nf + MAP_BLOCK - 1) / MAP_BLOCK), dim3(MAP_BLOCK), 0, s, m, mode, nf,
                       feat_filter, obs_off, frow, sel, rm, host_pw, chi2_tab, big, obs_cam, obs_z, chi2, valid, p_w);
}
template void launch_map_gather<float>(hipStream_t, const MapDev&, int, int, const int*, const int*, const int*,
                                       const int*, const unsigned long long*, const double*, const double*, float,
                                       int*, float*, float*, uint8_t*, float*);
template void launch_map_gather<double>(hipStream_t, const MapDev&, int, int, const int*, const int*, const int*,
                                        const int*, const unsigned long long*, const double*, const double*, double,
                                        int*, double*, double*, uint8_t*, double*);

}  // namespace msckf
