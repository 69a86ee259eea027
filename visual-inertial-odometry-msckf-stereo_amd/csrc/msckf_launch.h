// msckf_launch.h -- host-side launcher declarations + per-kernel HIP-event timer.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "msckf_common.h"
#include "msckf_gate_routes.h"

namespace msckf {

// Raise a kernel's dynamic-LDS limit to at least `bytes` on the current
// device.  hipFuncSetAttribute is per device, so the grant is remembered per
// (kernel, device) -- a process-wide flag would skip a context on a second
// device -- and under a lock (contexts may launch from several threads).
inline void lds_limit(const void* fn, size_t bytes) {
    if (bytes <= 64 * 1024) return;   // the default grant
    struct Grant { const void* fn; int dev; size_t bytes; };
    static std::mutex mu;
    static std::vector<Grant> grants;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    for (auto& e : grants)
        if (e.fn == fn && e.dev == dev) {
            if (e.bytes >= bytes) return;
            (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            e.bytes = bytes;
            return;
        }
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    grants.push_back({fn, dev, bytes});
}

// Accumulates device time per kernel name from HIP events recorded on the
// launch stream (so the measurement sees exactly the stream the kernel runs on).
// One timer per lane (msckf_subbatch.h): each has its own open interval, and
// msckf_kernel_times adds the lanes' totals.
struct KernelTimer {
    bool on = false;
    std::string only;    // non-empty: time this stage only (the others record no events)
    bool open = false;   // the last begin() recorded an event
    struct Pending { std::string name; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<std::string> names;
    std::vector<double> total_ms;
    std::vector<int> launches;
    std::vector<hipEvent_t> pool;

    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    void begin(hipStream_t s, const char* name) {
        open = on && (only.empty() || only == name);
        if (!open) return;
        Pending p{name, get(), get()};
        (void)hipEventRecord(p.a, s);
        pending.push_back(p);
    }
    void end(hipStream_t s) {
        if (!open || pending.empty()) return;
        (void)hipEventRecord(pending.back().b, s);
        open = false;
    }
    // call after the stream is synchronised
    void collect() {
        for (auto& p : pending) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, p.a, p.b);
            size_t k = 0;
            while (k < names.size() && names[k] != p.name) ++k;
            if (k == names.size()) { names.push_back(p.name); total_ms.push_back(0); launches.push_back(0); }
            total_ms[k] += ms;
            launches[k] += 1;
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    void reset() { names.clear(); total_ms.clear(); launches.clear(); }
    ~KernelTimer() {
        for (auto& p : pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// Per-filter stages batched over a device list of filter slots (one
// workgroup per listed filter).
template <typename T>
void launch_propagate(hipStream_t, const DevState<T>&, const Params<T>&, int nfilt, const int* filters,
                      const int* smp_off, const T* samples);
template <typename T>
void launch_augment(hipStream_t, const DevState<T>&, int nfilt, const int* filters);
template <typename T>
void launch_prune(hipStream_t, const DevState<T>&, int nfilt, const int* filters, const int* keep_off,
                  const int* keep, const int* kcam_off, const int* keep_cams);
template <typename T>
void launch_cov_diag(hipStream_t, const DevState<T>&, int nfilt, const int* filters, int i0, int n, T* out);
// Per-feature kernels packed S lanes per feature: features listed by class
// (M <= S), 64/S features per wavefront.
struct SegClasses {
    static constexpr int NC = 5;
    static constexpr int S[NC] = {8, 16, 32, 64, 128};   // 128: a whole wavefront, 2 observations per lane
    const int* list = nullptr;
    int off[NC + 1] = {};             // the loaded batch's lists, back to back in `list`
    int beg[NC] = {}, end[NC] = {};   // what a launch covers of each: all of it, or one lane's part (msckf_subbatch.h)
};
template <typename T>
void launch_triangulate(hipStream_t, const DevState<T>&, const Params<T>&, const FeatBatch<T>&, const SegClasses&);
// The lean feature path of one lane (fused assembly, no compact factors; the
// classes with one observation per lane): the ill lists (laid out as the class
// lists: a lane's part of a class has its own range) and the lane's two sets
// of FEAT_LEAN_NCLS counts -- the step appends to ill_cnt, and its second pass
// zeroes ill_cnt_next, which the lane's next lean step uses (both zero at
// allocation).  on == false (MSCKF_FEATURE=full): k_feature for every feature.
struct FeatLean {
    bool on = false;
    int* ill_list = nullptr;
    int* ill_cnt = nullptr;
    int* ill_cnt_next = nullptr;
};
// Returns whether the lean second pass ran (the caller then swaps the lane's count sets).
template <typename T>
bool launch_feature(hipStream_t, const DevState<T>&, const Params<T>&, const FeatBatch<T>&, const SegClasses&,
                    const FeatLean&);
// Feature index lists per gating route (device pointer + host offsets), one
// level: list l = gate_list_of(M) of msckf_gate_routes.h holds the tracks of
// exactly l + 1 16-row blocks (M <= 82), the last list M >= 83; gate_route
// names the kernel of each list.  Features keep ascending index inside a list.
struct GateClasses {
    const int* list = nullptr;
    int off[GATE_NLIST + 1] = {};
    int beg[GATE_NLIST] = {}, end[GATE_NLIST] = {};   // launched range of each list, as SegClasses
    int maxM[GATE_NLIST] = {};                         // of the whole list: a lane runs the whole batch's kernels
};
// Returns 0, or the 16-row block count of a non-empty feature list that no
// gating kernel is instantiated for (those features then keep the previous
// batch's gamma / accept: the caller must fail the update).
template <typename T>
int launch_gate(hipStream_t, const DevState<T>&, const Params<T>&, const FeatBatch<T>&, const GateClasses&);
// Gating on MFMA tiles (msckf_gate_mfma.hip; fp32: v_mfma_f32_16x16x4_f32, fp64:
// v_mfma_f64_16x16x4_f64) of one tile list, the tracks of exactly nb blocks:
// k_gate_mfma<nb>, one wavefront per feature, or k_gate_mfma_wt<nb, W>, a W-wave
// workgroup per feature, as gate_route(nb - 1, sizeof(T)) says.
// false: no kernel for this block count, nothing launched.
template <typename T>
bool launch_gate_tiles(hipStream_t, const DevState<T>&, const Params<T>&, const FeatBatch<T>&, const int* list,
                       int cnt, int nb, int maxM);
template <typename T>
void launch_select(hipStream_t, const DevState<T>&, const FeatBatch<T>&, const UpdWs<T>&, int row_cap);
template <typename T>
void launch_compress(hipStream_t, const DevState<T>&, const Params<T>&, const FeatBatch<T>&, const UpdWs<T>&, int maxnf,
                     int maxobs);
// The fused information assembly (no per-observation Gram records) runs when
// the window has <= 32 cams and its per-filter tables fit the LDS.
bool info_fused_fits(int Nmax, int maxnf);
// The global-memory gating kernel k_gate (M > GATE_TILE_MAXM) needs k_feature's
// compact QR factors and the (4M)^2 scratch FeatBatch::ysq
inline bool feature_needs_compact(int maxM) { return maxM > GATE_TILE_MAXM; }
bool kalman_chol_supported(int Cmax);
size_t kalman_global_ws_doubles(int Cmax);
// UpdWs::rev: whether the register-tile stage C of a batch of batch_B filters
// factors T in the reverse pivot order (msckf_kalman.hip)
bool kalman_reverse_order(int batch_B);
// Stage A of the register-tile windows (kalman_chol_supported) reads only P and
// writes only Lc / Vi / Sii / afail, so it is launched on a side stream at the
// start of the update chain; launch_kalman_chol then skips it.
// batch_B: the filter count of the whole batch, which picks the Cholesky path
// (MK_MIN_B) -- DevState::B is the launched lane's count and only sizes grids.
template <typename T>
void launch_kalman_a_reg(hipStream_t, const DevState<T>&, const UpdWs<T>&, KernelTimer*, int batch_B);
template <typename T>
void launch_kalman_chol(hipStream_t, const DevState<T>&, const Params<T>&, const UpdWs<T>&, KernelTimer*,
                        int batch_B);
template <typename T>
void launch_kalman(hipStream_t, const DevState<T>&, const Params<T>&, const UpdWs<T>&, KernelTimer*, int batch_B);

}  // namespace msckf
