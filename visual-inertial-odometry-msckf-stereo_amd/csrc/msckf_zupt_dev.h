// msckf_zupt_dev.h -- device views and launchers of the zero-velocity update
// (include/msckf_zupt.h; kernels in msckf_zupt.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "msckf_common.h"

namespace msckf {

constexpr int ZUPT_M = 9;    // rows of the full measurement; the stride of a W row
constexpr int ZUPT_TS = 32;  // k_zupt_apply's tile edge

// The context's ZUPT workspace, indexed by filter slot.
struct ZuptDev {
    double* W;          // [B][Dmax][ZUPT_M]  P H^T L^-T of the last applied update
    int* applied;       // [B]
    double* gamma;      // [B]
    long long* count;   // [B]  updates ever applied
};

// msckf_zupt_params_t as the kernels take it: the noise per group, the kept rows m.
struct ZuptArgs {
    double noise[3];
    double chi2, max_speed;
    int rows, m;
};

// filters: device list [nfilt]; means: device double [nfilt][6] (gyro mean, acc mean)
template <typename T>
void launch_zupt_gain(hipStream_t, const DevState<T>&, const ZuptDev&, const ZuptArgs&, int nfilt, const int* filters,
                      const double* means);
// maxD: the largest D = 21 + 6 n of the listed filters (sizes the tile grid)
template <typename T>
void launch_zupt_apply(hipStream_t, const DevState<T>&, const ZuptDev&, int m, int nfilt, const int* filters, int maxD);

}  // namespace msckf
