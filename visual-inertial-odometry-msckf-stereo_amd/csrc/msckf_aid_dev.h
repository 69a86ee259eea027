// msckf_aid_dev.h -- device views and launchers of the aiding fixes
// (include/msckf_aid.h; kernels in msckf_aid.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/msckf_aid.h"
#include "msckf_common.h"

namespace msckf {

constexpr int AID_M = 12;   // rows of the full measurement; the stride of a W row
constexpr int AID_C = 9;    // columns of P that H touches: 0:3, 6:9, 12:15

// The context's aiding workspace, indexed by filter slot.
struct AidDev {
    double* W;          // [B][Dmax][AID_M]  P H^T L^-T of the last applied fix
    int* applied;       // [B]
    double* gamma;      // [B]
    int* rows;          // [B]  the mask of the last fix
    long long* count;   // [B]  fixes ever applied
};

// filters: device list [nfilt]; fixes: device msckf_aid_fix_t [nfilt]
template <typename T>
void launch_aid_gain(hipStream_t, const DevState<T>&, const AidDev&, const msckf_aid_params_t&, int nfilt,
                     const int* filters, const msckf_aid_fix_t* fixes);
// maxD: the largest D = 21 + 6 n of the listed filters (sizes the tile grid)
template <typename T>
void launch_aid_apply(hipStream_t, const DevState<T>&, const AidDev&, int nfilt, const int* filters, int maxD);

}  // namespace msckf
