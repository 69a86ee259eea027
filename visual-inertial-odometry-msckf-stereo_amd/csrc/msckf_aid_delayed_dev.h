// msckf_aid_delayed_dev.h -- device views and launchers of the delayed aiding
// fixes (include/msckf_aid_delayed.h; kernels in msckf_aid_delayed.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/msckf_aid_delayed.h"
#include "msckf_common.h"

namespace msckf {

constexpr int ADL_M = 6;     // rows of the full measurement
constexpr int ADL_WS = 12;   // the stride of a W row: msckf_aid.h's workspace layout
constexpr int ADL_C = 18;    // columns of P that H touches: 15:21 and the twelve of clones s, s + 1

// The context's workspace of the delayed fixes, indexed by filter slot.
struct AidDelayedDev {
    double* W;          // [B][Dmax][ADL_WS]  P H^T L^-T of the last applied fix
    int* applied;       // [B]
    double* gamma;      // [B]
    int* rows;          // [B]  the mask of the last fix
    int* status;        // [B]  MSCKF_AID_DELAYED_*
    long long* count;   // [B]  fixes ever applied
};

// filters: device list [nfilt]; fixes: device msckf_aid_delayed_fix_t [nfilt]
template <typename T>
void launch_aid_delayed_gain(hipStream_t, const DevState<T>&, const AidDelayedDev&, const msckf_aid_params_t&, int nfilt,
                             const int* filters, const msckf_aid_delayed_fix_t* fixes);
// maxD: the largest D = 21 + 6 n of the listed filters (sizes the tile grid)
template <typename T>
void launch_aid_delayed_apply(hipStream_t, const DevState<T>&, const AidDelayedDev&, int nfilt, const int* filters,
                              int maxD);

}  // namespace msckf
