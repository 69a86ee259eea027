// msckf_anchor_dev.h -- device views and launchers of the anchor fixes
// (include/msckf_anchor.h; kernels in msckf_anchor.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/msckf_anchor.h"
#include "msckf_common.h"

namespace msckf {

constexpr int ANC_M = 12;                    // rows of the compressed measurement; the stride of a W row
constexpr int ANC_C = 12;                    // columns of P that H touches: 0:3, 12:15, 15:21
constexpr int ANC_K = MSCKF_ANCHOR_MAX;      // anchors per filter and call: one wave's lanes

// The context's anchor workspace, indexed by filter slot.
struct AnchorDev {
    double* W;          // [B][Dmax][ANC_M]  P H'^T L^-T of the last applied update
    int* applied;       // [B]
    int* used;          // [B]  K' of the last call
    int* rows;          // [B]  m of the last call
    long long* count;   // [B]  updates ever applied
    int* n;             // [B]  anchors of the last call
    double* gamma;      // [B][ANC_K]
    uint8_t* status;    // [B][ANC_K]
};

// The call's parameters and the context's stereo extrinsics, all double.
struct AnchorPrm {
    double obs_var, chi2, min_depth;
    int min_anchors;
    double R_cc[9], t_cc[3];
};

// filters: device list [nfilt]; off: device [nfilt + 1]; anchors: device msckf_anchor_t [off[nfilt]]
template <typename T>
void launch_anchor_gain(hipStream_t, const DevState<T>&, const AnchorDev&, const AnchorPrm&, int nfilt,
                        const int* filters, const int* off, const msckf_anchor_t* anchors);
// maxD: the largest D = 21 + 6 n of the listed filters (sizes the tile grid)
template <typename T>
void launch_anchor_apply(hipStream_t, const DevState<T>&, const AnchorDev&, int nfilt, const int* filters, int maxD);

}  // namespace msckf
