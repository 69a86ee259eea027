// msckf_zupt_dev.h -- device views and launchers of the zero-velocity update
// (include/msckf_zupt.h; kernels in msckf_zupt.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "msckf_common.h"
#include "msckf_standstill_dev.h"

namespace msckf {

constexpr int ZUPT_M = 9;    // rows of the full measurement; the stride of a W row
constexpr int ZUPT_TS = 32;  // k_zupt_apply's tile edge

// The context's ZUPT workspace, indexed by filter slot.
struct ZuptDev {
    double* W;          // [B][Dmax][ZUPT_M]  P H^T L^-T of the last applied update
    int* applied;       // [B]
    double* gamma;      // [B]
    long long* count;   // [B]  updates ever applied
    // the vision cue as the last cued call saw it (include/msckf_standstill.h)
    int* cue;           // [B]  status, -1 before the first cued call
    int* cue_n;         // [B]
    float* cue_d2;      // [B]
};

// msckf_zupt_cue_t as the cued gain kernel takes it, with the cue's source: rec != null, the
// front-end's motion records read in place through lane[w] (-1: no valid record); else n / d2
// of the call's input block (n < 0: no record).
struct ZuptCueArgs {
    double max_px2;
    int min_tracks, mode, unknown;
    const MotionRec* rec;
    const int* lane;    // device [nfilt]
    const int* n;       // device [nfilt]
    const float* d2;    // device [nfilt]
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
// the same launch with the cue in the decision (msckf_zupt_batch_cued)
template <typename T>
void launch_zupt_gain_cued(hipStream_t, const DevState<T>&, const ZuptDev&, const ZuptArgs&, const ZuptCueArgs&,
                           int nfilt, const int* filters, const double* means);
// maxD: the largest D = 21 + 6 n of the listed filters (sizes the tile grid)
template <typename T>
void launch_zupt_apply(hipStream_t, const DevState<T>&, const ZuptDev&, int m, int nfilt, const int* filters, int maxD);

}  // namespace msckf
