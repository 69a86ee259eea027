// msckf_standstill_dev.h -- what msckf_zupt_batch_cued (msckf_zupt_api.inc) reads of a
// front-end context (include/msckf_standstill.h): the lanes' motion records where they lie
// on the device, and the host's record of each lane's valid flag.  Defined in
// msckf_frontend.hip, which owns the context.
#pragma once
#include <cstdint>

struct mfe_ctx;

namespace msckf {

// a lane's record, written by k_trk_motion
struct MotionRec {
    int32_t n;   // the pairs behind the statistic (after_ransac)
    float d2;    // the q-quantile of the squared pixel displacement; NaN for n = 0
};

struct TrackMotionView {
    int device, n_lanes;
    const MotionRec* rec;        // device, [n_lanes]
    const unsigned char* valid;  // host, [n_lanes]
};

// false: null context or a context without track tables
bool mfe_track_motion(const mfe_ctx* c, TrackMotionView& v);

}  // namespace msckf
