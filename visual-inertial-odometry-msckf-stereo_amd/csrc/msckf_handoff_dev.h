// msckf_handoff_dev.h -- what msckf_map_add_lost_tracks (msckf_map_api.inc) reads of a
// front-end context (include/msckf_handoff.h): the lanes' message tables where they lie on
// the device, and the host's record of each lane's row count and valid flag.  Defined in
// msckf_frontend.hip, which owns the context.
#pragma once
#include <cstdint>

struct mfe_ctx;

namespace msckf {

struct TrackMsgView {
    int device, n_lanes, cap;
    const int64_t* ids;          // device, [n_lanes][cap]
    const double* uv;            // device, [n_lanes][cap][4]
    const int* n;                // host, [n_lanes]
    const unsigned char* valid;  // host, [n_lanes]
};

// false: null context or a context without track tables
bool mfe_track_messages(const mfe_ctx* c, TrackMsgView& v);

}  // namespace msckf
