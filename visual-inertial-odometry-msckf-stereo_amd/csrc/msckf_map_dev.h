// msckf_map_dev.h -- device views and launcher declarations of the feature
// map kept on the device (include/msckf_map.h; kernels in msckf_map.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace msckf {

// One of a context's two table sets, fixed stride [filter][cap]:
//   ids [B][cap], mask [B][cap][2], z [B][cap][Nmax][4], pw [B][cap][3], init [B][cap]
struct MapTab {
    int64_t* ids;
    unsigned long long* mask;
    double* z;
    double* pw;
    uint8_t* init;
};
struct MapDev {
    MapTab t[2];
    int cap, Nmax;
};

constexpr int MAP_HDR = 8;        // ints per named filter in a call's header (see each kernel)
constexpr int MAP_OUT = 4;        // ints per named filter a select call returns
constexpr int MAP_INFO = 4;       // ints per descriptor entry: M, involved count, initialised flag, row
constexpr int MAP_MAX_CAP = 2048; // ids + two int tables in LDS: 16 B per row

size_t map_lds_bytes(int cap);

// hdr: [filter, n, table read, newest slot, msg first, msg end, descriptor stride (>= every n), -]
void launch_map_add_lost(hipStream_t, const MapDev&, int nfilt, const int* hdr, const int64_t* msg_ids,
                         const double* msg_z, int* out, int64_t* desc_id, int* desc_info);
// hdr: [filter, n, table read, -, -, -, descriptor stride, -]; rm: the removed slots as a mask, two words per named filter
void launch_map_prune_select(hipStream_t, const MapDev&, int nfilt, const int* hdr, const unsigned long long* rm,
                             int* out, int64_t* desc_id, int* desc_info);
// msckf_keyframe_select (include/msckf_keyframes.h): the select with the two slots chosen in the kernel from the
// filter's cam records (cams: the context's [B][Nmax][CAM_STRIDE]); out[2], out[3] = the slots, ascending
// hdr: [filter, n, table read, cam states, -, -, descriptor stride, -]; rate: tracking rate per named filter
template <typename T>
void launch_map_keyframe_select(hipStream_t, const MapDev&, int nfilt, const int* hdr, const double* rate,
                                double rot_thr, double trans_thr, double rate_thr, const T* cams, int* out,
                                int64_t* desc_id, int* desc_info);
// hdr: [filter, n, table read, -, entry first, entry end, -, -]; entries: row, valid flag, position
void launch_map_prune_commit(hipStream_t, const MapDev&, int nfilt, const int* hdr, const unsigned long long* rm,
                             const int* ent_row, const int* ent_valid, const double* ent_pw);
// The fill of a loaded batch (msckf_map_load): per feature f of the arena,
// row frow[f] of filter feat_filter[f]'s table sel[filter]; mode as MSCKF_MAP_LOAD_*.
template <typename T>
void launch_map_gather(hipStream_t, const MapDev&, int mode, int nf, const int* feat_filter, const int* obs_off,
                       const int* frow, const int* sel, const unsigned long long* rm, const double* host_pw,
                       const double* chi2_tab, T big, int* obs_cam, T* obs_z, T* chi2, uint8_t* valid, T* p_w);

// The landmark rings (include/msckf_odometry.h), fixed stride [filter][cap]:
//   ids [B][cap], pw [B][cap][3], gamma [B][cap], nobs [B][cap], stamp [B][cap]; seq [B]
struct LmDev {
    int64_t* ids;
    double* pw;
    double* gamma;
    int* nobs;
    int* stamp;
    long long* seq;
    int cap;
};
constexpr int LM_HDR = 8;   // ints per named filter in an archive call's header
// msckf_landmarks_archive: per named filter the accepted features [first, first + count) of the loaded batch,
// in batch order, appended to the filter's ring.  frow: the batch's rows of the lost table (the load's device
// copy); include / p_w / gamma: the batch's results.
// hdr: [filter, lost table, first feature of the batch, count (<= ring cap), stamp, -, -, -]
template <typename T>
void launch_lm_archive(hipStream_t, const MapDev&, const LmDev&, int nfilt, const int* hdr, const int* frow,
                       const uint8_t* include, const T* p_w, const T* gamma);

}  // namespace msckf
