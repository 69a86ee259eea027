// msckf_subbatch.h -- how a batch of B filters is cut into lanes, and where the
// cut falls in the per-class feature lists.  A lane is a contiguous range of
// filter slots whose whole update chain is enqueued on streams of its own, so
// that one lane's kernels fill the CUs another lane's stage is draining.
// Plain C++17, no HIP include: a host compiler builds it alone
// (tests/test_subbatch_ref.py drives it).
#pragma once

namespace msckf {

constexpr int SUBBATCH_MAX_LANES = 2;
// The Kalman kernels keep 2 filters x 256 CUs = 512 filters resident: a lane of
// fewer filters cannot fill the chip on its own, so batches under 2 x 512 stay whole.
constexpr int SUBBATCH_MIN_B = 1024;

// Lanes of a batch of B filters.  forced: 0 = by size, 1 / 2 = that many lanes
// (MSCKF_SUBBATCH; two lanes need two filters).
constexpr int subbatch_lanes(int B, int forced) {
    if (B < 2) return 1;
    if (forced == 1 || forced == 2) return forced;
    return B >= SUBBATCH_MIN_B ? 2 : 1;
}

// First filter slot of `lane` of `nlanes` (lane == nlanes: B): two lanes cut at
// B / 2, lane 0 = [0, B / 2), lane 1 the rest (the larger half when B is odd).
constexpr int subbatch_first_filter(int B, int lane, int nlanes) {
    return lane <= 0 ? 0 : (lane >= nlanes ? B : B / 2);
}

// Index of the first entry >= f_cut of an ascending feature list.
inline int subbatch_cut(const int* list, int n, int f_cut) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (list[mid] < f_cut) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Class lists stored back to back (`flat`, list l = [off[l], off[l + 1]), each
// ascending in feature index -- load_features builds them so): cut[l] is the
// offset into `flat` where the entries of list l that are >= f_cut begin.  The
// features of the filters [0, b_cut) are [0, feat_off[b_cut]), so with f_cut =
// feat_off[b_cut] lane 0 takes [off[l], cut[l]) and lane 1 [cut[l], off[l + 1]).
inline void subbatch_cut_lists(const int* flat, const int* off, int nlists, int f_cut, int* cut) {
    for (int l = 0; l < nlists; ++l) cut[l] = off[l] + subbatch_cut(flat + off[l], off[l + 1] - off[l], f_cut);
}

// A class-list table (offsets off[0 .. nlists] into one flat list) narrowed to
// one lane: writes the nlists + 1 offsets of the lane's sub-lists.  They are not
// contiguous across classes, so the result is (begin, end) pairs: begin[l],
// end[l].
inline void subbatch_lane_lists(const int* off, const int* cut, int nlists, int lane, int nlanes, int* begin,
                                int* end) {
    for (int l = 0; l < nlists; ++l) {
        begin[l] = (nlanes == 1 || lane == 0) ? off[l] : cut[l];
        end[l] = (nlanes == 1 || lane == nlanes - 1) ? off[l + 1] : cut[l];
    }
}

}  // namespace msckf
