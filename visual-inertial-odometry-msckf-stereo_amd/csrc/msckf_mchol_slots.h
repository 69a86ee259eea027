// msckf_mchol_slots.h -- which 16 x 16 block of the lower triangle each wave of
// k_kal_mchol holds in which accumulator slot, as compile-time data.  The
// NBR (NBR + 1) / 2 lower blocks are numbered column by column (block column 0:
// rows 0 .. NBR - 1, block column 1: rows 1 .. NBR - 1, ...) and dealt round-robin:
// slot j of wave WV of NW holds block t = WV + NW j.  Within a wave the block
// column therefore never decreases with j, so the slots a pivot step of block
// column KB updates are a suffix of the wave's slots: first the slots of column
// KB itself (updated on the column's first three steps only), then the slots of
// the columns right of it (updated on every step).
// Plain C++17, no HIP include: a host compiler builds it alone
// (tests/test_mchol_slots_ref.py drives it).
#pragma once

namespace msckf {

constexpr int mk_nblk(int NBR) { return NBR * (NBR + 1) / 2; }
// accumulator slots per wave (the last one is empty in some waves)
constexpr int mk_nslots(int NBR, int NW) { return (mk_nblk(NBR) + NW - 1) / NW; }

// block column / row of block t of the column-major lower enumeration
constexpr int mk_col_of(int NBR, int t) {
    int cb = 0, rem = t;
    while (cb < NBR && rem >= NBR - cb) { rem -= NBR - cb; ++cb; }
    return cb;
}
constexpr int mk_row_of(int NBR, int t) {
    int cb = 0, rem = t;
    while (cb < NBR && rem >= NBR - cb) { rem -= NBR - cb; ++cb; }
    return cb + rem;
}

// slot j of wave WV: block row (-1: empty slot) and block column (NBR: an
// empty slot matches no column)
constexpr int mk_brow(int NBR, int NW, int WV, int j) {
    return WV + NW * j < mk_nblk(NBR) ? mk_row_of(NBR, WV + NW * j) : -1;
}
constexpr int mk_bcol(int NBR, int NW, int WV, int j) {
    return WV + NW * j < mk_nblk(NBR) ? mk_col_of(NBR, WV + NW * j) : NBR;
}

// first slot of wave WV whose block column is >= KB (the wave's slot count if
// there is none; empty slots count as column NBR)
constexpr int mk_first_slot(int NBR, int NW, int WV, int KB) {
    int j = 0;
    while (j < mk_nslots(NBR, NW) && mk_bcol(NBR, NW, WV, j) < KB) ++j;
    return j;
}
// slots of wave WV that hold a block
constexpr int mk_used_slots(int NBR, int NW, int WV) { return mk_first_slot(NBR, NW, WV, NBR); }

// every lower block is held exactly once, by a used slot, and a wave's block
// column never decreases with the slot
constexpr bool mk_map_ok(int NBR, int NW) {
    for (int c = 0; c < NBR; ++c)
        for (int r = c; r < NBR; ++r) {
            int owners = 0;
            for (int w = 0; w < NW; ++w)
                for (int j = 0; j < mk_nslots(NBR, NW); ++j)
                    if (mk_brow(NBR, NW, w, j) == r && mk_bcol(NBR, NW, w, j) == c) ++owners;
            if (owners != 1) return false;
        }
    for (int w = 0; w < NW; ++w) {
        int used = 0;
        for (int j = 0; j < mk_nslots(NBR, NW); ++j) {
            const int r = mk_brow(NBR, NW, w, j), c = mk_bcol(NBR, NW, w, j);
            if (r >= 0) {
                if (c > r || r >= NBR || used != j) return false;   // lower, in range, no gap before a used slot
                ++used;
            } else if (c != NBR) return false;
            if (j > 0 && c < mk_bcol(NBR, NW, w, j - 1)) return false;
        }
        if (used != mk_used_slots(NBR, NW, w)) return false;
    }
    return true;
}

static_assert(mk_map_ok(8, 4), "k_kal_mchol slot map, NBR 8");
static_assert(mk_map_ok(12, 4), "k_kal_mchol slot map, NBR 12");
static_assert(mk_map_ok(13, 4), "k_kal_mchol slot map, NBR 13");
static_assert(mk_map_ok(14, 4), "k_kal_mchol slot map, NBR 14");
static_assert(mk_nslots(13, 4) == 23 && mk_nslots(12, 4) == 20, "accumulators per wave of the bench's kernels");

}  // namespace msckf
