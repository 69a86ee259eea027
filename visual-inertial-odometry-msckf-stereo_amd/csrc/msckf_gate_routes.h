// msckf_gate_routes.h -- which gating kernel takes a track of M observations.
// The one table behind load_features' feature lists, launch_gate's loop and the
// dispatcher of msckf_gate_mfma.hip.  Plain C++17, no HIP include: a host
// compiler builds it alone (tests/test_track_sweep_ref.py prints it).
#pragma once

namespace msckf {

// The MFMA tile kernels eliminate a (3M + 4)-square matrix in 16-row blocks.
constexpr int gate_nb(int M) { return (3 * M + 4 + 15) / 16; }
// Longest track on the tile kernels; M >= 83 goes to the global-memory kernel
// k_gate, which reads k_feature's compact QR factors and the (4M)^2 scratch.
constexpr int GATE_TILE_MAXM = 82;
constexpr int GATE_NB_MAX = gate_nb(GATE_TILE_MAXM);   // 16
// Feature lists: list nb - 1 holds the tracks of exactly nb blocks (M <= 82),
// so its kernel has a compile-time block count; the last list holds M >= 83.
constexpr int GATE_NLIST = GATE_NB_MAX + 1;
constexpr int GATE_LIST_GLOBAL = GATE_NLIST - 1;
constexpr int gate_list_of(int M) { return M <= GATE_TILE_MAXM ? gate_nb(M) - 1 : GATE_LIST_GLOBAL; }

enum class GateKind { OneWave, Workgroup, Global };
struct GateRoute {
    GateKind kind;
    int waves;   // per feature
};
// OneWave: k_gate_mfma<nb>.  fp64 stops at 7 blocks, the accumulators of 8 would
// spill; fp32 lists of 7 / 8 blocks on two waves measured slower (50x400 gate
// 12.05 -> 12.39 ms, profiles/r06/wt2/).
// Workgroup: k_gate_mfma_wt<nb, waves>.  fp32 (profiles/r06/wt/, 80x1000): two
// waves beat four for nb <= 11 (1.07 / 1.62 / 1.55 against 1.16 / 2.21 / 1.91 ms)
// but spill at nb = 12; eight keep nb = 16 off scratch (2.34 ms against 7.93) and
// lose to four below it.  fp64 (8 VGPRs per accumulator block, profiles/r06/wt64/):
// 50x400 gate 42.8 ms with eight waves for every count, 32.2 with four up to 10.
constexpr GateRoute gate_route(int list, int scalar_bytes) {
    const int nb = list + 1;
    if (list >= GATE_LIST_GLOBAL) return {GateKind::Global, 4};   // k_gate: 256 threads
    if (scalar_bytes == 4)
        return nb <= 8 ? GateRoute{GateKind::OneWave, 1}
                       : GateRoute{GateKind::Workgroup, nb <= 11 ? 2 : (nb <= 15 ? 4 : 8)};
    return nb <= 7 ? GateRoute{GateKind::OneWave, 1} : GateRoute{GateKind::Workgroup, nb <= 10 ? 4 : 8};
}

constexpr bool gate_tile_lists_routed() {
    for (int ts = 4; ts <= 8; ts += 4)
        for (int l = 0; l < GATE_LIST_GLOBAL; ++l)
            if (gate_route(l, ts).kind == GateKind::Global) return false;
    return true;
}
static_assert(gate_tile_lists_routed(), "every block-count list needs a tile kernel in both precisions");

}  // namespace msckf
