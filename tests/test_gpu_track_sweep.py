"""GPU parity sweep over every track length: one feature for every observation
count M = 2 .. N through the batched update (tests/track_sweep.py), on the
window sizes N = 128 (the ABI's maximum: D = 789, cam masks up to bit 127, the
global-memory Kalman stages, k_info_big, every gate route) and N = 32 (the
largest register-tile Kalman window), fp64 and fp32, against the CPU oracle.

Gate routes (csrc/msckf_gate_routes.h: one feature list per block count nb =
ceil((3M + 4) / 16) up to M = 82, one beyond) and the kernel of each; the
results are grouped with 41 apart, in the device's list of 37..40:

    M            nb      fp32                       fp64
    2..4 .. 31..36  1..7   k_gate_mfma<nb> (one wave) k_gate_mfma<nb> (one wave, fp64 MFMA)
    37..40       8       k_gate_mfma<8>             k_gate_mfma_wt<8, 4>
    41           8       k_gate_mfma<8> (same list) k_gate_mfma_wt<8, 4> (same list)
    42..46       9       k_gate_mfma_wt<9, 2>       k_gate_mfma_wt<9, 4>
    47..52       10      k_gate_mfma_wt<10, 2>      k_gate_mfma_wt<10, 4>
    53..57       11      k_gate_mfma_wt<11, 2>      k_gate_mfma_wt<11, 8>
    58..62 .. 74..78  12..15  k_gate_mfma_wt<nb, 4>  k_gate_mfma_wt<nb, 8>
    79..82       16      k_gate_mfma_wt<16, 8>      k_gate_mfma_wt<16, 8>
    83..128      --      k_gate (global memory)     k_gate (global memory)

Triangulation and Jacobians run in the SegClasses lanes S = 8, 16, 32, 64, 128
(M = 8|9, 16|17, 32|33, 64|65 and 128 are all present).
"""
import time

import numpy as np
import pytest

from helpers import oracle_update, problem_to_dict, rounded
from track_sweep import (SWEEP_SEEDS, cached_sweep, check_sweep, route_name, route_worst, scrambled, state_arrays)
from msckf_amd import FilterConfig
from msckf_amd._lib import Context, pack_imu, pack_cams, unpack_imu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[128, 32])
def window(request):
    """(N, [(problem, reference)] of filter 0 (seed, flip 0) and filter 1
    (seed + 1, flip 1)): the oracle runs once per (N, seed, flip) and process."""
    N = request.param
    return N, [cached_sweep(N, SWEEP_SEEDS[N] + flip, flip) for flip in (0, 1)]


def _set_state(ctx, b, pr):
    d = problem_to_dict(pr)
    imu = pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                   q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                   R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"], gravity=d["gravity"], alias=True)
    ctx.set_state(b, imu, pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P)


def _run(ctx, B, items, triangulate, snapshot=False):
    """Loads the features of ``items`` = {filter slot: (problem, chi2, p_w or
    None)} (the other slots get an empty slice), takes the snapshot if asked,
    runs the update and returns {slot: got dict for check_sweep}, the raw
    result arrays and the wall time of load + update + results."""
    feat_off, obs_off, cams, zs, chi, pws = [0], [0], [], [], [], []
    for b in range(B):
        if b in items:
            pr, chi2, p_w = items[b]
            obs_off.extend(list(obs_off[-1] + pr.obs_off[1:]))
            cams.extend(pr.obs_cam)
            zs.extend(pr.obs_z)
            chi.extend(chi2)
            pws.append(p_w)
        feat_off.append(len(chi))
    p_w = None if triangulate else np.concatenate(pws)
    t0 = time.perf_counter()
    ctx.batch_load(feat_off, obs_off, cams, np.array(zs), p_w, np.array(chi))
    if snapshot:
        ctx.snapshot()
    ctx.batch_update(row_cap=0, triangulate=triangulate)
    acc, gam, pw, valid, rows = ctx.batch_results()
    dt = time.perf_counter() - t0
    got = {}
    for b in range(B):
        sl = slice(feat_off[b], feat_off[b + 1])
        imu, cam, P = ctx.get_state(b)
        got[b] = dict(valid=valid[sl], p_w=pw[sl], gamma=gam[sl], accept=acc[sl], rows=int(rows[b]), P=P,
                      cam_p=cam[:, 4:7], imu_p=unpack_imu(imu)["p"])
    return got, (acc, gam, pw, valid, rows), dt


def _check(ref, got, dtype, label, pr):
    """check_sweep; fp32: against the oracle rerun from the problem rounded to
    fp32 on the device's own positions and decisions, with the fp32 sigma2
    (check_fp32_batch, part 2).  Prints the measured figures before asserting."""
    state = None
    if dtype == np.float32:
        d32 = rounded(problem_to_dict(pr))
        s2 = float(np.float32(FilterConfig().observation_noise))
        st = oracle_update(d32, tri=(got["p_w"], got["valid"]), accept=got["accept"] & got["valid"], sigma2=s2)[0]
        state = state_arrays(st) + (d32["cam_p"], d32["imu_p"])
    P_ref = ref.P if state is None else state[0]
    worst = route_worst(ref, got)
    print("%s: rel(P) %.3e, invalid %d, worst gamma error per route: %s"
          % (label, np.linalg.norm(got["P"] - P_ref) / np.linalg.norm(P_ref), int((~got["valid"]).sum()),
             ", ".join("%s %.2e" % (route_name(r), e) for r, e in sorted(worst.items()))))
    return check_sweep(ref, got, dtype, label, state=state)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_track_sweep_vs_oracle(window, dtype):
    """One context, two filters with different states, three steps.

    1. Both filters hold a sweep (flip 0 / flip 1: contiguous and gapped tracks
       and accepted and rejected features alternate, thresholds at 2 x / 0.5 x
       the oracle's gamma so fp32 decisions must be exact too); triangulation on
       the device.
    2. After restore(): only filter 1's features, observation order scrambled,
       positions given by the host (the oracle's).  gamma is invariant under the
       permutation, so the sorted-order reference holds; filter 0 (an empty
       slice) must keep the snapshot's P bit for bit; every decision sits at
       another feature index than in step 1, so values left over from step 1
       cannot pass.
    3. fp64: step 1 again after restore() is bit-identical to step 1.

    Bounds: check_sweep (the project's: fp64 gamma rtol 1e-9 for every feature,
    rel(P) < 1e-9; fp32 gamma median < 1e-4 and p99 < 1e-3 per filter, median
    < 1e-4 per route, rel(P) < 1e-5, position corrections < 1e-4) plus the fp32
    per-feature cap FP32_GAMMA_CAP = 10 x the worst relative gamma error
    measured on an MI355X over both windows and steps 1 and 2 (step 3 is fp64).

    Measured on an MI355X (N = 128 and 32, both filters, steps 1 and 2), worst
    relative gamma error per route; every project bound passed unchanged:
      fp32  M=2..4 2.6e-5, 5..9 8.6e-5, 10..14 1.9e-5, 15..20 1.4e-5, 21..25 1.3e-5,
            26..30 2.0e-5, 31..36 1.9e-5, 37..40 6.4e-6, 41 1.5e-6, 42..46 1.1e-5,
            47..52 2.0e-5, 53..57 7.1e-6, 58..62 4.6e-5, 63..68 9.0e-6, 69..73 9.0e-5,
            74..78 6.4e-6, 79..82 3.4e-5, 83..128 8.2e-5; worst 8.96e-5, so
            FP32_GAMMA_CAP = 9.0e-4.  No route stands out from its neighbours.
      fp64  worst 2.4e-13 (M=83..128, k_gate); every other route <= 1.8e-13.
      rel(P): N = 128 fp64 6.9e-13, fp32 2.6e-8; N = 32 fp64 4.6e-14, fp32 2.7e-8.
      No fp32 feature came back invalid.  Load + update + results: 0.07 s per
      step at N = 128, 1 ms at N = 32; the module's ~9 s are the CPU oracle.
    The sweep found stage C2 of the register-tile Kalman window (k_kal_c2) one
    16-row tile short with 32 live cams in capacity 32: rel(P) 0.19 before the
    fix at N = 32 in fp64 (the fp32 context runs the same fp64 stages;
    launch_kalman_chol).
    """
    N, filters = window
    (pr0, ref0), (pr1, ref1) = filters
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=N, dtype=dtype)
    try:
        _set_state(ctx, 0, pr0)
        _set_state(ctx, 1, pr1)
        P0_before = ctx.get_state(0)[2]
        name = "N=%d %s" % (N, np.dtype(dtype).name)
        items = {0: (pr0, ref0.chi2, None), 1: (pr1, ref1.chi2, None)}
        got1, raw1, dt1 = _run(ctx, 2, items, triangulate=True, snapshot=True)
        for b, (pr, ref) in enumerate(filters):
            _check(ref, got1[b], dtype, "%s step 1 filter %d" % (name, b), pr)

        ctx.restore()
        sc1 = scrambled(pr1)
        got2, raw2, dt2 = _run(ctx, 2, {1: (sc1, ref1.chi2, ref1.tri_p)}, triangulate=False)
        assert got2[0]["rows"] == 0 and len(got2[0]["gamma"]) == 0
        np.testing.assert_array_equal(got2[0]["P"], P0_before)
        np.testing.assert_array_equal(got2[1]["valid"], np.ones(pr1.F, bool))
        _check(ref1, got2[1], dtype, "%s step 2 filter 1" % name, sc1)
        print("%s: load + update + results %.3f s (step 1), %.3f s (step 2)" % (name, dt1, dt2))

        if dtype == np.float64:
            ctx.restore()
            got3, raw3, _ = _run(ctx, 2, items, triangulate=True)
            for a, b in zip(raw1, raw3):
                np.testing.assert_array_equal(a, b)
            for b in range(2):
                for key in ("P", "cam_p", "imu_p"):
                    np.testing.assert_array_equal(got1[b][key], got3[b][key])
    finally:
        ctx.close()
