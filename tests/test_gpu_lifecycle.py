"""GPU parity over the filter window's life cycle (tests/lifecycle.py): the
kernels are selected by the context's cam capacity, the live window C_b = 6
n_cams grows and shrinks far below it, over stale P past D and stale
workspaces.  Every operation is compared with the oracle on the state read
back just before it, at the project's per-operation tolerances, fp64 and fp32.

Capacities and what they select (msckf_kalman.hip, launch_kalman_chol /
launch_gchol; the information assembly by Nmax):
    21   k_kal_b<8, 8> with k_kal_c2<7, 2, 8>, fused assembly
    32   k_kal_b<16, 12> with k_kal_c2<14, 1, 12> at the C = 192 edge, fused assembly
    34   the smallest global-memory window (k_gchol_*, k_kal_b1 / b2, k_kal_e), one-workgroup k_info
    52   global-memory window, multi-workgroup assembly
    128  the ABI's maximum: k_prune with R = 7 rows per chunk (fp64), D = 789 -> 261 -> 267 in ld = 789

Measured on an MI355X, worst over every step of every test here (all project
bounds unchanged and met; no defect found):
    operation                      fp64        fp32
    prune (P, cams, IMU)           bit-equal   bit-equal
    augment rel(P)                 2.6e-17     3.0e-8
    augment new cam record (abs)   5.4e-17     1.0e-7
    propagate rel(P), life cycle   5.7e-16     1.0e-6
    propagate rel(P), window sweep 1.1e-15     1.3e-6   (N = 10 | N = 0, 7 samples)
    update rel(P), caps 21..52     2.4e-14     3.0e-8
    update rel(P), cap 128         1.3e-13     2.8e-8
    update gamma (relative)        1.5e-12     5.0e-4   (fp32: printed, not bounded here; decisions identical)
    update positions (abs)         3.1e-15     --
    update corrections (relative)  2.5e-12     5.2e-5 cam (cap 128, full window), 5.0e-5 IMU (cap 21)
The fp32 correction figures are the fp32 storage of the corrected positions:
the oracle with that storage alone gives the same values to two digits
(test_lifecycle_ref.py holds them below 6e-5 for the pinned seeds).
MSCKF_KALMAN_CHOL = mfma / tiles (caps 21, 32, fp64): the same figures to the
last digit shown but gamma (7.7e-13 / 1.5e-12).  Breaking the REFERENCE instead
of a kernel (prune without the column compaction; propagation skipping the last
cam's cross block; the augment's new diagonal block off by 1 %) failed every
test here that runs that operation: 16, 46 and 34 of the 52 cases.
"""
import ctypes as C

import numpy as np
import pytest

import lifecycle as lc
from helpers import problem_to_dict, rounded
from lifecycle import (LIFECYCLE_SEEDS, WINDOW_CAPS, Lifecycle, State, cap128_script, check_augment, check_propagate,
                       check_prune, make_samples, propagate_batch_vs_oracle, start_state, window_script)
from msckf_amd import FilterConfig, synth
from msckf_amd._lib import CAM_LEN, IMU_LEN, Context, pack_cams, pack_imu

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]


def _padding_rows_are_zero(ctx, filters):
    """msckf_readback's cam output holds Nmax records per filter: those past
    n_cams are zero (the Python binding trims them, so call the ABI)."""
    fl = np.ascontiguousarray(filters, dtype=np.int32)
    n = len(fl)
    imu, cams = np.zeros((n, IMU_LEN)), np.full((n, ctx.Nmax, CAM_LEN), np.nan)
    nc = np.zeros(n, np.int32)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    ctx._check(ctx.lib.msckf_readback(ctx.h, n, fl.ctypes.data_as(ip), imu.ctypes.data_as(dp), cams.ctypes.data_as(dp),
                                      nc.ctypes.data_as(ip), 0, 0, None, None, None, None, None, None))
    for w, b in enumerate(fl):
        s = State(*ctx.get_state(int(b)))
        assert nc[w] == len(s.cams)
        np.testing.assert_array_equal(cams[w, :nc[w]], s.cams)
        np.testing.assert_array_equal(cams[w, nc[w]:], 0.0)
        np.testing.assert_array_equal(imu[w], s.imu)
    return nc


def _window(cap, dtype, name=""):
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=cap, dtype=dtype)
    try:
        L = window_script(Lifecycle(ctx, cap, dtype, 3, lc.WINDOW_FEATURES, LIFECYCLE_SEEDS[cap], name=name))
        nc = _padding_rows_are_zero(ctx, [1, 2, 0])
        assert list(nc) == [1, cap, lc.GROWTH[cap][-1]]
        print("[%s] worst: %s" % (L.name, ", ".join("%s %.3e" % kv for kv in sorted(L.worst.items()))))
        return L
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cap", WINDOW_CAPS)
def test_window_lifecycle_vs_oracle(cap, dtype, monkeypatch):
    """Three filters in one context of capacity cap (lifecycle.window_script):
    1 full-window update; 2 prune_batch to {0, last} | the odd slots | all but
    slot 0; 3 propagate_batch with 5 | 0 | 1 samples (the empty range leaves its
    filter bit-unchanged); 4 augment_batch of filters 0 and 2; 5 one batched
    update on live windows of 3 | cap // 2 | cap cams; 6 cov_diag_batch and
    readback against get_state; 7 filter 0 grown (propagate + augment) to C_b on
    either side of a 16-column tile edge and, above 32 cams, of a GNB panel
    edge, an update at each; 8 filter 1 pruned to one cam: no features, rows 0,
    state bit-unchanged while the others update.  MSCKF_KALMAN_CHOL unset: the
    Kalman stages the library picks by itself."""
    monkeypatch.delenv("MSCKF_KALMAN_CHOL", raising=False)
    _window(cap, dtype)


@pytest.mark.parametrize("kal", ["mfma", "tiles"])
@pytest.mark.parametrize("cap", [21, 32])
def test_window_lifecycle_kalman_paths(cap, kal, monkeypatch):
    """The same script on both implementations of the register-tile window's
    stages A / C1 (fp64), as test_kalman_cholesky_paths_vs_oracle forces them."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", kal)
    _window(cap, np.float64, name="cap %d float64 %s" % (cap, kal))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lifecycle_cap128(dtype):
    """One filter of capacity 128, 12 features: full update, prune to 40
    scattered slots, propagate 3 samples, augment, update."""
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=128, dtype=dtype)
    try:
        L = cap128_script(Lifecycle(ctx, 128, dtype, 1, lc.CAP128_FEATURES, LIFECYCLE_SEEDS[128]))
        assert [n for rec in L.updates for n, _, _ in rec] == [128, 41]
        print("[%s] worst: %s" % (L.name, ", ".join("%s %.3e" % kv for kv in sorted(L.worst.items()))))
    finally:
        ctx.close()


def _imu_record(d):
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"], gravity=d["gravity"], alias=True)


def _window_of(d, N):
    """The first N cams of problem d: cam arrays and the leading block of P."""
    out = dict(d)
    D = 21 + 6 * N
    out.update(N=N, cam_q=d["cam_q"][:N], cam_p=d["cam_p"][:N], cam_q_null=d["cam_q_null"][:N], P=d["P"][:D, :D].copy())
    return out


# (N, capacity): N + 0 and N + 2, at most 128 and (the ABI's minimum) at least 1
SWEEP = sorted({(N, max(1, min(128, N + extra))) for N in (0, 1, 10, 11, 22, 32, 33, 64, 128) for extra in (0, 2)})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,cap", SWEEP)
def test_propagate_window_sweep(N, cap, dtype):
    """k_propagate's MFMA cross block over 64-column chunks: windows with 6 N an
    exact multiple of 64 (N = 32, 64, 128), just past one (11, 22, 33), none and
    one cam; two filters with 1 | 7 samples in one launch; body and bounds of
    test_propagate_batch_vs_oracle.  With capacity above N (ld != D) the block
    past D holds another problem's covariance, not zeros: it must come back
    bit-unchanged (read by raising n_cams to the capacity), and the augment
    that follows must build the new row from the live window alone."""
    full = [problem_to_dict(synth.make_update_problem(max(cap, 3), 4, seed=700 + N + b)) for b in range(2)]
    full = [_window_of(d, cap) for d in full]
    if dtype == np.float32:
        full = [rounded(d) for d in full]
    ds = [_window_of(d, N) for d in full]
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=cap, dtype=dtype)
    try:
        for b, (d, f) in enumerate(zip(ds, full)):
            imu = _imu_record(d)
            ctx.set_state(b, imu, pack_cams(f["cam_q"], f["cam_p"], f["cam_q_null"]), f["P"])
            if N < cap:   # shrink the live window: P and the records past it stay
                ctx.set_state(b, imu, pack_cams(d["cam_q"], d["cam_p"], d["cam_q_null"]) if N else None, None)
            s = State(*ctx.get_state(b))
            assert len(s.cams) == N
            np.testing.assert_array_equal(s.P, d["P"])
        out = propagate_batch_vs_oracle(ctx, ds, [1, 7], dtype, seed=N)
        if N == cap:
            return
        D = 21 + 6 * N
        for b, ((_, imu, cams, P), f) in enumerate(zip(out, full)):
            ctx.set_state(b, imu, np.vstack([cams, pack_cams(f["cam_q"], f["cam_p"], f["cam_q_null"])[N:]]), None)
            P_all = ctx.get_state(b)[2]
            assert P_all.shape == f["P"].shape
            np.testing.assert_array_equal(P_all[:D, :D], P)
            np.testing.assert_array_equal(P_all[D:, :], f["P"][D:, :])
            np.testing.assert_array_equal(P_all[:, D:], f["P"][:, D:])
            ctx.set_state(b, imu, cams if N else None, None)
            before = State(*ctx.get_state(b))
            np.testing.assert_array_equal(before.P, P)
            ctx.augment(b)
            check_augment(before, State(*ctx.get_state(b)), dtype, "[N=%d cap %d filter %d]" % (N, cap, b))
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_prune_subsets_exact(dtype):
    """k_prune at capacity 34, each from the same 34-cam state: all cams, the
    first only, the last only, an unsorted list with a repeated slot -- bit-exact;
    the empty list is the benign no-op; an out-of-range slot raises and leaves
    the state bit-unchanged."""
    cap = 34
    s0, _ = start_state(cap, LIFECYCLE_SEEDS[cap], 4)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=cap, dtype=dtype)
    try:
        for rm in (list(range(cap)), [0], [cap - 1], [20, 7, 3, 7, 33, 20]):
            ctx.set_state(0, s0.imu, s0.cams, s0.P)
            before = State(*ctx.get_state(0))
            ctx.prune(0, rm)
            check_prune(before, rm, State(*ctx.get_state(0)), "[%s rm %s]" % (np.dtype(dtype).name, rm[:6]))
        ctx.set_state(0, s0.imu, s0.cams, s0.P)
        before = State(*ctx.get_state(0))
        ctx.prune(0, [])
        lc._assert_state_equal(State(*ctx.get_state(0)), before, "empty list")
        for rm in ([cap], [-1], [2, cap + 6, 5]):
            with pytest.raises(RuntimeError, match="out of range"):
                ctx.prune(0, rm)
            lc._assert_state_equal(State(*ctx.get_state(0)), before, "out of range %s" % rm)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_augment_to_capacity(dtype):
    """Capacity 5: from no cams to five, a few samples then a clone, each step
    against the oracle; the sixth augment raises and changes nothing."""
    cap = 5
    s0, _ = start_state(cap, LIFECYCLE_SEEDS[21], 4)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=cap, dtype=dtype)
    name = np.dtype(dtype).name
    try:
        ctx.set_state(0, s0.imu, None, s0.P[:21, :21])
        for n in range(cap):
            before = State(*ctx.get_state(0))
            assert len(before.cams) == n and before.P.shape == (21 + 6 * n,) * 2
            dt, gyro, acc = make_samples(before, 2, (cap, n))
            if dtype == np.float32:
                dt, gyro, acc = (a.astype(np.float32).astype(float) for a in (dt, gyro, acc))
            ctx.propagate(0, dt, gyro, acc)
            mid = State(*ctx.get_state(0))
            check_propagate(before, dt, gyro, acc, mid, dtype, "[%s n=%d]" % (name, n))
            ctx.augment(0)
            check_augment(mid, State(*ctx.get_state(0)), dtype, "[%s n=%d]" % (name, n))
        full = State(*ctx.get_state(0))
        assert len(full.cams) == cap
        with pytest.raises(RuntimeError, match="capacity 5 exhausted"):
            ctx.augment(0)
        with pytest.raises(RuntimeError, match="capacity 5 exhausted"):
            ctx.augment_batch([0])
        after = State(*ctx.get_state(0))
        assert len(after.cams) == cap
        lc._assert_state_equal(after, full, "after the refused augment")
    finally:
        ctx.close()
