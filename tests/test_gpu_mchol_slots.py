"""k_kal_mchol with compile-time slot maps (msckf_kalman.hip mk_wave,
msckf_mchol_slots.h): stage C1 runs one code path per wave and block
column and leaves its pivot loop at the first step past the filter's own window,
which can fall in the middle of a block column.  Every case runs both stages on
the matrix cores (MSCKF_KALMAN_CHOL=mfma) in an fp64 context, in both pivot
orders of stage C, against the CPU oracle at the bounds of
test_gpu_kalman_reversed.py: |dP| / |P| < 1e-9, positions to 1e-10, decisions equal.
"""
import numpy as np
import pytest

from helpers import problem_to_dict, oracle_update
from msckf_amd import synth, FilterConfig, CHI2_05
from msckf_amd._lib import Context, pack_imu, pack_cams, unpack_imu

pytestmark = pytest.mark.gpu

F = 40
ORDERS = ["reverse", "forward"]
_cache = {}


def problem(ncams, seed):
    """(problem, dict, oracle result) of one synthetic update, computed once (a window of two
    cams: every track spans both, the generator's random tracks start at three observations)."""
    key = (ncams, seed)
    if key not in _cache:
        pr = synth.make_update_problem(ncams, F, seed=seed, full_tracks=ncams < 3)
        d = problem_to_dict(pr)
        _cache[key] = (pr, d, oracle_update(d))
    return _cache[key]


def imu_record(d):
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"],
                    gravity=d["gravity"], alias=True)


def set_states(ctx, items, P_of=None):
    for b, (pr, d, _) in enumerate(items):
        P = pr.P if P_of is None or b not in P_of else P_of[b]
        ctx.set_state(b, imu_record(d), pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), P)


def load(ctx, items):
    feat_off = np.concatenate([[0], np.cumsum([pr.F for pr, _, _ in items])])
    obs_off, cams, zs, chi = [0], [], [], []
    for pr, _, _ in items:
        obs_off.extend(list(obs_off[-1] + pr.obs_off[1:]))
        cams.extend(pr.obs_cam)
        zs.extend(pr.obs_z)
        chi.extend(CHI2_05[m - 2] for m in pr.track_lengths())
    ctx.batch_load(feat_off, obs_off, cams, np.array(zs), None, np.array(chi))
    return feat_off


def check_state(ctx, b, pr, st):
    imu, cams, P = ctx.get_state(b)
    err = np.linalg.norm(P - st.P) / np.linalg.norm(st.P)
    print("filter %d, %d cams: |dP|/|P| = %.2e" % (b, pr.N, err))
    assert err < 1e-9, (b, pr.N, err)
    np.testing.assert_allclose(cams[:, 4:7], np.stack([c.p for c in st.cams.values()]), atol=1e-10)
    np.testing.assert_allclose(unpack_imu(imu)["p"], st.imu.p, atol=1e-10)


def check_vs_oracle(ctx, items, feat_off, acc):
    for b, (pr, d, (st, acc_o, _, _, _)) in enumerate(items):
        np.testing.assert_array_equal(acc[feat_off[b]:feat_off[b + 1]], acc_o)
        check_state(ctx, b, pr, st)


@pytest.mark.parametrize("order", ORDERS)
def test_windows_leaving_inside_a_block_column(order, monkeypatch):
    """One context of capacity 30 (the bench's kernels: stage A with 13 block rows, C1 with 12)
    whose five filters hold live windows of 2, 3, 7, 13 and 29 cams: Cp = 12, 20, 44, 80, 176, so
    the pivot loops leave at sc = 3, 1, 3, 0 and 0 of a block column.  Then the windows are
    rotated among the slots and updated again."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", "mfma")
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    items = [problem(n, 800 + n) for n in (2, 3, 7, 13, 29)]
    ctx = Context(FilterConfig(), n_filters=5, n_cam_capacity=30, dtype=np.float64)
    try:
        for rot in (0, 2):
            cur = items[rot:] + items[:rot]
            set_states(ctx, cur)
            feat_off = load(ctx, cur)
            ctx.batch_update(row_cap=0, triangulate=True)
            acc = ctx.batch_results()[0]
            check_vs_oracle(ctx, cur, feat_off, acc)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ncams", [29, 31])
def test_capacities_29_and_31(ncams, order, monkeypatch):
    """Capacities outside the existing sweep: stage A with 13 / 14 block rows and the IMU rows
    starting at offsets 0 / 12 of their block (Cp = 176 / 188), C1 with 12 block rows."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", "mfma")
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    items = [problem(ncams, 820 + b) for b in range(2)]
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=ncams, dtype=np.float64)
    try:
        set_states(ctx, items)
        feat_off = load(ctx, items)
        ctx.batch_update(row_cap=0, triangulate=True)
        acc = ctx.batch_results()[0]
        check_vs_oracle(ctx, items, feat_off, acc)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ORDERS)
def test_indefinite_pcc_beside_healthy_filters(order, monkeypatch):
    """Four filters of 10 cams, the third with the indefinite P_cc of
    test_update_rejects_corrupted_covariance (a negative eigenvalue of 10 x the largest cam
    variance).  The parent commit's behaviour, kept: the shifted retries cannot repair such a
    P_cc, stage A flags the filter, stage C1 skips it, and the results report rc = -3 "state
    covariance P_cc not positive definite" naming slot 2; the failed filter's covariance stays
    as it was set; the three healthy filters are updated and match the oracle.  (The decisions
    are not returned by an update that reports a failure, so the states are what is compared.)"""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", "mfma")
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    items = [problem(10, 840 + b) for b in range(4)]
    P = items[2][0].P.copy()
    v = np.zeros(P.shape[0])
    v[27:33] = 1.0 / np.sqrt(6.0)
    P -= 10.0 * np.abs(np.diag(P)[21:]).max() * np.outer(v, v)
    assert np.linalg.eigvalsh(P[21:, 21:]).min() < -1e-3 * np.abs(np.diag(P)[21:]).max()
    ctx = Context(FilterConfig(), n_filters=4, n_cam_capacity=10, dtype=np.float64)
    try:
        set_states(ctx, items, P_of={2: P})
        load(ctx, items)
        ctx.batch_update(row_cap=0, triangulate=True)
        with pytest.raises(RuntimeError, match=r"P_cc not positive definite \(filter slot 2,.*rc=-3"):
            ctx.batch_results()
        for b in (0, 1, 3):
            pr, d, (st, _, _, _, _) = items[b]
            check_state(ctx, b, pr, st)
        P_after = ctx.get_state(2)[2]
        print("failed filter: covariance unchanged:", np.array_equal(P_after, P))
        np.testing.assert_array_equal(P_after, P)
    finally:
        ctx.close()
