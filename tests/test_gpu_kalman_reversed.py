"""Kalman stage C in reverse pivot order (msckf_kalman.hip): C1
factors J T J, C2 solves the reversed right-hand sides and neither computes
nor stores the leading zeros of the Lc rows' solutions, E1 masks them by
index.  P+ and dx are the same quantities as in the forward order, so every
case is held against the CPU oracle at the bound of
test_kalman_cholesky_paths_vs_oracle (fp64 context: P <= 1e-9 relative,
positions to 1e-10).

Batches of 64 filters or more take the reverse order, smaller ones the forward
order (kalman_reverse_order: golden stream s4 needs the forward order's
pivots); both run the same kernels under one flag, so every case here runs
with MSCKF_KALMAN_ORDER=reverse and =forward.

Window sizes: 3 cams -- C = 18, two 16-column tiles with 14 padding columns;
10 -- C = 60; 21 / 22 -- C = 126 / 132, either side of the Cq <= 128 launch
split (k_kal_c2<7,2,8> against <13,1,12>); 30 -- C = 180, the bench window;
32 -- C = 192, a multiple of 16 (no padding column) on the 14-tile C2.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import problem_to_dict, oracle_update
from msckf_amd import synth, FilterConfig, CHI2_05
from msckf_amd._lib import Context, pack_imu, pack_cams, unpack_imu

pytestmark = pytest.mark.gpu

F = 40
_cache = {}


def problem(ncams, seed):
    """(problem, dict, oracle result) of one synthetic update, computed once."""
    key = (ncams, seed)
    if key not in _cache:
        pr = synth.make_update_problem(ncams, F, seed=seed)
        d = problem_to_dict(pr)
        _cache[key] = (pr, d, oracle_update(d))
    return _cache[key]


def imu_record(d):
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"],
                    gravity=d["gravity"], alias=True)


def set_states(ctx, items):
    for b, (pr, d, _) in enumerate(items):
        ctx.set_state(b, imu_record(d), pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P)


def load(ctx, items, chi2=None):
    feat_off = np.concatenate([[0], np.cumsum([pr.F for pr, _, _ in items])])
    obs_off, cams, zs, chi = [0], [], [], []
    for pr, _, _ in items:
        obs_off.extend(list(obs_off[-1] + pr.obs_off[1:]))
        cams.extend(pr.obs_cam)
        zs.extend(pr.obs_z)
        chi.extend(CHI2_05[m - 2] for m in pr.track_lengths())
    chi = np.array(chi) if chi2 is None else np.full(len(chi), chi2)
    ctx.batch_load(feat_off, obs_off, cams, np.array(zs), None, chi)
    return feat_off


def check_vs_oracle(ctx, items, feat_off, acc):
    for b, (pr, d, (st, acc_o, _, _, _)) in enumerate(items):
        np.testing.assert_array_equal(acc[feat_off[b]:feat_off[b + 1]], acc_o)
        imu, cams, P = ctx.get_state(b)
        err = np.linalg.norm(P - st.P) / np.linalg.norm(st.P)
        print("filter %d, %d cams: |dP|/|P| = %.2e" % (b, pr.N, err))
        assert err < 1e-9, (b, pr.N, err)
        np.testing.assert_allclose(cams[:, 4:7], np.stack([c.p for c in st.cams.values()]), atol=1e-10)
        np.testing.assert_allclose(unpack_imu(imu)["p"], st.imu.p, atol=1e-10)


ORDERS = ["reverse", "forward"]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kal", ["tiles", "mfma"])
@pytest.mark.parametrize("ncams,B", [(3, 2), (10, 3), (21, 2), (22, 2), (30, 2), (32, 1)])
def test_reversed_order_vs_oracle(ncams, B, kal, order, monkeypatch):
    """A full update at each window size where the index map can go wrong, on
    both stage C1 implementations (the capacity is the window itself)."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", kal)
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    items = [problem(ncams, 700 + b) for b in range(B)]
    ctx = Context(FilterConfig(), n_filters=B, n_cam_capacity=ncams, dtype=np.float64)
    try:
        set_states(ctx, items)
        feat_off = load(ctx, items)
        ctx.batch_update(row_cap=0, triangulate=True)
        acc = ctx.batch_results()[0]
        check_vs_oracle(ctx, items, feat_off, acc)
    finally:
        ctx.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kal", ["tiles", "mfma"])
def test_mixed_then_rotated_windows(kal, order, monkeypatch):
    """Three filters of 32, 5 and 21 cams in one context of capacity 32 (the
    reversal maps each filter's own C, not Cmax), then the same windows rotated
    twice among the slots: every slot that runs a smaller window then holds in
    its W what a larger one left there, which stage E must not read."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", kal)
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    items = [problem(32, 710), problem(5, 711), problem(21, 712)]
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=32, dtype=np.float64)
    try:
        for rot in range(3):
            cur = items[rot:] + items[:rot]   # slots hold 32, 5, 21 / 5, 21, 32 / 21, 32, 5 cams
            set_states(ctx, cur)
            feat_off = load(ctx, cur)
            ctx.batch_update(row_cap=0, triangulate=True)
            acc = ctx.batch_results()[0]
            check_vs_oracle(ctx, cur, feat_off, acc)
    finally:
        ctx.close()


def _debug(ctx, name, which=None, buf=None):
    fn = getattr(ctx.lib, name)
    if which is None:
        fn.argtypes = [C.c_void_p]
        args = ()
    else:
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_size_t]
        args = (which, buf.ctypes.data_as(C.POINTER(C.c_double)), buf.size)
    fn.restype = C.c_int
    ctx._check(fn(ctx.h, *args))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("ncams", [10, 30])
def test_stage_e_reads_only_what_c2_wrote(ncams, order, monkeypatch):
    """The Kalman stages alone, twice from the same state and H_thin; before
    the second run all of W is NaN.  C2 writes every element that E1 reads (in
    the reverse order it leaves the structural zeros unwritten and E1 masks
    them by index), so the two results are equal bit for bit and finite."""
    monkeypatch.setenv("MSCKF_KALMAN_ORDER", order)
    pr, d, _ = problem(ncams, 720)
    Cmax, Dmax = 6 * ncams, 21 + 6 * ncams
    Cp = (Cmax + 15) & ~15
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=ncams, dtype=np.float64)
    try:
        items = [(pr, d, None)]
        set_states(ctx, items)
        load(ctx, items, chi2=1e30)
        ctx.batch_update(row_cap=0, triangulate=True)
        assert ctx.batch_results()[4][0] > 0
        H = np.zeros(Cmax * (Cmax + 1))
        _debug(ctx, "msckf_debug_workspace", 6, H)
        assert np.abs(np.tril(H.reshape(Cmax, Cmax + 1)[:, :Cmax])).max() > 0   # (A is stored as its lower triangle)
        out = []
        for poison in (False, True):
            set_states(ctx, items)
            _debug(ctx, "msckf_debug_set_workspace", 6, H)
            if poison:
                _debug(ctx, "msckf_debug_set_workspace", 5, np.full((Dmax + 1) * Cp, np.nan))
            _debug(ctx, "msckf_debug_kalman")
            ctx.batch_results()
            out.append(ctx.get_state(0))
        (imu0, cams0, P0), (imu1, cams1, P1) = out
        assert np.isfinite(P0).all() and np.isfinite(P1).all()
        assert np.isfinite(imu1).all() and np.isfinite(cams1).all()
        assert not np.array_equal(P0, pr.P)   # the update did run
        np.testing.assert_array_equal(P0, P1)
        np.testing.assert_array_equal(imu0, imu1)
        np.testing.assert_array_equal(cams0, cams1)
    finally:
        ctx.close()
