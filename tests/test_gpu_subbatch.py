"""The update chain as two lanes (csrc/msckf_subbatch.h: filters [0, B / 2) and
the rest, each lane's chain on streams of its own) against the same chain as one
lane.  A lane runs the kernels the whole batch runs on the same per-filter and
per-feature data, so every comparison here is bitwise: MSCKF_SUBBATCH=2 against
MSCKF_SUBBATCH=1 on fresh contexts -- accepted, gamma, p_w, valid, rows and the
state of every filter.  Every run also asks the library how many lanes its
last chain ran as (msckf_debug_lanes), so a comparison cannot pass because the
split was never taken."""
import ctypes
import dataclasses

import numpy as np
import pytest

from conftest import golden, rel
from helpers import problem_to_dict, feature_obs, oracle_update
from msckf_amd import synth, FilterConfig, CHI2_05
from msckf_amd._lib import Context, pack_imu, pack_cams

pytestmark = pytest.mark.gpu

STAGES = ["restore", "triangulate", "kalman_a", "feature_jacobian", "gate", "select", "compress", "kalman_b",
          "kalman_c", "kalman_e", "kalman_correct"]


def imu_record(d):
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"], gravity=d["gravity"], alias=True)


def with_short_tracks(pr):
    """Every fifth feature of the problem cut to its first two observations
    (synth draws track lengths from 3 up)."""
    keep = np.concatenate([np.arange(a, a + (2 if f % 5 == 0 else b - a))
                           for f, (a, b) in enumerate(zip(pr.obs_off[:-1], pr.obs_off[1:]))])
    M = np.where(np.arange(pr.F) % 5 == 0, 2, np.diff(pr.obs_off))
    off = np.concatenate([[0], np.cumsum(M)]).astype(np.int32)
    return dataclasses.replace(pr, obs_off=off, obs_cam=pr.obs_cam[keep], obs_z=pr.obs_z[keep])


def first_features(pr, n):
    """The problem with its first n features only (n = 0: a filter without features)."""
    k = int(pr.obs_off[n])
    return dataclasses.replace(pr, F=n, landmarks=pr.landmarks[:n], obs_off=pr.obs_off[:n + 1],
                               obs_cam=pr.obs_cam[:k], obs_z=pr.obs_z[:k])


def make_ctx(problems, dtype):
    ctx = Context(FilterConfig(), n_filters=len(problems), n_cam_capacity=max(p.N for p in problems) + 2, dtype=dtype)
    for b, p in enumerate(problems):
        ctx.set_state(b, imu_record(problem_to_dict(p)), pack_cams(p.cam_q, p.cam_p, p.cam_q_null), p.P)
    return ctx


def load(ctx, problems, given_positions=False):
    feat_off = np.concatenate([[0], np.cumsum([p.F for p in problems])])
    obs_off = np.concatenate([[0], np.cumsum(np.concatenate([p.track_lengths() for p in problems]))])
    cams = np.concatenate([p.obs_cam for p in problems])
    zs = np.concatenate([p.obs_z for p in problems])
    chi = np.array([CHI2_05[m - 2] for p in problems for m in p.track_lengths()])
    pw = np.concatenate([p.landmarks for p in problems]) if given_positions else None
    ctx.batch_load(feat_off, obs_off, cams, zs, pw, chi)
    return feat_off


def lanes_of(ctx):
    """Lanes of the context's last restore / update chain (debug hook of the library)."""
    fn = ctx.lib.msckf_debug_lanes
    fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
    return ctx._check(fn(ctx.h))


def states(ctx):
    return [ctx.get_state(b) for b in range(ctx.B)]


def run_update(monkeypatch, lanes, problems, dtype, triangulate=True, row_cap=0):
    monkeypatch.setenv("MSCKF_SUBBATCH", str(lanes))
    ctx = make_ctx(problems, dtype)
    try:
        load(ctx, problems, given_positions=not triangulate)
        ctx.batch_update(row_cap=row_cap, triangulate=triangulate)
        assert lanes_of(ctx) == lanes
        return ctx.batch_results(), states(ctx)
    finally:
        ctx.close()


def assert_same(got, want):
    (res_g, st_g), (res_w, st_w) = got, want
    for name, a, b in zip(("accepted", "gamma", "p_w", "valid", "rows"), res_g, res_w):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert len(st_g) == len(st_w)
    for b, (sg, sw) in enumerate(zip(st_g, st_w)):
        for name, x, y in zip(("imu", "cams", "P"), sg, sw):
            np.testing.assert_array_equal(x, y, err_msg="%s of filter %d" % (name, b))


@pytest.fixture(scope="module")
def mixed():
    """B = 5 (odd: lanes of 2 and 3 filters), 8 cams, 20 features per filter with
    tracks of 2 .. 8 observations; filter 3 -- in lane 1 -- has no features."""
    problems = [with_short_tracks(synth.make_update_problem(8, 20, seed=500 + b)) for b in range(5)]
    problems[3] = first_features(problems[3], 0)
    M = np.concatenate([p.track_lengths() for p in problems])
    assert M.min() == 2 and M.max() == 8
    return problems


@pytest.mark.parametrize("row_cap", [0, 40])
@pytest.mark.parametrize("triangulate", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_mixed_batch(mixed, dtype, triangulate, row_cap, monkeypatch):
    two = run_update(monkeypatch, 2, mixed, dtype, triangulate, row_cap)
    one = run_update(monkeypatch, 1, mixed, dtype, triangulate, row_cap)
    assert_same(two, one)
    rows = two[0][4]
    assert rows[3] == 0 and (np.delete(rows, 3) > 0).all()
    if row_cap:   # the cap bites: a feature is stacked while the rows before it are within the cap, so a
        # filter ends at most one track (4 * 8 - 3 rows) past it -- and without the cap stacks more
        assert (rows <= row_cap + 29).all()
        free = run_update(monkeypatch, 2, mixed, dtype, triangulate, 0)[0][4]
        assert (np.delete(free, 3) > np.delete(rows, 3)).all()


def test_small_mixed_batch_vs_oracle(mixed, monkeypatch):
    (acc, gam, pw, valid, rows), st = run_update(monkeypatch, 2, mixed, np.float64)
    feat_off = np.concatenate([[0], np.cumsum([p.F for p in mixed])])
    for b, p in enumerate(mixed):
        ref, acc_o, tri_p, tri_ok, _ = oracle_update(problem_to_dict(p))
        sl = slice(feat_off[b], feat_off[b + 1])
        np.testing.assert_array_equal(valid[sl], tri_ok)
        np.testing.assert_array_equal(acc[sl], acc_o)
        assert rel(st[b][2], ref.P) < 1e-9, b


def test_path_choice_is_the_whole_batch(monkeypatch):
    """B = 96: the halves of 48 fall below the 64 filters from which the Kalman
    stages A / C1 run on the matrix cores, so a choice made per lane would take
    the register-tile Cholesky and differ in the last bits."""
    problems = [synth.make_update_problem(6, 8, seed=700 + b) for b in range(96)]
    assert_same(run_update(monkeypatch, 2, problems, np.float64), run_update(monkeypatch, 1, problems, np.float64))


def test_empty_second_lane(monkeypatch):
    problems = [synth.make_update_problem(8, 12, seed=800 + b) for b in range(4)]
    problems[2], problems[3] = first_features(problems[2], 0), first_features(problems[3], 0)
    two = run_update(monkeypatch, 2, problems, np.float32)
    assert_same(two, run_update(monkeypatch, 1, problems, np.float32))
    assert (two[0][4][:2] > 0).all() and (two[0][4][2:] == 0).all()
    for b in (2, 3):   # untouched
        np.testing.assert_array_equal(two[1][b][2], problems[b].P.astype(np.float32).astype(np.float64))


def test_ordering_without_host_sync(monkeypatch):
    """restore -> update -> restore -> update on the lanes' own streams, then
    set_state of a lane-1 filter and a propagation of every filter on the
    context's stream, with no synchronisation in between: the single-stream
    calls must be ordered after lane 1's work and the next laned call after them."""
    problems = [synth.make_update_problem(8, 12, seed=900 + b) for b in range(4)]
    other = synth.make_update_problem(8, 12, seed=950)
    rng = np.random.default_rng(5)
    n = 6
    dt, gyro, acc = np.full(4 * n, 0.005), 0.1 * rng.standard_normal((4 * n, 3)), rng.standard_normal((4 * n, 3))

    def run(lanes):
        monkeypatch.setenv("MSCKF_SUBBATCH", str(lanes))
        ctx = make_ctx(problems, np.float64)
        try:
            load(ctx, problems)
            ctx.snapshot()
            for _ in range(2):
                ctx.restore()
                assert lanes_of(ctx) == lanes
                ctx.batch_update(row_cap=0, triangulate=True)
                assert lanes_of(ctx) == lanes
            ctx.set_state(3, imu_record(problem_to_dict(other)), pack_cams(other.cam_q, other.cam_p, other.cam_q_null),
                          other.P)
            ctx.propagate_batch(np.arange(4), np.arange(5) * n, dt, gyro, acc)
            st = states(ctx)
            return ctx.batch_results(), st
        finally:
            ctx.close()

    two = run(2)
    assert_same(two, run(1))
    assert_same(two, run(2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_single_filter_update_of_a_lane1_filter(dtype, monkeypatch):
    """msckf_update (Context.update) enqueues the chain and reads the results in
    one call: under a split the read, on the context's stream, must wait for lane
    1.  B = 3, the updated filter is slot 2 (lane 1 = slots 1 and 2); the other
    filters have no features and must stay as they were."""
    problems = [synth.make_update_problem(8, 24, seed=1100 + b) for b in range(3)]
    p = problems[2]
    chi = np.array([CHI2_05[m - 2] for m in p.track_lengths()])

    def run(lanes):
        monkeypatch.setenv("MSCKF_SUBBATCH", str(lanes))
        ctx = make_ctx(problems, dtype)
        try:
            out = [ctx.update(2, p.obs_off, p.obs_cam, p.obs_z, p.landmarks, chi) for _ in range(2)]
            assert lanes_of(ctx) == lanes
            return out, states(ctx)
        finally:
            ctx.close()

    (two, st2), (one, st1) = run(2), run(1)
    for (a2, g2, r2), (a1, g1, r1) in zip(two, one):
        np.testing.assert_array_equal(a2, a1)
        np.testing.assert_array_equal(g2, g1)
        assert r2 == r1 and r2 > 0 and a2.any()
    for b in range(3):
        for x, y in zip(st2[b], st1[b]):
            np.testing.assert_array_equal(x, y)


def test_profiling_accounting(monkeypatch):
    """Profiling every stage runs one lane (a stage's time stays its uncontended
    time) and reports every stage once per call; profiling one stage keeps the
    lanes and reports the sum of their intervals."""
    monkeypatch.setenv("MSCKF_SUBBATCH", "2")
    problems = [synth.make_update_problem(8, 12, seed=1000 + b) for b in range(4)]
    ctx = make_ctx(problems, np.float32)
    try:
        load(ctx, problems)
        ctx.snapshot()
        k = 3
        ctx.set_profiling(True)
        for _ in range(k):
            ctx.restore()
            ctx.batch_update(row_cap=0, triangulate=True)
        ctx.sync()
        assert lanes_of(ctx) == 1
        times = ctx.kernel_times()
        assert sorted(times) == sorted(STAGES)
        for name in STAGES:
            assert times[name][1] == k and times[name][0] > 0, (name, times[name])
        ctx.set_profiling(False)
        ctx.set_profiling_stage("gate")
        for _ in range(k):
            ctx.restore()
            ctx.batch_update(row_cap=0, triangulate=True)
        ctx.sync()
        assert lanes_of(ctx) == 2
        times = ctx.kernel_times()
        assert list(times) == ["gate"] and times["gate"][0] > 0 and times["gate"][1] == k
        ctx.set_profiling(False)
    finally:
        ctx.close()


def test_failure_names_the_absolute_slot(monkeypatch):
    """The input of test_update_rejects_corrupted_covariance (test_gpu_parity.py),
    the indefinite P_cc in filter 2 of 3 -- lane 1 holds filters 1 and 2, so the
    failing filter is lane 1's local slot 1."""
    monkeypatch.setenv("MSCKF_SUBBATCH", "2")
    d = golden("update_n10_f40")
    bad = d["P"].copy()
    v = np.zeros(bad.shape[0])
    v[27:33] = 1.0 / np.sqrt(6.0)
    bad -= 10.0 * np.abs(np.diag(bad)[21:]).max() * np.outer(v, v)
    sel = [f for f in range(int(d["F"])) if d["tri_ok"][f]]
    obs = [feature_obs(d, f) for f in sel]
    M = [len(o) for o in obs]
    nobs = sum(M)
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=int(d["N"]) + 2)
    try:
        for b in range(3):
            ctx.set_state(b, imu_record(d), pack_cams(d["cam_q"], d["cam_p"], d["cam_q_null"]), bad if b == 2 else d["P"])
        cams = [c for o in obs for c, _ in o] * 3
        zs = np.array([z for o in obs for _, z in o] * 3)
        ctx.batch_load(np.arange(4) * len(sel), np.concatenate([[0], np.cumsum(M * 3)]), cams, zs,
                       np.tile(d["tri_p"][sel], (3, 1)), np.full(3 * len(sel), 1e30))
        assert len(cams) == 3 * nobs
        ctx.batch_update(row_cap=0, triangulate=False)
        with pytest.raises(RuntimeError, match=r"filter slot 2,.*rc=-3"):
            ctx.batch_results()
    finally:
        ctx.close()
