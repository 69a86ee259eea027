"""The vision standstill cue (include/msckf_standstill.h) on the GPU against its
numpy restatement tests/standstill_ref.py: the motion statistic as a set call
and inside the tracked frame, the cued zero-velocity update from host arrays
and from the front-end's records on the device, and StereoVIO with
ZuptConfig(vision=VisionCue(...)) under both hand-offs.

The statistic is compared bit for bit (it is a selection among float32 values
formed by three rounded operations); the cued update's state and covariance are
held to tests/test_gpu_zupt.py's bounds for the same scalar, its decisions and
records exactly; a filter that is not applied keeps every byte.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import msckf_amd
import msckf_amd.frontend as fe_mod
from msckf_amd import FilterConfig, VisionCue, ZuptConfig, _lib
from msckf_amd._lib import Context, MsckfZuptCueT, MsckfZuptParamsT
from msckf_amd.scheduler import MultiMSCKF, StereoVIO
from conftest import golden
from frontend_ref_scenes import ImgMsg, ImuMsg, StereoMsg, scene_config
from lifecycle import State, oracle_of
import frontend_synth as fs
import frontend_tracks_ref as tr
import standstill_ref as S
import zupt_ref as Z
import test_gpu_tracks as tt
from test_gpu_zupt import check_against, means, problem, put, same_state

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 0, 4096, 0]   # an empty set between two full ones, one at the end
QS = [0.0, 0.5, 0.9, 1.0]


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# --------------------------------------------------------- mfe_motion_sets --
def _grid(n, rng):
    """prev on a quarter-pixel grid, so that a quarter-pixel displacement is exact in float32."""
    return (rng.integers(0, 4 * 4000, (n, 2)) / 4.0).astype(np.float32)


def pat_all_equal(n, rng):
    p = _grid(n, rng)
    return p, p + np.float32([3.25, 1.5])


def pat_zero(n, rng):
    p = rng.uniform(0, 8192, (n, 2)).astype(np.float32)
    return p, p.copy()


def pat_ties(n, rng):
    """Three values of d2 in long runs: rank k falls inside a run of equal values."""
    p = _grid(n, rng)
    d = np.zeros((n, 2), np.float32)
    d[:, 0] = rng.integers(0, 3, n)
    return p, p + d


def pat_ascending(n, rng):
    p = np.zeros((n, 2), np.float32)
    c = p.copy()
    c[:, 0] = 0.5 * np.arange(n)
    return p, c


def pat_descending(n, rng):
    p, c = pat_ascending(n, rng)
    return p, c[::-1].copy()


def pat_outlier(n, rng):
    p = _grid(n, rng)
    c = p.copy()
    if n:
        p[n // 3], c[n // 3] = (0.0, 0.0), (8191.0, 8191.0)
    return p, c


def pat_ulp(n, rng):
    """Displacements that are consecutive float32 values, shuffled."""
    p = np.zeros((n, 2), np.float32)
    c = p.copy()
    x = np.float32(1000.0)
    vals = []
    for _ in range(n):
        vals.append(x)
        x = np.nextafter(x, np.float32(np.inf))
    c[:, 0] = rng.permutation(np.array(vals, np.float32)) if n else []
    return p, c


def pat_random(n, rng):
    return rng.uniform(0, 8192, (n, 2)).astype(np.float32), rng.uniform(0, 8192, (n, 2)).astype(np.float32)


PATTERNS = dict(all_equal=pat_all_equal, zero=pat_zero, ties=pat_ties, ascending=pat_ascending,
                descending=pat_descending, outlier=pat_outlier, ulp=pat_ulp, random=pat_random)


@pytest.fixture(scope="module")
def small_fe():
    fe = fe_mod.Frontend(32, 32, nslot=1, max_level=0, max_points=8192)
    yield fe
    fe.close()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_motion_sets_equal_numpy_bit_for_bit(small_fe, pattern):
    rng = np.random.default_rng(sorted(PATTERNS).index(pattern))
    sets = [PATTERNS[pattern](n, rng) for n in SIZES]
    for p, c in sets:
        assert p.dtype == c.dtype == np.float32 and (p >= 0).all() and (c < 8192).all() and (p < 8192).all()
    for q in QS:
        want = [S.motion_stat(p, c, q) for p, c in sets]
        n, d2 = small_fe.motion_sets(sets, q)
        assert n.tolist() == SIZES == [w[0] for w in want]
        wd = np.array([w[1] for w in want], np.float32)
        empty = np.array(SIZES) == 0
        assert np.isnan(d2[empty]).all() and np.isnan(wd[empty]).all()
        np.testing.assert_array_equal(bits(d2[~empty]), bits(wd[~empty]), err_msg="q = %g" % q)
        n2, d22 = small_fe.motion_sets(sets, q)                  # a repeat gives the same bits
        assert n2.tolist() == n.tolist() and bits(d22).tolist() == bits(d2).tolist()
    if pattern == "ties":   # the scenario's condition: rank k lies strictly inside a run of equal values
        d = np.sort(S.motion_d2(*sets[SIZES.index(1000)]))
        k = S.motion_k(1000, 0.5)
        assert d[k - 1] == d[k] == d[k + 1]


def _raw_motion_sets(fe, n_sets, off, prev, curr, q, n_out, d2_out):
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    return fe.lib.mfe_motion_sets(fe.h, n_sets, ptr(off, C.c_int32), ptr(prev, C.c_float), ptr(curr, C.c_float),
                                  C.c_double(q), ptr(n_out, C.c_int32), ptr(d2_out, C.c_float))


def test_motion_sets_argument_errors_leave_the_outputs(small_fe):
    rng = np.random.default_rng(5)
    off = np.array([0, 3, 3, 8], np.int32)
    prev, curr = pat_random(8, rng)
    n_out, d2_out = np.full(3, 77, np.int32), np.full(3, 7.5, np.float32)
    big = np.array([0, 4097], np.int32)
    big_pts = np.zeros((4097, 2), np.float32)
    inf, nan = prev.copy(), curr.copy()
    inf[4, 1], nan[7, 0] = np.inf, np.nan
    bad = [
        (3, None, prev, curr, 0.5, n_out, d2_out), (3, off, None, curr, 0.5, n_out, d2_out),
        (3, off, prev, None, 0.5, n_out, d2_out), (3, off, prev, curr, 0.5, None, d2_out),
        (3, off, prev, curr, 0.5, n_out, None),
        (3, off, prev, curr, -0.1, n_out, d2_out), (3, off, prev, curr, 1.1, n_out, d2_out),
        (3, off, prev, curr, float("nan"), n_out, d2_out),
        (3, np.array([0, 5, 3, 8], np.int32), prev, curr, 0.5, n_out, d2_out),      # not monotone
        (3, np.array([1, 3, 3, 8], np.int32), prev, curr, 0.5, n_out, d2_out),      # does not start at 0
        (1, big, big_pts, big_pts, 0.5, n_out, d2_out),                             # a set above 4096
        (3, off, inf, curr, 0.5, n_out, d2_out), (3, off, prev, nan, 0.5, n_out, d2_out),
        (-1, off, prev, curr, 0.5, n_out, d2_out),
    ]
    for k, args in enumerate(bad):
        assert _raw_motion_sets(small_fe, *args) == -1, k
        assert (n_out == 77).all() and (d2_out == 7.5).all(), k
    assert _raw_motion_sets(small_fe, 3, off, prev, curr, 0.5, n_out, d2_out) == 0
    assert n_out.tolist() == [3, 0, 5] and np.isnan(d2_out[1])


# ---------------------------------------------------------------- the step --
GRID, CAP = (4, 5, 3, 5), 485                      # cap >= 420 + 20 * 3 and no multiple of 256
LANES = [(420, 0, False, 33), (40, 1, True, 35)]   # (rows, camera kind, RANSAC, texture seed), as test_gpu_tracks.py's


class _Spy:
    """The operator object with the occupied lists of fast_grid_sets kept: step 6 receives
    exactly the tracked cam0 points of step 4's survivors."""

    def __init__(self, fe):
        self._fe, self.occupied = fe, None

    def __getattr__(self, name):
        return getattr(self._fe, name)

    def fast_grid_sets(self, sets, *a, **kw):
        self.occupied = [np.asarray(s[1], np.float32).reshape(-1, 2).copy() for s in sets]
        return self._fe.fast_grid_sets(sets, *a, **kw)


def _survivor_stat(table, trace, occupied, i, q):
    keep = trace["keep", i]
    rows = np.nonzero(keep[0])[0]
    rows = rows[keep[1]]
    rows = rows[keep[2]]
    assert len(rows) == len(occupied)
    return S.motion_stat(table.cam0[rows], occupied, q)


def _run_steps(on, to_message, qs=(0.5, 0.9)):
    """Two steps of the two lanes on a fresh context; with ``on`` the numpy restatement runs
    beside the device (on the same context's set calls) and yields the wanted records."""
    W, H = tt.W, tt.H
    fe = fe_mod.Frontend(W, H, nslot=6, max_level=tt.LK["max_level"], max_points=4096)
    out = dict(res=[], tables=[], msgs=[], motion=[], want=[], valid0=None)
    try:
        fe.tracks_create(2, CAP, *GRID)
        grid = tr.Grid(*GRID)
        frames = [tt.lane_frames(seed) for *_, seed in LANES]
        fe.upload_many([3 * l + 1 + j for l in range(2) for j in range(2)],
                       np.stack([frames[l][0][j] for l in range(2) for j in range(2)]))
        tables = {l: tt.lane_table(fe, l, n, kind, seed) for l, (n, kind, _, seed) in enumerate(LANES)}
        for l, t in tables.items():
            fe.tracks_put(l, t.ids, t.life, t.cam0, t.cam1, t.next_id)
        out["valid0"] = [fe.tracks_motion_get(l) for l in range(2)]
        for step in range(2):
            c0 = [3 * l if step == 0 else 3 * l + 1 for l in range(2)]
            fe.upload_many([s for l in range(2) for s in (c0[l], 3 * l + 2)],
                           np.stack([frames[l][step + 1][j] for l in range(2) for j in range(2)]))
            args = [tt.lane_args(l, kind, rs, step, seed) for l, (_, kind, rs, seed) in enumerate(LANES)]
            if on:
                fe.tracks_motion_enable(True, qs[step])
                spy, trace = _Spy(fe), {}
                _, nxt, _ = tr.step(spy, tables, args, grid, W, H, tt.THRESHOLD, inlier_error=tt.INLIER_ERROR,
                                    n_hyp=tt.N_HYP, trace=trace, **tt.LK)
                out["want"].append([_survivor_stat(tables[l], trace, spy.occupied[l], l, qs[step]) for l in range(2)])
                tables = {**tables, **nxt}
            res = fe.tracks_step(args, tt.THRESHOLD, inlier_error=tt.INLIER_ERROR, n_hyp=tt.N_HYP,
                                 to_message=to_message, **tt.LK)
            out["res"].append(res)
            out["tables"].append([fe.tracks_get(l) for l in range(2)])
            out["msgs"].append([fe.tracks_msg_get(l) for l in range(2)])
            out["motion"].append([fe.tracks_motion_get(l) for l in range(2)])
        out["fe"] = fe
        out["args"], out["final_tables"] = args, tables
        return out
    except BaseException:
        fe.close()
        raise


def _same_runs(a, b):
    for ra, rb in zip(a["res"], b["res"]):
        for x, y in zip(ra, rb):
            assert (x.n, x.n_total, x.next_id) == (y.n, y.n_total, y.next_id)
            np.testing.assert_array_equal(x.counters, y.counters)
            assert (x.ids is None) == (y.ids is None)
            if x.ids is not None:
                assert x.ids.tobytes() == y.ids.tobytes() and x.uv.tobytes() == y.uv.tobytes()
    for ta, tb in zip(a["tables"], b["tables"]):
        for x, y in zip(ta, tb):
            assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))
    for ma, mb in zip(a["msgs"], b["msgs"]):
        for x, y in zip(ma, mb):
            assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


@pytest.mark.parametrize("to_message", [False, True])
def test_step_writes_the_record_and_nothing_else(to_message):
    off = _run_steps(False, to_message)
    off["fe"].close()
    on = _run_steps(True, to_message)
    fe = on["fe"]
    try:
        _same_runs(on, off)                                     # tables, messages, counters, ids: bit-equal
        assert all(not v[0] for v in on["valid0"])              # after mfe_tracks_put
        assert all(not v[0] and v[1] == 0 and np.isnan(v[2]) for step in off["motion"] for v in step)
        assert on["res"][0][0].counters[3] > 256                # one lane's survivors pass one 256-row chunk
        for step in range(2):
            for l in range(2):
                valid, n, d2 = on["motion"][step][l]
                wn, wd2 = on["want"][step][l]
                assert valid and n == wn == on["res"][step][l].counters[3] and n > 0
                assert bits(d2) == bits(wd2), (step, l, d2, wd2)
        # a step that fails with -3 leaves the record invalid, and the tables as they were
        with pytest.raises(msckf_amd.MsckfError, match="rc=-3"):
            fe.tracks_step(on["args"], tt.THRESHOLD, max_kp=1, inlier_error=tt.INLIER_ERROR, n_hyp=tt.N_HYP,
                           to_message=to_message, **tt.LK)
        assert [fe.tracks_motion_get(l)[0] for l in range(2)] == [False, False]
        # the record comes back with the next good step of a lane, and only that lane's
        fe.tracks_step(on["args"][:1], tt.THRESHOLD, inlier_error=tt.INLIER_ERROR, n_hyp=tt.N_HYP,
                       to_message=to_message, **tt.LK)
        assert [fe.tracks_motion_get(l)[0] for l in range(2)] == [True, False]
        t = on["final_tables"][0]
        fe.tracks_put(0, t.ids[:5], t.life[:5], t.cam0[:5], t.cam1[:5], t.next_id)
        assert fe.tracks_motion_get(0)[0] is False
        # with the switch off again a step invalidates and writes nothing
        fe.tracks_motion_enable(False, 0.5)
        with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
            fe.tracks_motion_enable(True, 1.5)
    finally:
        fe.close()


def test_motion_enable_needs_tables():
    fe = fe_mod.Frontend(32, 32, nslot=3, max_level=0, max_points=64)
    try:
        with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
            fe.tracks_motion_enable(True, 0.5)
    finally:
        fe.close()


# ------------------------------------------------- the cued update, host source --
CAMS = [0, 1, 3, 3]                       # filter 3's S is made indefinite
MIN_TRACKS, MAX_PX = 5, 1.5
# (n, d2) per status; UNKNOWN both as "no record" and as too few tracks
CUES = {S.STILL: [(5, 2.25), (40, 0.0)], S.MOVING: [(5, np.nextafter(np.float32(2.25), np.float32(3))), (9, 100.0)],
        S.UNKNOWN: [(-1, 0.0), (4, 0.0), (0, np.nan)]}
GATES = {"pass": dict(chi2=1e30, max_speed=1e30), "gamma": dict(chi2=0.0, max_speed=1e30),
         "speed": dict(chi2=1e30, max_speed=0.0)}


def _fill(ctx):
    for b, N in enumerate(CAMS):
        d = problem(N, 4100 + b)
        if b == 3:
            d["P"][6, 6] = -1.0             # S = H P H^T + R loses positive definiteness
        put(ctx, b, d)
    return [State(*ctx.get_state(b)) for b in range(len(CAMS))]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_cued_update_decision_table(dtype):
    """Every cell the state can reach: {pd (filters 0-2), not pd (filter 3)} x the gate's
    three outcomes x the statuses (rotated over the filters from call to call) x the two
    modes x the two policies."""
    ctx = Context(FilterConfig(), n_filters=4, n_cam_capacity=4, dtype=dtype)
    seen = set()
    try:
        w, a = means(11, 4)
        fl = [2, 0, 3, 1]
        call = 0
        for (gname, gate), mode, unknown in itertools.product(GATES.items(), ("veto", "either"), ("imu", "reject")):
            for rot in range(3):
                prm = ZuptConfig(**gate)
                cue = VisionCue(max_px=MAX_PX, min_tracks=MIN_TRACKS, mode=mode, unknown=unknown)
                before = _fill(ctx)
                status = [(k + rot) % 3 for k in range(4)]
                pick = [CUES[s][(call + k) % len(CUES[s])] for k, s in enumerate(status)]
                cn = np.array([p[0] for p in pick], np.int32)
                cd = np.array([p[1] for p in pick], np.float32)
                ctx.zupt_batch_cued(fl, w, a, prm, cue, cue_n=cn, cue_d2=cd)
                app, gam, cnt, r_cue, r_n, r_d2 = ctx.zupt_cue_results(fl)
                for k, b in enumerate(fl):
                    st = oracle_of(before[b])
                    want_app, want_gam, want_status = S.zupt_update_cued(st, w[k], a[k], prm, cue, cn[k], cd[k])
                    what = "%s %s %s rot %d filter %d " % (gname, mode, unknown, rot, b)
                    assert want_status == status[k] == r_cue[k], what
                    assert bool(app[k]) == want_app, what
                    assert (b == 3) == np.isnan(want_gam) == np.isnan(gam[k]), what
                    if b != 3:
                        np.testing.assert_allclose(gam[k], want_gam, rtol=1e-9, err_msg=what)
                    if cn[k] < 0:
                        assert r_n[k] == -1 and np.isnan(r_d2[k]), what
                    else:
                        assert r_n[k] == cn[k] and bits(r_d2[k]) == bits(cd[k]), what
                    after = State(*ctx.get_state(b))
                    if want_app:
                        check_against(after, st, dtype, what)
                        np.testing.assert_array_equal(after.P, after.P.T)
                    else:
                        assert same_state(before[b], after), what
                    seen.add((b != 3, gname, status[k], mode, unknown, want_app))
                call += 1
        # each cell of the table occurred, with a positive definite S and without
        cells = {c[:5] for c in seen}
        assert len(cells) == 2 * 3 * 3 * 2 * 2
        assert any(c[5] for c in seen if c[1] == "speed" and c[3] == "either")       # vision overrides the speed gate
        assert not any(c[5] for c in seen if not c[0])                               # never without a factor of S
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_veto_with_still_cues_is_the_plain_update_bit_for_bit(dtype):
    prm = ZuptConfig(vel_noise=1e-2, max_speed=2.0)
    cue = VisionCue(max_px=MAX_PX, min_tracks=MIN_TRACKS, mode="veto")
    outs = []
    for cued in (False, True):
        ctx = Context(FilterConfig(), n_filters=4, n_cam_capacity=4, dtype=dtype)
        try:
            for b, N in enumerate(CAMS):
                d = problem(N, 4200 + b, v_scale=0.01)
                if b == 1:
                    d["imu_v"] = np.array([3.0, 0.0, 0.0])     # refused by max_speed
                put(ctx, b, d)
            before = [State(*ctx.get_state(b)) for b in range(4)]
            fl = [3, 1, 0, 2]
            w = np.array([_lib.unpack_imu(before[b].imu)["bg"] for b in fl])
            a = np.array([_lib.unpack_imu(before[b].imu)["ba"] - Z.O.to_rotation(_lib.unpack_imu(before[b].imu)["q"])
                          @ _lib.unpack_imu(before[b].imu)["gravity"] for b in fl])
            if cued:
                ctx.zupt_batch_cued(fl, w, a, prm, cue, cue_n=[9, 9, 9, 9], cue_d2=[0.0, 1.0, 2.25, 0.5])
                app, gam, cnt = ctx.zupt_cue_results(fl)[:3]
            else:
                ctx.zupt_batch(fl, w, a, prm)
                app, gam, cnt = ctx.zupt_results(fl)
                assert (ctx.zupt_cue_results(fl)[3] == -1).all()            # the plain call leaves the cue records
            outs.append(([ctx.get_state(b) for b in range(4)], app, gam, cnt))
        finally:
            ctx.close()
    (sa, aa, ga, ca), (sb, ab, gb, cb) = outs
    assert aa.tolist() == ab.tolist() and aa.any() and not aa.all()
    assert ga.tobytes() == gb.tobytes() and ca.tolist() == cb.tolist()
    for x, y in zip(sa, sb):
        assert same_state(x, y)


def test_cued_records_and_argument_errors():
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=4)
    try:
        app, gam, cnt, cue, cn, cd = ctx.zupt_cue_results([0, 1, 2])        # before anything was enqueued
        assert not app.any() and np.isnan(gam).all() and (cnt == 0).all()
        assert (cue == -1).all() and (cn == -1).all() and np.isnan(cd).all()
        put(ctx, 0, problem(2, 1))
        before = State(*ctx.get_state(0))
        w, a = means(0, 2)
        ok_p = dict(vel_noise=1e-4, gyro_noise=4e-6, acc_noise=4e-4, chi2=1e30, max_speed=1e30, rows=7)
        ok_c = dict(max_px=1.0, min_tracks=1, mode=0, unknown=0)
        P, Q = lambda **kw: MsckfZuptParamsT(*{**ok_p, **kw}.values()), lambda **kw: MsckfZuptCueT(*{**ok_c, **kw}.values())
        n1, d1 = np.array([3], np.int32), np.array([0.0], np.float32)
        bad = [(P(rows=0), Q()), (P(vel_noise=0.0), Q()), (P(max_speed=-1.0), Q()), (P(chi2=float("nan")), Q()),
               (P(), Q(max_px=-1.0)), (P(), Q(max_px=float("nan"))), (P(), Q(min_tracks=0)), (P(), Q(mode=2)),
               (P(), Q(mode=-1)), (P(), Q(unknown=2))]
        for p, q in bad:
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch_cued([0], w[:1], a[:1], p, q, cue_n=n1, cue_d2=d1)
        for kw in (dict(cue_n=None, cue_d2=d1), dict(cue_n=n1, cue_d2=None)):      # fe == NULL with a null cue array
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch_cued([0], w[:1], a[:1], P(), Q(), **kw)
        for fl in ([0, 0], [3], [-1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch_cued(fl, w[:len(fl)], a[:len(fl)], P(), Q(), cue_n=[1] * len(fl), cue_d2=[0.0] * len(fl))
        ptr = lambda x, t: x.ctypes.data_as(C.POINTER(t))
        fl = np.array([0], np.int32)
        assert ctx.lib.msckf_zupt_batch_cued(ctx.h, None, 1, ptr(fl, C.c_int32), None, ptr(n1, C.c_int32),
                                             ptr(d1, C.c_float), ptr(w, C.c_double), ptr(a, C.c_double),
                                             C.byref(P()), None) == -1              # a null cue
        app, gam, cnt, cue, cn, cd = ctx.zupt_cue_results([0, 1, 2])
        assert not app.any() and (cnt == 0).all() and (cue == -1).all() and (cn == -1).all() and np.isnan(cd).all()
        assert same_state(before, State(*ctx.get_state(0)))
        # and a good call writes the listed slot's records only
        ctx.zupt_batch_cued([0], w[:1], a[:1], P(), Q(mode=1), cue_n=n1, cue_d2=d1)
        app, gam, cnt, cue, cn, cd = ctx.zupt_cue_results([0, 1])
        assert app.tolist() == [True, False] and cnt.tolist() == [1, 0]
        assert cue.tolist() == [S.STILL, -1] and cn.tolist() == [3, -1] and cd[0] == 0.0 and np.isnan(cd[1])
    finally:
        ctx.close()


# ------------------------------------------------------------ device source --
def test_cued_update_reads_the_front_end_record_on_the_device():
    on = _run_steps(True, True, qs=(0.5, 0.5))
    fe = on["fe"]
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=4)
    bare = fe_mod.Frontend(32, 32, nslot=3, max_level=0, max_points=64)
    try:
        for b in range(2):
            put(ctx, b, problem(2, 4300 + b))
        w, a = means(3, 2)
        prm = ZuptConfig(chi2=1e30, max_speed=1e30)
        cue = VisionCue(max_px=0.01, min_tracks=1, mode="veto", unknown="reject")
        rec = [fe.tracks_motion_get(l) for l in range(2)]
        assert all(r[0] for r in rec)
        ctx.zupt_batch_cued([1, 0], w, a, prm, cue, fe=fe, lanes=[0, 1])
        app, _, _, r_cue, r_n, r_d2 = ctx.zupt_cue_results([1, 0])            # synchronises before the next put
        for k, l in enumerate([0, 1]):
            assert r_n[k] == rec[l][1] and bits(r_d2[k]) == bits(rec[l][2])
            assert r_cue[k] == S.cue_status(rec[l][1], rec[l][2], cue) == S.MOVING     # the scene moves by 2.5 px
        assert not app.any()
        t = on["final_tables"][0]
        fe.tracks_put(0, t.ids[:5], t.life[:5], t.cam0[:5], t.cam1[:5], t.next_id)     # lane 0's record is gone
        before = State(*ctx.get_state(1))
        ctx.zupt_batch_cued([1, 0], w, a, prm, cue, fe=fe, lanes=[0, 1])
        app, _, _, r_cue, r_n, r_d2 = ctx.zupt_cue_results([1, 0])
        assert r_cue.tolist() == [S.UNKNOWN, S.MOVING] and r_n[0] == -1 and np.isnan(r_d2[0]) and r_n[1] == rec[1][1]
        assert not app.any() and same_state(before, State(*ctx.get_state(1)))          # unknown = reject
        for lanes in ([0, 2], [-1, 0], [1, 1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch_cued([1, 0], w, a, prm, cue, fe=fe, lanes=lanes)
        with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):                       # no track tables
            ctx.zupt_batch_cued([1, 0], w, a, prm, cue, fe=bare, lanes=[0, 1])
    finally:
        bare.close()
        ctx.close()
        fe.close()


# --------------------------------------------------------------- end to end --
N_REST_FRAMES, N_MOVE_FRAMES = 6, 4
_e2e = {}


def _stream():
    """200 IMU samples at rest up to the first frame's stamp (gravity initialisation), then
    N_REST_FRAMES identical stereo pairs and N_MOVE_FRAMES of the scene moving by its step;
    every frame's last IMU sample carries the frame's stamp, so the filter's first frame
    propagates one sample and enqueues its update."""
    g = golden("frontend_ref")
    W, H = (int(v) for v in g["size"])
    name = "rectified"
    f = fs.texture_fn(int(g[name + "_seed"]), W=W, H=H)
    still = np.array([0.0, 0.0, 9.81])
    lead = [ImuMsg(-0.005 * j, np.zeros(3), still) for j in range(200, 0, -1)]
    frames = []
    for k in range(N_REST_FRAMES + N_MOVE_FRAMES):
        t = 0.05 * k
        imu = [ImuMsg(t - 0.005 * j, np.zeros(3), still) for j in range(9 if k else 0, -1, -1)]
        dx, dy = np.array(g[name + "_step"], float) * max(0, k - N_REST_FRAMES + 1)
        disp = float(g[name + "_disparity"])
        frames.append((imu, StereoMsg(t, ImgMsg(t, fs.render(f, W, H, dx, dy)), ImgMsg(t, fs.render(f, W, H, dx - disp, dy)))))
    return scene_config(g, name), lead, frames


def _run_vio(handoff, zupt):
    key = (handoff, zupt.vision is not None)
    if key in _e2e:
        return _e2e[key]
    cfg, lead, frames = _stream()
    with StereoVIO(FilterConfig(), cfg, handoff=handoff, zupt=zupt) as vio:
        for m in lead:
            vio.imu_callback(m)
        res = []
        for imu, msg in frames:
            for m in imu:
                vio.imu_callback(m)
            res.append(vio.stereo_callback(msg))
        motion = vio.multi.frontend.track_motion(0) if zupt.vision is not None else None
        _e2e[key] = dict(res=res, log=list(vio.zupt_log), launches=vio.launches, motion=motion,
                         on=vio.multi.frontend.track_motion_on)
    return _e2e[key]


def _pose_bytes(r):
    return (np.asarray(r.pose._vio_R__).tobytes(), np.asarray(r.pose._vio_t__).tobytes(), np.asarray(r.velocity).tobytes())


@pytest.mark.parametrize("handoff", ["device", "host"])
def test_stereo_vio_with_the_vision_cue(handoff):
    cue = VisionCue(mode="either")                              # the defaults: half a pixel, 20 tracks
    got = _run_vio(handoff, ZuptConfig(vision=cue))
    n = N_REST_FRAMES + N_MOVE_FRAMES
    assert all(r is not None for r in got["res"]) and len(got["log"]) == n
    status = [e[3] for e in got["log"]]
    assert status[0] == S.UNKNOWN and got["log"][0][4] == -1 and np.isnan(got["log"][0][5])     # the lane's first frame
    assert status[1:N_REST_FRAMES] == [S.STILL] * (N_REST_FRAMES - 1)
    assert status[N_REST_FRAMES:] == [S.MOVING] * N_MOVE_FRAMES
    assert all(e[4] >= cue.min_tracks for e in got["log"][1:])
    assert all(e[1] for e in got["log"][1:N_REST_FRAMES])       # EITHER: a still image applies the update
    last = got["log"][-1]
    assert got["motion"][0] and got["motion"][1] == last[4] and bits(got["motion"][2]) == bits(np.float32(last[5]))
    other = _run_vio("host" if handoff == "device" else "device", ZuptConfig(vision=cue))
    assert len(other["log"]) == n
    for x, y in zip(got["log"], other["log"]):                  # the same log, NaN included
        assert x[:2] == y[:2] and x[3:5] == y[3:5]
        assert np.float64(x[2]).tobytes() == np.float64(y[2]).tobytes()
        assert bits(np.float32(x[5])) == bits(np.float32(y[5]))
    for x, y in zip(got["res"], other["res"]):
        assert _pose_bytes(x) == _pose_bytes(y)


def test_stereo_vio_without_the_cue_runs_the_plain_update():
    plain = _run_vio("device", ZuptConfig())
    cued = _run_vio("device", ZuptConfig(vision=VisionCue(mode="either")))
    assert not plain["on"] and cued["on"]
    assert all(len(e) == 3 for e in plain["log"]) and len(plain["log"]) == N_REST_FRAMES + N_MOVE_FRAMES
    # no call is added on either side: the device hand-off's cue costs no request of its own
    assert plain["launches"] == cued["launches"]
    assert "tracks_motion_get" not in plain["launches"]["frontend"]
    host = _run_vio("host", ZuptConfig(vision=VisionCue(mode="either")))
    assert host["launches"]["frontend"]["tracks_motion_get"] == N_REST_FRAMES + N_MOVE_FRAMES - 1
    # the poses and the log are those of the two classes wired by hand, on a front-end config built
    # without the new fields and through the plain msckf_zupt_batch
    cfg, lead, frames = _stream()
    on = fe_mod.FrontendConfig(**{**{k: v for k, v in vars(cfg).items() if not k.startswith("track_motion")},
                                  "device_pipeline": True, "device_tracks": True})
    mp = fe_mod.MultiImageProcessor(1, lane_configs=[on])
    ms = MultiMSCKF(1, config=FilterConfig(), device_map=True, device_keyframes=True, zupt=ZuptConfig())
    try:
        for m in lead:
            mp.imu_callback(0, m)
            ms.imu_callback(0, m)
        res = []
        for imu, msg in frames:
            for m in imu:
                mp.imu_callback(0, m)
                ms.imu_callback(0, m)
            res.append(ms.feature_callbacks(mp.stereo_callbacks({0: msg}, arrays=True))[0])
        assert not mp.track_motion_on and "tracks_motion_get" not in mp.launches
        assert len(res) == len(plain["res"]) and all(r is not None for r in res)
        for x, y in zip(plain["res"], res):
            assert _pose_bytes(x) == _pose_bytes(y)
        assert len(ms.lanes[0].zupt_log) == len(plain["log"])
        for x, y in zip(plain["log"], ms.lanes[0].zupt_log):
            assert x[:2] == y[:2] and np.float64(x[2]).tobytes() == np.float64(y[2]).tobytes()
        wired_f = dict(ms.launches)
        assert wired_f.pop("map_add_lost") == plain["launches"]["filter"]["map_add_lost_tracks"]
        assert wired_f == {k: v for k, v in plain["launches"]["filter"].items() if k != "map_add_lost_tracks"}
    finally:
        mp.close()
        ms.close()
