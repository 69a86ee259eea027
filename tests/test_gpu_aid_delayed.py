"""The delayed aiding fixes (include/msckf_aid_delayed.h) on the GPU against
their numpy restatement tests/aid_delayed_ref.py, and through the host classes.

The setup and the tolerances are test_gpu_aid.py's: states and covariances from
synth.make_update_problem(N, 4, seed), the reference on the state READ BACK from
the device; fp64 P <= 1e-9 relative and the state to atol 1e-11, gamma to rtol
1e-9 in both dtypes, fp32 P <= 1e-4 relative and the state to atol 1e-6.  Before
a decision is compared, the reference's gamma is asserted to lie off the gate by
1e-6 relative.

N = 7 | 8, 12 | 13, 17 | 18 and 39 | 40 put D = 21 + 6 N on both sides of 64, 96,
128 and 256 (the tiles of k_aid_delayed_apply and the gain's rows per pass); N =
1 and 2 are the smallest windows a fix can use, N = 128 the largest.
"""
import numpy as np
import pytest

from lifecycle import State, oracle_of
import msckf_amd
from msckf_amd import CHI2_95, AidingConfig, AidingFix, FilterConfig, chi2_threshold, synth
from msckf_amd._lib import Context, aid_delayed_fix
from msckf_amd.replay import FeatureStream, replay
from msckf_amd.scheduler import MultiMSCKF, StereoVIO
import aid_ref as A
import aid_delayed_ref as Dl
from test_aid_delayed_ref import AXIS, MASKS, fix_for, params
from test_gpu_aid import FIRST_BLIND, STREAM, T0, short, to_fix
from test_gpu_zupt import check_against, problem, put, same_state

pytestmark = pytest.mark.gpu


def reference(state, prm, fix):
    """(oracle state after the update, applied, gamma, status), the gate's margin asserted."""
    st = oracle_of(state)
    if Dl.in_window(st, fix[2], fix[3]):
        pd, gam = Dl.gamma_of(st, prm, fix)
        gate = Dl.gate_of(prm, fix[4])
        if pd:
            assert abs(gam - gate) > 1e-6 * abs(gate), (gam, gate)
    app, gam, status = Dl.update(st, prm, fix)
    return st, app, gam, status


def run_one(ctx, b, prm, fix):
    ctx.aid_delayed_batch([b], [aid_delayed_fix(*fix)], prm)
    app, gam, rows, sta, cnt = ctx.aid_delayed_results([b])
    return bool(app[0]), gam[0], int(rows[0]), int(sta[0]), int(cnt[0])


def with_clone_rotation(d, slot, angle):
    """The problem with clone slot + 1 rotated by ``angle`` about AXIS from clone
    slot (None: the same quaternion, bit for bit)."""
    from oracle import msckf_oracle as O
    q = np.array(d["cam_q"], float)
    q[slot + 1] = q[slot] if angle is None else O.to_quaternion(Dl.so3_exp(angle * AXIS) @ O.to_rotation(q[slot]))
    d["cam_q"] = q
    return d


def check_one(ctx, b, prm, fix, dtype, what=""):
    before = State(*ctx.get_state(b))
    st, app, gam, status = reference(before, prm, fix)
    assert app and status == Dl.APPLIED, what
    got_app, got_gam, rows, sta, cnt = run_one(ctx, b, prm, fix)
    after = State(*ctx.get_state(b))
    assert got_app and sta == Dl.APPLIED and rows == fix[4], what
    np.testing.assert_allclose(got_gam, gam, rtol=1e-9, err_msg=what)
    check_against(after, st, dtype, what)
    np.testing.assert_array_equal(after.P, after.P.T)
    return cnt


# ------------------------------------------------------------------ ABI --

def test_argument_errors_enqueue_nothing():
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(3, 1))
        before = State(*ctx.get_state(0))
        prm = params()
        z, var, _, _, _ = fix_for(oracle_of(before), prm, 0x3f, 0, 0.5, 0)
        nan = float("nan")

        def fx(rows=0x3f, slot=0, lam=0.5, **kw):
            zz, vv = z.copy(), var.copy()
            for k, v in kw.items():
                (zz if k[0] == "z" else vv)[int(k[1:])] = v
            return aid_delayed_fix(zz, vv, slot, lam, rows)

        def raw(prm, **kw):
            p = prm.params()
            for k, v in kw.items():
                getattr(p, k)[:] = v
            return p

        bad = [(fx(rows=0), prm), (fx(rows=0x40), prm), (fx(rows=-1), prm), (fx(v0=0.0), prm), (fx(v5=-1.0), prm),
               (fx(v4=nan), prm), (fx(z2=nan), prm), (fx(lam=-1e-3), prm), (fx(lam=1.0), prm), (fx(lam=nan), prm),
               (fx(slot=-1), prm), (fx(slot=4), prm),
               (fx(rows=Dl.DIR), raw(prm, dir_w=[1.0, 2e-3, 0.0])),
               (fx(rows=Dl.POS), raw(prm, chi2=[1.0, 1.0, nan] + [1.0] * 9))]
        for f, p in bad:
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.aid_delayed_batch([0], [f], p)
        for fl in ([0, 0], [3], [-1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.aid_delayed_batch(fl, [fx()] * len(fl), prm)
        ctx.aid_delayed_batch([], [], prm)   # a no-op
        app, gam, rows, sta, cnt = ctx.aid_delayed_results([0, 1, 2])   # the records' initial values
        assert not app.any() and np.isnan(gam).all() and (rows == 0).all() and (cnt == 0).all()
        assert (sta == Dl.NONE).all()
        assert same_state(before, State(*ctx.get_state(0)))
        # legal: what the masked rows and the unused parameters hold does not matter
        ok = fx(rows=Dl.POS, z5=nan, v5=-1.0)
        ctx.aid_delayed_batch([0], [ok], raw(prm, R_body=[nan] * 9, dir_w=[0, 0, 0], chi2=[nan, nan, 1e30] + [nan] * 9))
        app, _, _, sta, _ = ctx.aid_delayed_results([0, 1])
        assert app.tolist() == [True, False] and sta.tolist() == [Dl.APPLIED, Dl.NONE]
    finally:
        ctx.close()


# --------------------------------------------------------------- parity --

def pairs_of(N):
    """(slot, lambda): the clone pair first, in the middle and last."""
    if N == 1:
        return [(0, 0.0)]
    return sorted(set([(0, 0.5), ((N - 2) // 2, 0.37), (N - 2, 0.5)]))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", [1, 2, 7, 8, 12, 13, 17, 18, 39, 40, 128])
def test_window_sizes(N, dtype):
    prm = params()
    pairs = pairs_of(N)
    ctx = Context(FilterConfig(), n_filters=len(pairs), n_cam_capacity=N, dtype=dtype)
    try:
        for b, (slot, lam) in enumerate(pairs):
            put(ctx, b, problem(N, 500 + N))
            fix = fix_for(oracle_of(State(*ctx.get_state(b))), prm, 0x3f, slot, lam, N + b)
            assert check_one(ctx, b, prm, fix, dtype, "N %d slot %d " % (N, slot)) == 1
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_window_below_capacity(dtype):
    """The stride of P and of the cam records is the capacity's (128), not the window's (5)."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=128, dtype=dtype)
    try:
        for b in range(2):
            put(ctx, b, problem(5, 728 + b))
        before = [State(*ctx.get_state(b)) for b in range(2)]
        fixes = {0: fix_for(oracle_of(before[0]), prm, 0x3f, 3, 0.25, 1), 1: fix_for(oracle_of(before[1]), prm, 0x3f, 4, 0.0, 2)}
        ctx.aid_delayed_batch([1, 0], [aid_delayed_fix(*fixes[1]), aid_delayed_fix(*fixes[0])], prm)
        got_app, got_gam, _, sta, _ = ctx.aid_delayed_results([1, 0])
        for k, b in enumerate([1, 0]):
            st, app, gam, _ = reference(before[b], prm, fixes[b])
            assert app and got_app[k] and sta[k] == Dl.APPLIED
            np.testing.assert_allclose(got_gam[k], gam, rtol=1e-9)
            after = State(*ctx.get_state(b))
            check_against(after, st, dtype, "filter %d " % b)
            np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("angle,lam,last", [(None, 0.37, False), (1e-9, 0.37, False), (0.3, 0.37, False),
                                            (0.3, 0.0, True), (0.3, 0.999, False), (None, 0.999, False)])
def test_interpolation_corners(angle, lam, last, dtype):
    """Identical clone rotations (the phi = 0 series branch), phi = 1e-9 and 0.3
    rad, lambda = 0 on the last clone (slot = n - 1) and lambda = 0.999."""
    prm = params()
    N = 6
    slot = N - 1 if last else 2
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=N, dtype=dtype)
    try:
        d = problem(N, 640)
        put(ctx, 0, d if last else with_clone_rotation(d, slot, angle))
        before = State(*ctx.get_state(0))
        if angle is None:
            assert before.cams[slot, 0:4].tobytes() == before.cams[slot + 1, 0:4].tobytes()
        fix = fix_for(oracle_of(before), prm, 0x3f, slot, lam, 3)
        check_one(ctx, 0, prm, fix, dtype)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rows", MASKS)
def test_row_masks(rows, dtype):
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=6, dtype=dtype)
    try:
        put(ctx, 0, problem(6, 700 + rows))
        before = State(*ctx.get_state(0))
        z, var, slot, lam, _ = fix_for(oracle_of(before), prm, rows, 3, 0.6, rows)
        for g in range(6):   # the masked rows' entries are ignored
            if not (rows >> g) & 1:
                z[g], var[g] = np.nan, -1.0
        check_one(ctx, 0, prm, (z, var, slot, lam, rows), dtype)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mixed_batch(dtype):
    """Seven slots with 3 .. 9 cams, filters = [4, 1, 5, 2, 6] under the CHI2_95
    gate: slot 4 POS | DIR on clones (2, 3), slot 1 POS 0.5 m off and rejected by
    gamma, slot 5 POS z alone with lambda = 0, slot 2 with slot = n (BAD_SLOT),
    slot 6 with slot = n - 1 and lambda > 0 (BAD_SLOT).  Rejected, BAD_SLOT and
    unlisted slots keep every byte; slot 5 is updated again by a second call."""
    prm = params(chi2=None)
    ctx = Context(FilterConfig(), n_filters=7, n_cam_capacity=10, dtype=dtype)
    try:
        for b in range(7):
            put(ctx, b, problem(3 + b, 800 + b))
        before = [State(*ctx.get_state(b)) for b in range(7)]
        n = [3 + b for b in range(7)]
        fl = [4, 1, 5, 2, 6]
        spec = [(Dl.POS | Dl.DIR, 2, 0.3), (Dl.POS, 1, 0.7), (0x04, 4, 0.0), (Dl.POS, n[2], 0.0), (Dl.DIR, n[6] - 1, 0.5)]
        fixes = []
        for b, (rows, slot, lam) in zip(fl, spec):
            ok = Dl.in_window(oracle_of(before[b]), slot, lam)
            z, var, _, _, _ = fix_for(oracle_of(before[b]), prm, rows, slot if ok else 0, lam if ok else 0.0, 40 + b, off=0.02)
            if b == 1:
                z[0:3] += 0.5
            fixes.append((z, var, slot, lam, rows))
        refs = [reference(before[b], prm, f) for b, f in zip(fl, fixes)]
        assert [r[1] for r in refs] == [True, False, True, False, False]
        assert [r[3] for r in refs] == [Dl.APPLIED, Dl.GATED, Dl.APPLIED, Dl.BAD_SLOT, Dl.BAD_SLOT]
        ctx.aid_delayed_batch(fl, [aid_delayed_fix(*f) for f in fixes], prm)
        app, gam, rows, sta, cnt = ctx.aid_delayed_results(fl)
        assert app.tolist() == [True, False, True, False, False] and cnt.tolist() == [1, 0, 1, 0, 0]
        assert rows.tolist() == [s[0] for s in spec] and sta.tolist() == [r[3] for r in refs]
        np.testing.assert_allclose(gam[:3], [r[2] for r in refs[:3]], rtol=1e-9)
        assert np.isnan(gam[3:]).all()
        mid = [State(*ctx.get_state(b)) for b in range(7)]
        for b in (0, 1, 2, 3, 6):   # unlisted, rejected by gamma, BAD_SLOT
            assert same_state(before[b], mid[b]), b
        for k in (0, 2):
            check_against(mid[fl[k]], refs[k][0], dtype, "slot %d " % fl[k])
            np.testing.assert_array_equal(mid[fl[k]].P, mid[fl[k]].P.T)
        # slot 5 again, DIR on its first pair
        fix = fix_for(oracle_of(mid[5]), prm, Dl.DIR, 0, 0.9, 50, off=0.02)
        st5, app5, gam5, _ = reference(mid[5], prm, fix)
        assert app5
        ctx.aid_delayed_batch([5], [aid_delayed_fix(*fix)], prm)
        app, gam, rows, sta, cnt = ctx.aid_delayed_results([5, 4, 1, 0])
        assert app.tolist() == [True, True, False, False] and cnt.tolist() == [2, 1, 0, 0]
        assert rows.tolist() == [Dl.DIR, Dl.POS | Dl.DIR, Dl.POS, 0] and sta[3] == Dl.NONE
        np.testing.assert_allclose(gam[0], gam5, rtol=1e-9)
        check_against(State(*ctx.get_state(5)), st5, dtype, "slot 5 again ")
        for b in (0, 1, 2, 3, 4, 6):
            assert same_state(mid[b], State(*ctx.get_state(b))), b
    finally:
        ctx.close()


# ----------------------------------------------------------- properties --

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_repeat_gives_the_same_bits(dtype):
    prm = params()
    outs = []
    for _ in range(2):
        ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=13, dtype=dtype)
        try:
            for b in range(2):
                put(ctx, b, problem(12 + b, 900 + b))
            fixes = [fix_for(oracle_of(State(*ctx.get_state(b))), prm, (0x3f, 0x1d)[b], (3, 11)[b], (0.4, 0.8)[b], 9 + b)
                     for b in range(2)]
            ctx.aid_delayed_batch([0, 1], [aid_delayed_fix(*f) for f in fixes], prm)
            outs.append([ctx.get_state(b) for b in range(2)] + [ctx.aid_delayed_results([0, 1])])
        finally:
            ctx.close()
    for x, y in zip(outs[0], outs[1]):
        assert same_state(x, y)
    assert outs[0][2][0].all()
    for b in range(2):
        np.testing.assert_array_equal(outs[0][b][2], outs[0][b][2].T)


@pytest.mark.parametrize("chi2", [0.0, -1.0])
def test_non_positive_chi2_never_applies(chi2):
    prm = params(chi2=chi2)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 960))
        before = State(*ctx.get_state(0))
        app, gam, rows, sta, cnt = run_one(ctx, 0, prm, fix_for(oracle_of(before), prm, 0x3f, 1, 0.5, 6))
        assert not app and np.isfinite(gam) and gam > 0 and cnt == 0 and rows == 0x3f and sta == Dl.GATED
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_indefinite_innovation_covariance():
    """P[21 + 6 s + 3, 21 + 6 s + 3] strongly negative through set_state: S is not
    positive definite, gamma is NaN, nothing is applied or written, and that is
    no error."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 970)
        P = d["P"].copy()
        s = 1
        P[21 + 6 * s + 3, 21 + 6 * s + 3] = -10.0
        put(ctx, 0, d, P=P)
        before = State(*ctx.get_state(0))
        fix = fix_for(oracle_of(before), prm, 0x3f, s, 0.5, 7)
        _, app, gam, status = reference(before, prm, fix)
        assert not app and np.isnan(gam) and status == Dl.NOT_PD
        got_app, got_gam, rows, sta, cnt = run_one(ctx, 0, prm, fix)
        assert not got_app and np.isnan(got_gam) and cnt == 0 and rows == 0x3f and sta == Dl.NOT_PD
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_kernels_have_stage_timers():
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 980))
        ctx.set_profiling(True)
        run_one(ctx, 0, prm, fix_for(oracle_of(State(*ctx.get_state(0))), prm, 0x3f, 2, 0.5, 8))
        times = ctx.kernel_times()
        assert times["aid_delayed_gain"][1] == 1 and times["aid_delayed_apply"][1] == 1
        assert "aid_gain" not in times or times["aid_gain"][1] == 0
    finally:
        ctx.close()


# --------------------------------------------------------- host classes --

LATENCY = 0.2


def delayed_config(**kw):
    return AidingConfig(**{**dict(lever=A.LEVER, dir_w=tuple(A.DIR_W), max_age=A.MAX_AGE, delayed=True), **kw})


class Recording(msckf_amd.MSCKF):
    """MSCKF that notes the kinds of the requests it serves."""

    def _serve(self, req):
        self.__dict__.setdefault("kinds", []).append((self._n_published, req[0]))
        return super()._serve(req)


def test_msckf_with_late_fixes_follows_the_oracle():
    """MSCKF(aiding=AidingConfig(delayed=True)) in fp64 on test_gpu_aid's short
    outage stream, POS fixes by the recipe handed over 0.2 s after their stamp
    and, from the 8th on, a second POS fix per message at zero latency (so frames
    carry a delayed and a current fix), against OracleAidDelayed frame by frame:
    the same routing and decisions (the feature gates' and the stacked shapes
    too), the pose within 1e-6 relative, and the delayed request served before
    the frame's "aid" request."""
    oseq, plain, Al, seq = short()
    late = Dl.late_messages(plain[:, 0], T0, Al, A.POS, LATENCY)
    late += [(m[0], m) for _, m in Dl.late_messages(plain[:, 0], T0, Al, A.POS, 0.0, seed=300)[8:]]
    late.sort(key=lambda e: e[0])
    orc = Dl.OracleAidDelayed(FilterConfig(), chi2_threshold, delayed_config())
    ref = Dl.run_outage_late(orc, seq, FIRST_BLIND, late)
    assert len(orc.aid_delayed_log) >= 10 and len(orc.aid_log) == 8
    both = set(e[0] for e in orc.aid_delayed_log) & set(e[0] for e in orc.aid_log)
    assert both
    gate = CHI2_95[2]
    assert all(abs(e[3] - gate) > 1e-3 * gate for e in orc.aid_log + orc.aid_delayed_log)
    flt = Recording(aiding=delayed_config())
    try:
        k, recs = 0, []
        for kind, m in oseq.events():
            tm = m.vio_timestamp__ if kind == 0 else m.timestamp
            while k < len(late) and late[k][0] <= tm:
                flt.aiding_callback(to_fix(late[k][1]))
                k += 1
            if kind == 0:
                flt.imu_callback(m)
                continue
            if flt.feature_callback(m) is not None:
                s = flt.imu_state()
                recs.append(np.concatenate([[m.timestamp], s["p"], s["v"], s["q"]]))
        rec = np.array(recs)
        assert rec.shape == ref.shape
        assert [(f, r, a) for f, r, a, _ in flt.aid_log] == [(f, r, a) for f, r, a, _ in orc.aid_log]
        assert [(e[0], e[1], e[2], e[4], e[6]) for e in flt.aid_delayed_log] == \
            [(e[0], e[1], e[2], e[4], e[6]) for e in orc.aid_delayed_log]
        np.testing.assert_allclose([e[5] for e in flt.aid_delayed_log], [e[5] for e in orc.aid_delayed_log], atol=1e-12)
        assert flt.aid_delayed_count == sum(e[2] for e in orc.aid_delayed_log)
        assert [(f, t) for f, t, _ in flt.aid_dropped_log] == [(f, t) for f, t, _ in orc.aid_dropped]
        # gamma is quadratic in r; r is ~ 2 sigma = 0.04 and the two states are held to 1e-6: 2 x 1e-6 / 0.04
        np.testing.assert_allclose([e[3] for e in flt.aid_delayed_log], [e[3] for e in orc.aid_delayed_log], rtol=1e-3)
        np.testing.assert_allclose([e[3] for e in flt.aid_log], [e[3] for e in orc.aid_log], rtol=1e-3)
        assert np.array(flt.gate_log).tolist() == np.array(orc.gate_log).tolist()
        assert np.array(flt.shape_log).tolist() == np.array(orc.shape_log).tolist()
        pose = [1, 2, 3, 7, 8, 9, 10]   # p, q
        for k in range(len(ref)):
            assert np.linalg.norm(rec[k, pose] - ref[k, pose]) <= 1e-6 * np.linalg.norm(ref[k, pose]), k
        for f in both:   # the stated order within a frame
            kinds = [kd for fr, kd in flt.kinds if fr == f and kd in ("aid_delayed", "aid", "augment")]
            assert kinds == ["aid_delayed", "aid", "augment"], (f, kinds)
    finally:
        flt.close()


def lane_config():
    """max_age below the recipe's 12 ms lead: every fix is stale at the frame
    that follows it, waits there (it is newer than the newest clone) and takes
    the delayed path one frame on, 62 ms old -- late fixes from messages that
    run_streams can be given up front."""
    return delayed_config(max_age=0.005)


def lane_messages():
    """Late fixes per lane: POS before every 4th published frame, none, POS +
    DIR before every 2nd -- and on lane 2 a second message 5 ms after every
    4th, so some frame steps have two late fixes on a lane."""
    _, plain, Al, _ = short()
    ft = plain[:24, 0]
    lane2 = A.fix_messages(ft, T0, Al, A.POS | A.DIR, seed=101, every=2)
    lane2 += A.fix_messages(ft, T0, Al, A.POS, seed=102, every=4, lead=0.007)
    return [A.fix_messages(ft, T0, Al, A.POS), [], sorted(lane2, key=lambda m: m[0])]


def cut_stream(n):
    oseq = short()[0]
    return FeatureStream.from_synthetic(synth.Sequence(
        [m for m in oseq.imu if m.vio_timestamp__ <= oseq.frames[n - 1].timestamp], oseq.frames[:n], oseq.gt_t[:n],
        oseq.gt_p[:n], oseq.gt_R[:n]))


@pytest.mark.parametrize("on_device", [False, True])
def test_scheduler_with_late_fixes_equals_single_filters(on_device):
    """Three lanes on the first 44 frames of the stream, late fixes on lanes 0
    and 2 at different rates: every lane equals its single filter bit for bit,
    and "aid_delayed" is launched once per frame step and request index that
    any lane has."""
    kw = dict(device_map=True, device_keyframes=True) if on_device else {}
    st = cut_stream(44)
    lanes = lane_messages()
    singles = []
    for msgs in lanes:
        flt = msckf_amd.MSCKF(aiding=lane_config(), **kw)
        try:
            for m in msgs:
                flt.aiding_callback(to_fix(m))
            traj = replay(flt, st)
            singles.append((traj, list(flt.aid_delayed_log), flt.aid_delayed_count, flt.ctx.get_state(0), list(flt.aid_log),
                            list(flt.cam_times)))
        finally:
            flt.close()
    logs = [s[1] for s in singles]
    assert len(logs[0]) >= 5 and logs[1] == [] and len(logs[2]) >= 15 and all(s[4] == [] for s in singles)
    flat = [e for lg in logs for e in lg]   # under the 95 % gate one fix in twenty is expected to be rejected
    assert all(e[6] in (Dl.APPLIED, Dl.GATED) for e in flat) and sum(e[2] for e in flat) >= 0.8 * len(flat)
    per_frame = {}
    for lg in logs:
        cnt = {}
        for e in lg:
            cnt[e[0]] = cnt.get(e[0], 0) + 1
        for f, c in cnt.items():
            per_frame[f] = max(per_frame.get(f, 0), c)
    assert max(per_frame.values()) == 2
    multi = MultiMSCKF(3, aiding=lane_config(), **kw)
    try:
        for i, msgs in enumerate(lanes):
            for m in msgs:
                multi.aiding_callback(i, to_fix(m))
        trajs = multi.run_streams([st, st, st])
        assert multi.launches["aid_delayed"] == sum(per_frame.values())
        assert "aid" not in multi.launches
        for i, ln in enumerate(multi.lanes):
            t1, log1, cnt1, state1, _, times1 = singles[i]
            assert np.asarray(trajs[i].p).tobytes() == np.asarray(t1.p).tobytes(), i
            assert ln.aid_delayed_log == log1 and ln.aid_delayed_count == cnt1, i
            assert same_state(multi.ctx.get_state(i), state1), i
            assert ln.cam_times == times1 and len(ln.cam_times) == len(ln.cam_ids), i
    finally:
        multi.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_option_off_makes_no_delayed_call(on_device):
    """delayed=False: the stale fixes are dropped as before, no "aid_delayed"
    request exists and the launches are those of a run without the new fields
    in play (the same messages under the parent's AidingConfig)."""
    kw = dict(device_map=True, device_keyframes=True) if on_device else {}
    st = cut_stream(30)
    msgs = lane_messages()[0]
    runs = []
    for cfg in (delayed_config(max_age=0.005, delayed=False),
                AidingConfig(lever=A.LEVER, dir_w=tuple(A.DIR_W), max_age=0.005)):
        multi = MultiMSCKF(2, aiding=cfg, **kw)
        try:
            for m in msgs:
                multi.aiding_callback(0, to_fix(m))
            trajs = multi.run_streams([st, st])
            assert "aid_delayed" not in multi.launches and "aid_delayed_results" not in multi.launches
            assert "aid" not in multi.launches   # every fix is stale
            assert multi.lanes[0].aid_delayed_log == [] and multi.lanes[0].aid_delayed_count == 0
            app, gam, rows, sta, cnt = multi.ctx.aid_delayed_results([0, 1])   # the context never made the workspace
            assert not app.any() and np.isnan(gam).all() and (rows == 0).all() and (sta == Dl.NONE).all()
            runs.append((dict(multi.launches), np.asarray(trajs[0].p).tobytes()))
        finally:
            multi.close()
    assert runs[0] == runs[1]


def test_stereo_vio_smoke():
    """StereoVIO(aiding=AidingConfig(delayed=True)) on tests/frontend_synth.py's
    rectified scene with a loose height fix stamped three frames back at every
    frame: the fixes land on a clone's own time (lambda = 0) or, where that
    clone has been pruned from the six-clone window, between its neighbours;
    the log fills, the records are finite and the poses too."""
    from conftest import golden
    from frontend_ref_scenes import SCENES, scene_config
    import frontend_lanes_ref as lr
    import frontend_synth as fs
    g = golden("frontend_ref")
    W, H = (int(v) for v in g["size"])
    name = SCENES[0]
    frames = lr.stream_frames(fs.texture_fn(int(g[name + "_seed"]), W=W, H=H), W, H, 30, g[name + "_step"],
                              g[name + "_gyro"], float(g[name + "_disparity"]))
    cfg = FilterConfig()
    cfg.max_cam_state_size = 6
    with StereoVIO(cfg, scene_config(g, name), aiding=AidingConfig(delayed=True)) as vio:
        res = []
        for k, (imu, msg) in enumerate(frames):
            for m in imu:
                vio.imu_callback(m)
            if k >= 3:
                vio.aiding_callback(AidingFix(0.05 * (k - 3), position=[0.0, 0.0, 0.0], position_var=100.0,
                                              position_axes=(0, 0, 1)))
            res.append(vio.stereo_callback(msg))
        pub = [r for r in res if r is not None]
        log = vio.aid_delayed_log
        assert len(pub) > 1 and len(log) > 3 and vio.aid_log == []
        print(log)
        assert all(np.isfinite(e[3]) and e[1] == 0x04 and 0.0 <= e[5] < 1.0 and e[6] in (Dl.APPLIED, Dl.GATED)
                   for e in log)
        assert any(e[5] == 0.0 for e in log)   # a clone's own time, unless that clone was pruned meanwhile
        assert vio.aid_delayed_count == sum(e[2] for e in log) > 0
        for r in pub:
            assert np.isfinite(r.pose._vio_t__).all() and np.isfinite(r.pose._vio_R__).all()
        assert vio.launches["filter"]["aid_delayed"] == len(log)
