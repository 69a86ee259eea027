"""The aiding fixes (include/msckf_aid.h) on the GPU against their numpy
restatement tests/aid_ref.py, and through the host classes.

States and covariances come from synth.make_update_problem(N, 4, seed) as in
test_gpu_zupt.py; the reference runs on the state READ BACK from the device, so
the rounding of the input to fp32 is not charged to the kernel.

Tolerances (test_gpu_zupt.py's): fp64 P <= 1e-9 relative and the state to atol
1e-11; gamma to rtol 1e-9 in both dtypes (the gate is computed in fp64 from the
stored values); fp32 P <= 1e-4 relative, the fp32 state to atol 1e-6.  Before a
decision is compared, the reference's gamma is asserted to lie off the gate by
1e-6 relative.

k_aid_apply works on 32 x 32 tiles and D = 21 + 6 N is never a multiple of 32:
N = 1 | 2, 7 | 8, 12 | 13, 17 | 18 and 39 | 40 put D on both sides of 32, 64, 96,
128 and 256 (k_aid_gain's rows per pass); N = 128 is the largest window.
"""
import numpy as np
import pytest

from lifecycle import State, oracle_of
import msckf_amd
from msckf_amd import CHI2_95, AidingConfig, AidingFix, FilterConfig, chi2_threshold, synth
from msckf_amd._lib import Context, aid_fix, unpack_imu
from msckf_amd.replay import FeatureStream, replay
from msckf_amd.scheduler import MultiMSCKF, StereoVIO
import aid_ref as A
from test_aid_ref import MASKS, fix_for, params, stream_config
from test_gpu_zupt import check_against, problem, put, same_state

pytestmark = pytest.mark.gpu


def reference(state, prm, fix):
    """(oracle state after the update, applied, gamma), the gate's margin asserted."""
    st = oracle_of(state)
    pd, gam = A.aid_gamma(st, prm, fix)
    gate = A.gate_of(prm, fix[3])
    if pd:
        assert abs(gam - gate) > 1e-6 * abs(gate), (gam, gate)
    app, gam = A.aid_update(st, prm, fix)
    return st, app, gam


def run_one(ctx, b, prm, fix):
    ctx.aid_batch([b], [aid_fix(*fix)], prm)
    app, gam, rows, cnt = ctx.aid_results([b])
    return bool(app[0]), gam[0], int(rows[0]), int(cnt[0])


# ------------------------------------------------------------------ ABI --

def test_argument_errors_enqueue_nothing():
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(2, 1))
        before = State(*ctx.get_state(0))
        prm = params()
        z, var, dt, _ = fix_for(oracle_of(before), prm, 0xfff, 0)
        nan = float("nan")

        def fx(rows=0xfff, dt=dt, **kw):
            zz, vv = z.copy(), var.copy()
            for k, v in kw.items():
                (zz if k[0] == "z" else vv)[int(k[1:])] = v
            return aid_fix(zz, vv, dt, rows)

        def raw(prm, **kw):
            p = prm.params()
            for k, v in kw.items():
                getattr(p, k)[:] = v
            return p

        bad = [(fx(rows=0), prm), (fx(rows=0x1000), prm), (fx(rows=-1), prm), (fx(v0=0.0), prm), (fx(v11=-1.0), prm),
               (fx(v4=nan), prm), (fx(z7=nan), prm), (fx(dt=-1e-3), prm), (fx(dt=nan), prm),
               (fx(rows=A.BVEL), raw(prm, R_body=[2, 0, 0, 0, 1, 0, 0, 0, 1])),
               (fx(rows=A.BVEL), raw(prm, R_body=[nan] * 9)),
               (fx(rows=A.DIR), raw(prm, dir_w=[1.0, 2e-3, 0.0])),
               (fx(rows=A.POS), raw(prm, chi2=[1.0, 1.0, nan] + [1.0] * 9))]
        for f, p in bad:
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.aid_batch([0], [f], p)
        for fl in ([0, 0], [3], [-1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.aid_batch(fl, [fx()] * len(fl), prm)
        app, gam, rows, cnt = ctx.aid_results([0, 1, 2])   # the records' initial values
        assert not app.any() and np.isnan(gam).all() and (rows == 0).all() and (cnt == 0).all()
        assert same_state(before, State(*ctx.get_state(0)))
        # legal: what the masked rows and the unused groups' parameters hold does not matter
        ok = fx(rows=A.POS, z5=nan, v5=-1.0)
        ctx.aid_batch([0], [ok], raw(prm, R_body=[nan] * 9, dir_w=[0, 0, 0], chi2=[nan, nan, 1e30] + [nan] * 9))
        assert ctx.aid_results([0])[0][0]
    finally:
        ctx.close()


# --------------------------------------------------------------- parity --

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", [0, 1, 2, 7, 8, 12, 13, 17, 18, 39, 40, 128])
def test_window_sizes(N, dtype):
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=max(N, 1), dtype=dtype)
    try:
        put(ctx, 0, problem(N, 500 + N))
        before = State(*ctx.get_state(0))
        fix = fix_for(oracle_of(before), prm, 0xfff, N)
        st, app, gam = reference(before, prm, fix)
        assert app
        got_app, got_gam, rows, cnt = run_one(ctx, 0, prm, fix)
        after = State(*ctx.get_state(0))
        assert got_app == app and cnt == 1 and rows == 0xfff
        np.testing.assert_allclose(got_gam, gam, rtol=1e-9)
        check_against(after, st, dtype)
        np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cap,N", [(12, 3), (128, 5)])
def test_window_below_capacity(cap, N, dtype):
    """The stride of P is Dmax = 21 + 6 cap, not D."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=cap, dtype=dtype)
    try:
        for b in range(2):
            put(ctx, b, problem(N, 600 + cap + b))
        before = [State(*ctx.get_state(b)) for b in range(2)]
        fixes = {b: fix_for(oracle_of(before[b]), prm, 0xfff, cap + b) for b in range(2)}
        ctx.aid_batch([1, 0], [aid_fix(*fixes[1]), aid_fix(*fixes[0])], prm)
        got_app, got_gam, _, _ = ctx.aid_results([1, 0])
        for k, b in enumerate([1, 0]):
            st, app, gam = reference(before[b], prm, fixes[b])
            assert app and got_app[k]
            np.testing.assert_allclose(got_gam[k], gam, rtol=1e-9)
            after = State(*ctx.get_state(b))
            check_against(after, st, dtype, "filter %d " % b)
            np.testing.assert_array_equal(after.P, after.P.T)
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
        z, var, dt, _ = fix_for(oracle_of(before), prm, rows, rows)
        for g in range(12):   # the masked rows' entries are ignored
            if not (rows >> g) & 1:
                z[g], var[g] = np.nan, -1.0
        fix = (z, var, dt, rows)
        st, app, gam = reference(before, prm, fix)
        got_app, got_gam, got_rows, _ = run_one(ctx, 0, prm, fix)
        assert app and got_app and got_rows == rows
        np.testing.assert_allclose(got_gam, gam, rtol=1e-9)
        after = State(*ctx.get_state(0))
        check_against(after, st, dtype)
        np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mixed_batch(dtype):
    """Six slots, filters = [4, 1, 5] with masks POS+VEL, BVEL y+z and all rows
    and ages 0.03, 0, 0.012 in one call under the CHI2_95 gate: slot 1's fix is
    0.5 m/s off and rejected (gamma 71.5 against 5.99; the others 0.30 against
    12.59 and 0.49 against 21.03); slot 5 is updated again by a second call with DIR
    alone.  Rejected and unlisted slots keep every byte; the records say so."""
    prm = params(chi2=None)
    ctx = Context(FilterConfig(), n_filters=6, n_cam_capacity=8, dtype=dtype)
    try:
        for b in range(6):
            put(ctx, b, problem(3 + b, 800 + b))
        before = [State(*ctx.get_state(b)) for b in range(6)]
        fl, masks, ages = [4, 1, 5], [A.POS | A.VEL, 0x180, 0xfff], [0.03, 0.0, 0.012]
        fixes = []
        for b, rows, dt in zip(fl, masks, ages):
            z, var, _, _ = fix_for(oracle_of(before[b]), prm, rows, 40 + b, dt=dt, off=0.02)
            if b == 1:
                z[6:9] += 0.5
            fixes.append((z, var, dt, rows))
        refs = [reference(before[b], prm, f) for b, f in zip(fl, fixes)]
        assert [r[1] for r in refs] == [True, False, True]
        ctx.aid_batch(fl, [aid_fix(*f) for f in fixes], prm)
        app, gam, rows, cnt = ctx.aid_results(fl)
        assert app.tolist() == [True, False, True] and cnt.tolist() == [1, 0, 1] and rows.tolist() == masks
        np.testing.assert_allclose(gam, [r[2] for r in refs], rtol=1e-9)
        mid = [State(*ctx.get_state(b)) for b in range(6)]
        for b in (0, 1, 2, 3):   # unlisted, and slot 1 rejected by gamma
            assert same_state(before[b], mid[b]), b
        for k in (0, 2):
            check_against(mid[fl[k]], refs[k][0], dtype, "slot %d " % fl[k])
            np.testing.assert_array_equal(mid[fl[k]].P, mid[fl[k]].P.T)
        # slot 5 again, DIR alone
        z, var, _, _ = fix_for(oracle_of(mid[5]), prm, A.DIR, 50, off=0.02)
        st5, app5, gam5 = reference(mid[5], prm, (z, var, 0.0, A.DIR))
        assert app5
        ctx.aid_batch([5], [aid_fix(z, var, 0.0, A.DIR)], prm)
        app, gam, rows, cnt = ctx.aid_results([5, 4, 1, 0])
        assert app.tolist() == [True, True, False, False] and cnt.tolist() == [2, 1, 0, 0]
        assert rows.tolist() == [A.DIR, A.POS | A.VEL, 0x180, 0]
        np.testing.assert_allclose(gam[0], gam5, rtol=1e-9)
        check_against(State(*ctx.get_state(5)), st5, dtype, "slot 5 again ")
        for b in range(5):
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
            fixes = [fix_for(oracle_of(State(*ctx.get_state(b))), prm, (0xfff, 0x1ff)[b], 9 + b) for b in range(2)]
            ctx.aid_batch([0, 1], [aid_fix(*f) for f in fixes], prm)
            outs.append([ctx.get_state(b) for b in range(2)] + [ctx.aid_results([0, 1])])
        finally:
            ctx.close()
    for x, y in zip(outs[0], outs[1]):
        assert same_state(x, y)
    assert outs[0][2][0].all()
    for b in range(2):
        np.testing.assert_array_equal(outs[0][b][2], outs[0][b][2].T)


@pytest.mark.parametrize("alias", [True, False])
def test_aliased_nulls_move_with_the_correction(alias):
    """Quirk Q5: with nulls_alias = 1 the record's null velocity and position are
    the corrected ones, with 0 they keep their values."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 950)
        d["imu_p_null"], d["imu_v_null"] = d["imu_p"] + 0.5, d["imu_v"] - 0.25
        put(ctx, 0, d, alias=alias)
        before = unpack_imu(ctx.get_state(0)[0])
        fix = fix_for(oracle_of(State(*ctx.get_state(0))), prm, A.POS | A.VEL, 5)
        assert run_one(ctx, 0, prm, fix)[0]
        s = unpack_imu(ctx.get_state(0)[0])
        assert np.abs(s["v"] - before["v"]).max() > 1e-3 and s["alias"] == alias
        if alias:
            np.testing.assert_array_equal(s["v_null"], s["v"])
            np.testing.assert_array_equal(s["p_null"], s["p"])
        else:
            np.testing.assert_array_equal(s["v_null"], before["v_null"])
            np.testing.assert_array_equal(s["p_null"], before["p_null"])
    finally:
        ctx.close()


@pytest.mark.parametrize("chi2", [0.0, -1.0])
def test_non_positive_chi2_never_applies(chi2):
    prm = params(chi2=chi2)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 960))
        before = State(*ctx.get_state(0))
        app, gam, rows, cnt = run_one(ctx, 0, prm, fix_for(oracle_of(before), prm, 0xfff, 6))
        assert not app and np.isfinite(gam) and gam > 0 and cnt == 0 and rows == 0xfff
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_indefinite_innovation_covariance():
    """P[12, 12] strongly negative through set_state: S is not positive definite,
    gamma is NaN, nothing is applied or written, and that is no error."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 970)
        P = d["P"].copy()
        P[12, 12] = -10.0
        put(ctx, 0, d, P=P)
        before = State(*ctx.get_state(0))
        fix = fix_for(oracle_of(before), prm, 0xfff, 7)
        _, app, gam = reference(before, prm, fix)
        assert not app and np.isnan(gam)
        got_app, got_gam, rows, cnt = run_one(ctx, 0, prm, fix)
        assert not got_app and np.isnan(got_gam) and cnt == 0 and rows == 0xfff
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_kernels_have_stage_timers():
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 980))
        ctx.set_profiling(True)
        run_one(ctx, 0, prm, fix_for(oracle_of(State(*ctx.get_state(0))), prm, 0xfff, 8))
        times = ctx.kernel_times()
        assert times["aid_gain"][1] == 1 and times["aid_apply"][1] == 1
    finally:
        ctx.close()


# --------------------------------------------------------- host classes --

STREAM = dict(n_frames=60, static_s=1.2, seed=0)   # 84 frames, 64 published, a fix before every 4th: 16
FIRST_BLIND = 26
T0 = 100.0 + STREAM["static_s"]
_short = None


def short():
    """(outage sequence, plain oracle records, alignment), computed once."""
    global _short
    if _short is None:
        seq = synth.make_sequence(**STREAM)
        plain = A.run_outage(A.O.OracleMSCKF(FilterConfig(), chi2_threshold), seq, FIRST_BLIND)
        _short = (A.outage_sequence(seq, FIRST_BLIND), plain, A.alignment(plain[0], seq), seq)
    return _short


def to_fix(msg):
    """aid_ref's (t, z, var, rows) as the host class's message."""
    t, z, var, rows = msg
    kw = {}
    for g, name in enumerate(("position", "velocity", "body_velocity", "direction")):
        if (rows >> (3 * g)) & 7:
            kw[name] = z[3 * g:3 * g + 3]
            kw[name + "_var"] = tuple(var[3 * g:3 * g + 3])
            kw[name + "_axes"] = tuple((rows >> (3 * g + ax)) & 1 for ax in range(3))
    return AidingFix(t, **kw)


def test_msckf_with_aiding_follows_the_oracle():
    """MSCKF(aiding=...) in fp64 on the short outage stream (n_frames = 60, no
    features from frame index 26 on, the accelerometer bias, POS + VEL fixes by
    the recipe) against OracleAid, frame by frame: the same decisions (the
    feature gates' and the stacked shapes too), and the pose within the
    sequence tolerance (1e-6 relative; the unit quaternion sets the scale).
    The oracle ends 0.0806 m from the truth without fixes and 0.0152 m with
    them, 16 of 16 applied, the largest gamma 11.72 against the gate 12.59."""
    oseq, plain, Al, seq = short()
    rows = A.POS | A.VEL
    msgs = A.fix_messages(plain[:, 0], T0, Al, rows)
    orc = A.OracleAid(FilterConfig(), chi2_threshold, stream_config())
    ref = A.run_outage(orc, seq, FIRST_BLIND, msgs)
    gate = CHI2_95[5]
    assert len(orc.aid_log) == len(msgs) == 16
    assert all(abs(g - gate) > 1e-3 * gate for _, _, _, g in orc.aid_log)
    flt = msckf_amd.MSCKF(aiding=stream_config())
    try:
        for m in msgs:
            flt.aiding_callback(to_fix(m))
        recs = []
        for kind, m in oseq.events():
            if kind == 0:
                flt.imu_callback(m)
                continue
            if flt.feature_callback(m) is not None:
                s = flt.imu_state()
                recs.append(np.concatenate([[m.timestamp], s["p"], s["v"], s["q"]]))
        rec = np.array(recs)
        assert rec.shape == ref.shape
        assert [(f, r, a) for f, r, a, _ in flt.aid_log] == [(f, r, a) for f, r, a, _ in orc.aid_log]
        assert flt.aid_count == sum(a for _, _, a, _ in orc.aid_log) == 16
        # gamma is quadratic in r; r is ~ 2 sigma = 0.04 and the two states are held to 1e-6: 2 x 1e-6 / 0.04
        np.testing.assert_allclose([g for *_, g in flt.aid_log], [g for *_, g in orc.aid_log], rtol=1e-3)
        assert np.array(flt.gate_log).tolist() == np.array(orc.gate_log).tolist()
        assert np.array(flt.shape_log).tolist() == np.array(orc.shape_log).tolist()
        pose = [1, 2, 3, 7, 8, 9, 10]   # p, q
        for k in range(len(ref)):
            assert np.linalg.norm(rec[k, pose] - ref[k, pose]) <= 1e-6 * np.linalg.norm(ref[k, pose]), k
    finally:
        flt.close()


def lane_messages():
    """Fixes per lane of the scheduler test: POS + VEL before every 4th
    published frame, none, all rows before every 2nd."""
    _, plain, Al, _ = short()
    ft = plain[:24, 0]
    return [A.fix_messages(ft, T0, Al, A.POS | A.VEL), [], A.fix_messages(ft, T0, Al, 0xfff, seed=101, every=2)]


@pytest.mark.parametrize("on_device", [False, True])
def test_scheduler_with_aiding_equals_single_filters(on_device):
    """Three lanes on the first 44 frames of the stream, fixes on lanes 0 and 2
    only: every lane equals its single filter bit for bit, with one "aid"
    launch (and one read of the records) per frame step that has any fix --
    the 12 even published frames -- and none otherwise."""
    kw = dict(device_map=True, device_keyframes=True) if on_device else {}
    oseq = short()[0]
    cut = synth.Sequence([m for m in oseq.imu if m.vio_timestamp__ <= oseq.frames[43].timestamp], oseq.frames[:44],
                         oseq.gt_t[:44], oseq.gt_p[:44], oseq.gt_R[:44])
    st = FeatureStream.from_synthetic(cut)
    lanes = lane_messages()
    singles = []
    for msgs in lanes:
        flt = msckf_amd.MSCKF(aiding=stream_config(), **kw)
        try:
            for m in msgs:
                flt.aiding_callback(to_fix(m))
            traj = replay(flt, st)
            singles.append((traj, list(flt.aid_log), flt.aid_count, flt.ctx.get_state(0)))
        finally:
            flt.close()
    assert [len(s[1]) for s in singles] == [6, 0, 12]
    multi = MultiMSCKF(3, aiding=stream_config(), **kw)
    try:
        for i, msgs in enumerate(lanes):
            for m in msgs:
                multi.aiding_callback(i, to_fix(m))
        trajs = multi.run_streams([st, st, st])
        assert multi.launches["aid"] == multi.launches["aid_results"] == 12
        for i, ln in enumerate(multi.lanes):
            t1, log1, cnt1, state1 = singles[i]
            assert np.asarray(trajs[i].p).tobytes() == np.asarray(t1.p).tobytes(), i
            assert ln.aid_log == log1 and ln.aid_count == cnt1, i
            assert same_state(multi.ctx.get_state(i), state1), i
    finally:
        multi.close()


def test_option_off_makes_no_aid_call():
    oseq = short()[0]
    st = FeatureStream.from_synthetic(synth.Sequence([m for m in oseq.imu if m.vio_timestamp__ <= oseq.frames[29].timestamp],
                                                     oseq.frames[:30], oseq.gt_t[:30], oseq.gt_p[:30], oseq.gt_R[:30]))
    multi = MultiMSCKF(2)
    try:
        multi.run_streams([st, st])
        assert "aid" not in multi.launches and "aid_results" not in multi.launches
        assert multi.lanes[0].aid_log == [] and multi.lanes[0].aid_count == 0
        with pytest.raises(ValueError):
            multi.aiding_callback(0, AidingFix(0.0, position=[0, 0, 0]))
        app, gam, rows, cnt = multi.ctx.aid_results([0, 1])   # the context never made the workspace
        assert not app.any() and np.isnan(gam).all() and (rows == 0).all() and (cnt == 0).all()
    finally:
        multi.close()


def test_stereo_vio_smoke():
    """StereoVIO(aiding=...) on tests/frontend_synth.py's rectified scene with a
    loose position fix at the origin before every published frame: the log
    fills, the records are finite and the poses too."""
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
    with StereoVIO(cfg, scene_config(g, name), aiding=AidingConfig(max_age=1.0)) as vio:
        res = []
        for k, (imu, msg) in enumerate(frames):
            for m in imu:
                vio.imu_callback(m)
            vio.aiding_callback(AidingFix(0.05 * k, position=[0.0, 0.0, 0.0], position_var=100.0,
                                          position_axes=(0, 0, 1)))
            res.append(vio.stereo_callback(msg))
        pub = [r for r in res if r is not None]
        assert len(pub) > 1 and len(vio.aid_log) == len(pub)
        assert all(np.isfinite(g_) and r_ == 0x004 for _, r_, _, g_ in vio.aid_log)
        assert vio.aid_count == sum(a for _, _, a, _ in vio.aid_log) > 0
        for r in pub:
            assert np.isfinite(r.pose._vio_t__).all() and np.isfinite(r.pose._vio_R__).all()
        assert vio.launches["filter"]["aid"] == vio.launches["filter"]["aid_results"] == len(vio.aid_log)
