"""The zero-velocity update (include/msckf_zupt.h) on the GPU against its numpy
restatement tests/zupt_ref.py, and through the host classes.

States and covariances come from synth.make_update_problem(N, 4, seed) as in
test_gpu_parity.py; the reference runs on the state READ BACK from the device,
so the rounding of the input to fp32 is not charged to the kernel.

Tolerances (test_gpu_parity.py's): fp64 P <= 1e-9 relative and the state to
atol 1e-11; gamma to rtol 1e-9 in both dtypes (the gate is computed in fp64
from the stored values); fp32 P <= 1e-4 relative, the fp32 state to atol 1e-6
(dx is computed in fp64 and added in fp32: a few ulps, 6e-8 each, of components
of size <= 1).  Before a decision is compared, the reference's gamma and speed
are asserted to lie off the gate's thresholds by 1e-6 (relative for chi2).

k_zupt_apply works on 32 x 32 tiles and D = 21 + 6 N is never a multiple of 32:
N = 1 | 2, 7 | 8, 12 | 13, 17 | 18 and 39 | 40 put D on both sides of 32, 64, 96,
128 and 256.
"""
import numpy as np
import pytest

from helpers import problem_to_dict
from lifecycle import State, oracle_of
import msckf_amd
from msckf_amd import FilterConfig, ZuptConfig, chi2_threshold, synth
from msckf_amd._lib import Context, MsckfZuptParamsT, pack_cams, pack_imu, unpack_imu
from msckf_amd.replay import FeatureStream, replay
from msckf_amd.scheduler import MultiMSCKF, StereoVIO
import zupt_ref as Z
from test_zupt_ref import MASKS, N_MOVING, N_REST, STREAM

pytestmark = pytest.mark.gpu

FORCE = dict(chi2=1e30, max_speed=1e30)   # every positive definite S is applied


def problem(N, seed, v_scale=1.0):
    """make_update_problem(max(N, 3), 4, seed) cut to N cams (the generator needs three), as a dict."""
    d = problem_to_dict(synth.make_update_problem(max(N, 3), 4, seed))
    D = 21 + 6 * N
    d.update(N=N, cam_q=d["cam_q"][:N], cam_p=d["cam_p"][:N], cam_q_null=d["cam_q_null"][:N],
             P=d["P"][:D, :D].copy(), imu_v=d["imu_v"] * v_scale)
    return d


def put(ctx, b, d, alias=True, P=None):
    imu = pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"], q_null=d["imu_q_null"],
                   p_null=d["imu_p_null"], v_null=d["imu_v_null"], R_imu_cam0=d["imu_R_imu_cam0"],
                   t_cam0_imu=d["imu_t_cam0_imu"], gravity=d["gravity"], alias=alias)
    N = int(d["N"])
    ctx.set_state(b, imu, pack_cams(d["cam_q"], d["cam_p"], d["cam_q_null"]) if N else None, d["P"] if P is None else P)


def means(seed, n=1):
    rng = np.random.default_rng(seed)
    return 0.01 * rng.standard_normal((n, 3)), np.array([0.0, 0.0, 9.81]) + 0.05 * rng.standard_normal((n, 3))


def reference(state, w, a, prm):
    """(oracle state after the update, applied, gamma), the gate's margins asserted."""
    st = oracle_of(state)
    pd, gam = Z.zupt_gamma(st, w, a, prm)
    if pd:
        assert abs(gam - prm.gate()) > 1e-6 * abs(prm.gate()), (gam, prm.gate())
    assert abs(np.linalg.norm(st.imu.v) - prm.max_speed) > 1e-6
    app, gam = Z.zupt_update(st, w, a, prm)
    return st, app, gam


def check_against(got, st, dtype, what=""):
    """The device state ``got`` (a State) against the oracle state ``st``."""
    f64 = np.dtype(dtype) == np.float64
    assert np.linalg.norm(got.P - st.P) <= (1e-9 if f64 else 1e-4) * np.linalg.norm(st.P), what
    atol = 1e-11 if f64 else 1e-6
    s = unpack_imu(np.asarray(got.imu))
    for f in ("q", "p", "v", "bg", "ba", "R_imu_cam0", "t_cam0_imu"):
        np.testing.assert_allclose(s[f], getattr(st.imu, f), atol=atol, err_msg=what + f)
    for k, c in enumerate(st.cams.values()):
        np.testing.assert_allclose(got.cams[k, 0:4], c.q, atol=atol, err_msg=what)
        np.testing.assert_allclose(got.cams[k, 4:7], c.p, atol=atol, err_msg=what)


def same_state(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------ ABI --

def test_argument_errors_enqueue_nothing():
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(2, 1))
        before = State(*ctx.get_state(0))
        w, a = means(0, 2)
        ok = dict(vel_noise=1e-4, gyro_noise=4e-6, acc_noise=4e-4, chi2=1e30, max_speed=1e30, rows=7)
        bad = [dict(rows=0), dict(rows=8), dict(rows=-1), dict(vel_noise=0.0), dict(gyro_noise=-1.0),
               dict(acc_noise=float("nan")), dict(max_speed=-1.0), dict(max_speed=float("nan")),
               dict(chi2=float("nan"))]
        for kw in bad:
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch([0], w[:1], a[:1], MsckfZuptParamsT(*{**ok, **kw}.values()))
        for fl in ([0, 0], [3], [-1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.zupt_batch(fl, w[:len(fl)], a[:len(fl)], MsckfZuptParamsT(*ok.values()))
        app, gam, cnt = ctx.zupt_results([0, 1, 2])   # the records' initial values
        assert not app.any() and np.isnan(gam).all() and (cnt == 0).all()
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


# --------------------------------------------------------------- parity --

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("N", [0, 1, 2, 7, 8, 12, 13, 17, 18, 39, 40, 128])
def test_window_sizes(N, dtype):
    prm = ZuptConfig(**FORCE)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=max(N, 1), dtype=dtype)
    try:
        put(ctx, 0, problem(N, 500 + N))
        before = State(*ctx.get_state(0))
        w, a = means(N)
        st, app, gam = reference(before, w[0], a[0], prm)
        assert app
        ctx.zupt_batch([0], w, a, prm)
        got_app, got_gam, cnt = ctx.zupt_results([0])
        after = State(*ctx.get_state(0))
        assert bool(got_app[0]) == app and cnt[0] == 1
        np.testing.assert_allclose(got_gam[0], gam, rtol=1e-9)
        check_against(after, st, dtype)
        np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cap,N", [(12, 3), (128, 5)])
def test_window_below_capacity(cap, N, dtype):
    """The stride of P is Dmax = 21 + 6 cap, not D."""
    prm = ZuptConfig(**FORCE)
    ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=cap, dtype=dtype)
    try:
        for b in range(2):
            put(ctx, b, problem(N, 600 + cap + b))
        before = [State(*ctx.get_state(b)) for b in range(2)]
        w, a = means(cap, 2)
        ctx.zupt_batch([1, 0], w, a, prm)
        got_app, got_gam, _ = ctx.zupt_results([1, 0])
        for k, b in enumerate([1, 0]):
            st, app, gam = reference(before[b], w[k], a[k], prm)
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
    prm = ZuptConfig(rows=rows, **FORCE)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=6, dtype=dtype)
    try:
        put(ctx, 0, problem(6, 700 + prm.mask()))
        before = State(*ctx.get_state(0))
        w, a = means(prm.mask())
        st, app, gam = reference(before, w[0], a[0], prm)
        ctx.zupt_batch([0], w, a, prm)
        got_app, got_gam, _ = ctx.zupt_results([0])
        assert app and got_app[0]
        np.testing.assert_allclose(got_gam[0], gam, rtol=1e-9)
        after = State(*ctx.get_state(0))
        check_against(after, st, dtype)
        np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mixed_batch(dtype):
    """Six slots, filters = [4, 1, 5]: slot 4 is applied (|v| ~ 2e-3), slot 1 is
    rejected by gamma (v set to 1 m/s along x, max_speed above it), slot 5
    (0.05 m/s) is applied and then rejected by max_speed alone in a second call
    with a huge chi2.  Rejected and unlisted
    slots keep every byte; the records say so."""
    ctx = Context(FilterConfig(), n_filters=6, n_cam_capacity=8, dtype=dtype)
    try:
        for b in range(6):
            d = problem(3 + b, 800 + b, v_scale=0.01)
            if b == 1:
                d["imu_v"] = np.array([1.0, 0.0, 0.0])
            if b == 5:
                d["imu_v"] = np.array([0.0, 0.05, 0.0])
            put(ctx, b, d)
        before = [State(*ctx.get_state(b)) for b in range(6)]
        # resting means per listed filter: the rates the biases explain, the specific force gravity explains
        fl = [4, 1, 5]
        w = np.array([unpack_imu(before[b].imu)["bg"] for b in fl])
        a = np.array([unpack_imu(before[b].imu)["ba"] - Z.O.to_rotation(unpack_imu(before[b].imu)["q"])
                      @ unpack_imu(before[b].imu)["gravity"] for b in fl])
        gate = ZuptConfig(vel_noise=1e-2, chi2=chi2_threshold(9), max_speed=2.0)
        refs = [reference(before[b], w[k], a[k], gate) for k, b in enumerate(fl)]
        assert [r[1] for r in refs] == [True, False, True]
        ctx.zupt_batch(fl, w, a, gate)
        app, gam, cnt = ctx.zupt_results(fl)
        assert app.tolist() == [True, False, True] and cnt.tolist() == [1, 0, 1]
        np.testing.assert_allclose(gam, [r[2] for r in refs], rtol=1e-9)
        mid = [State(*ctx.get_state(b)) for b in range(6)]
        for b in (0, 1, 2, 3):   # unlisted, and slot 1 rejected by gamma
            assert same_state(before[b], mid[b]), b
        for k in (0, 2):
            check_against(mid[fl[k]], refs[k][0], dtype, "slot %d " % fl[k])
        # slot 5 again: what the update left of its 0.05 m/s against max_speed 1e-4, and a huge chi2
        speed = ZuptConfig(vel_noise=1e-2, chi2=1e30, max_speed=1e-4)
        st5, app5, gam5 = reference(mid[5], w[2], a[2], speed)
        assert not app5 and np.isfinite(gam5)
        ctx.zupt_batch([5], w[2:], a[2:], speed)
        app, gam, cnt = ctx.zupt_results([5, 4, 0])
        assert app.tolist() == [False, True, False] and cnt.tolist() == [1, 1, 0]
        np.testing.assert_allclose(gam[0], gam5, rtol=1e-9)
        for b in range(6):
            assert same_state(mid[b], State(*ctx.get_state(b))), b
    finally:
        ctx.close()


# ----------------------------------------------------------- properties --

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_repeat_gives_the_same_bits(dtype):
    outs = []
    for _ in range(2):
        ctx = Context(FilterConfig(), n_filters=2, n_cam_capacity=13, dtype=dtype)
        try:
            for b in range(2):
                put(ctx, b, problem(12 + b, 900 + b))
            w, a = means(9, 2)
            ctx.zupt_batch([0, 1], w, a, ZuptConfig(**FORCE))
            outs.append([ctx.get_state(b) for b in range(2)] + [ctx.zupt_results([0, 1])])
        finally:
            ctx.close()
    for x, y in zip(outs[0], outs[1]):
        assert same_state(x, y)
    for b in range(2):
        np.testing.assert_array_equal(outs[0][b][2], outs[0][b][2].T)


@pytest.mark.parametrize("alias", [True, False])
def test_aliased_nulls_move_with_the_correction(alias):
    """Quirk Q5: with nulls_alias = 1 the record's null velocity and position are
    the corrected ones, with 0 they keep their values."""
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 950)
        d["imu_p_null"], d["imu_v_null"] = d["imu_p"] + 0.5, d["imu_v"] - 0.25
        put(ctx, 0, d, alias=alias)
        before = unpack_imu(ctx.get_state(0)[0])
        w, a = means(5)
        ctx.zupt_batch([0], w, a, ZuptConfig(**FORCE))
        assert ctx.zupt_results([0])[0][0]
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
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 960))
        before = State(*ctx.get_state(0))
        w, a = means(6)
        ctx.zupt_batch([0], w, a, ZuptConfig(chi2=chi2, max_speed=1e30))
        app, gam, cnt = ctx.zupt_results([0])
        assert not app[0] and np.isfinite(gam[0]) and gam[0] > 0 and cnt[0] == 0
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_indefinite_innovation_covariance():
    """P[6, 6] strongly negative through set_state: S is not positive definite,
    gamma is NaN, nothing is applied or written, and that is no error."""
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 970)
        P = d["P"].copy()
        P[6, 6] = -10.0
        put(ctx, 0, d, P=P)
        before = State(*ctx.get_state(0))
        w, a = means(7)
        prm = ZuptConfig(**FORCE)
        _, app, gam = reference(before, w[0], a[0], prm)
        assert not app and np.isnan(gam)
        ctx.zupt_batch([0], w, a, prm)
        got_app, got_gam, cnt = ctx.zupt_results([0])
        assert not got_app[0] and np.isnan(got_gam[0]) and cnt[0] == 0
        assert same_state(before, State(*ctx.get_state(0)))
    finally:
        ctx.close()


def test_kernels_have_stage_timers():
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 980))
        ctx.set_profiling(True)
        w, a = means(8)
        ctx.zupt_batch([0], w, a, ZuptConfig(**FORCE))
        ctx.zupt_results([0])
        times = ctx.kernel_times()
        assert times["zupt_gain"][1] == 1 and times["zupt_apply"][1] == 1
    finally:
        ctx.close()


# --------------------------------------------------------- host classes --

_stream = None


def stream():
    global _stream
    if _stream is None:
        seq = synth.make_sequence(**STREAM)
        _stream = (seq, FeatureStream.from_synthetic(seq))
    return _stream


def run_single(**kw):
    flt = msckf_amd.MSCKF(zupt=ZuptConfig(), **kw)
    try:
        traj = replay(flt, stream()[1])
        return traj, list(flt.zupt_log), flt.zupt_count, flt.ctx.get_state(0)
    finally:
        flt.close()


def test_msckf_with_zupt_follows_the_oracle():
    """MSCKF(zupt=ZuptConfig()) in fp64 on test_zupt_ref.py's stream against
    OracleZupt, frame by frame: the same decisions (the feature gates' and the
    stacked shapes too), and the pose -- position and attitude -- within the
    sequence tolerance (1e-6 relative; the unit quaternion sets the scale).

    Measured on an MI355X: |dp| grows to 6.2e-7, |dq| to 6.2e-8; the velocity,
    which the tolerance does not cover, differs by up to 1.8e-6 in the moving
    frames and gamma by up to 1.9e-5 relative.  The growth is the feature
    updates' on a stream that starts with 2.5 s without parallax, not the new
    kernels' (1e-9 per call, above): the same stream with zupt=None leaves the
    oracle by 4.6e-6 in position and 6.3e-6 in velocity."""
    seq, st = stream()
    orc = Z.OracleZupt(FilterConfig(), chi2_threshold, ZuptConfig())
    ref = Z.run_oracle(orc, seq)
    flt = msckf_amd.MSCKF(zupt=ZuptConfig())
    try:
        recs = []
        for kind, m in seq.events():
            if kind == 0:
                flt.imu_callback(m)
                continue
            if flt.feature_callback(m) is not None:
                s = flt.imu_state()
                recs.append(np.concatenate([[m.timestamp], s["p"], s["v"], s["q"]]))
        rec = np.array(recs)
        assert rec.shape == ref.shape and len(rec) == N_REST + N_MOVING
        assert [(f, a) for f, a, _ in flt.zupt_log] == [(f, a) for f, a, _ in orc.zupt_log]
        # gamma is quadratic in r, and r's velocity rows are ~1e-3 m/s at rest while the two states are held to
        # 1e-6 absolute (below): 2 x 1e-6 / 1e-3
        np.testing.assert_allclose([g for _, _, g in flt.zupt_log], [g for _, _, g in orc.zupt_log], rtol=2e-3)
        assert flt.zupt_count == sum(a for _, a, _ in orc.zupt_log) >= N_REST
        assert np.array(flt.gate_log).tolist() == np.array(orc.gate_log).tolist()
        assert np.array(flt.shape_log).tolist() == np.array(orc.shape_log).tolist()
        pose = [1, 2, 3, 7, 8, 9, 10]   # p, q
        for k in range(len(ref)):
            assert np.linalg.norm(rec[k, pose] - ref[k, pose]) <= 1e-6 * np.linalg.norm(ref[k, pose]), k
    finally:
        flt.close()


@pytest.mark.parametrize("on_device", [False, True])
def test_scheduler_with_zupt_equals_single_filters(on_device):
    """The stream in three lanes of MultiMSCKF(3, zupt=...) equals the single
    filter bit for bit, with one "zupt" launch (and one read of the records) per
    frame step."""
    kw = dict(device_map=True, device_keyframes=True) if on_device else {}
    st = stream()[1]
    t1, log1, cnt1, state1 = run_single(**kw)
    multi = MultiMSCKF(3, zupt=ZuptConfig(), **kw)
    try:
        trajs = multi.run_streams([st, st, st])
        assert multi.launches["zupt"] == multi.launches["zupt_results"] == len(log1) == N_REST + N_MOVING
        assert multi.launches["zupt"] == multi.launches["augment"]
        for i, ln in enumerate(multi.lanes):
            assert np.asarray(trajs[i].p).tobytes() == np.asarray(t1.p).tobytes(), i
            assert ln.zupt_log == log1 and ln.zupt_count == cnt1, i
            assert same_state(multi.ctx.get_state(i), state1), i
    finally:
        multi.close()


def test_option_off_makes_no_zupt_call():
    st = stream()[1]
    multi = MultiMSCKF(2)
    try:
        multi.run_streams([st, st])
        assert "zupt" not in multi.launches and "zupt_results" not in multi.launches
        assert multi.lanes[0].zupt_log == [] and multi.lanes[0].zupt_count == 0
        app, gam, cnt = multi.ctx.zupt_results([0, 1])   # the context never made the workspace
        assert not app.any() and np.isnan(gam).all() and (cnt == 0).all()
    finally:
        multi.close()


def test_stereo_vio_smoke():
    """StereoVIO(zupt=...) on tests/frontend_synth.py's rectified scene: the log
    fills -- one entry per published frame but the first, whose image stamp
    starts the propagation -- and the poses are finite."""
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
    with StereoVIO(cfg, scene_config(g, name), zupt=ZuptConfig()) as vio:
        res = []
        for imu, msg in frames:
            for m in imu:
                vio.imu_callback(m)
            res.append(vio.stereo_callback(msg))
        pub = [r for r in res if r is not None]
        assert len(pub) > 1 and len(vio.zupt_log) == len(pub) - 1
        assert all(np.isfinite(g_) for _, _, g_ in vio.zupt_log)
        assert vio.zupt_count == sum(a for _, a, _ in vio.zupt_log)
        for r in pub:
            assert np.isfinite(r.pose._vio_t__).all() and np.isfinite(r.pose._vio_R__).all()
        assert vio.launches["filter"]["zupt"] == vio.launches["filter"]["zupt_results"] == len(vio.zupt_log)
