"""The anchor fixes (include/msckf_anchor.h) on the GPU against their numpy
restatement tests/anchor_ref.py, and through the host classes.

States and covariances come from synth.make_update_problem(N, 4, seed) as in
test_gpu_zupt.py; the reference runs on the state READ BACK from the device, so
the rounding of the input to fp32 is not charged to the kernel.  The reference
update is the UNCOMPRESSED one (all 4 K' whitened rows): the device's QR is
checked against something that does not contain it.

Tolerances (test_gpu_zupt.py's): fp64 P <= 1e-9 relative and the state to atol
1e-11; fp32 P <= 1e-4 relative, the fp32 state to atol 1e-6; gamma_l to rtol
1e-9 in both dtypes (the gates are computed in fp64 from the stored values).
Before a status is compared, the reference's gamma_l is asserted to lie off
the gate by 1e-6 relative.  Anchors lie 2 to 8 m in front of the state's own
cam0, inside the field of view, with z = zhat + 0.002 * normal
(test_anchor_ref.anchors_for).

k_anchor_apply works on 32 x 32 tiles and D = 21 + 6 N is never a multiple of
32: N = 1 | 2, 7 | 8, 12 | 13, 17 | 18 and 39 | 40 put D on both sides of 32, 64,
96, 128 and 256 (k_anchor_gain's rows per pass); N = 128 is the largest window.
K = 3 is the last anchor count without the QR, 4 the first with it; 64 fills
the wave and the 256 rows of the stack.
"""
import numpy as np
import pytest

from lifecycle import State, oracle_of
import msckf_amd
from msckf_amd import AnchorConfig, AnchorFix, FilterConfig, chi2_threshold, synth
from msckf_amd._lib import Context, pack_anchors, unpack_imu
from msckf_amd.replay import FeatureStream, replay
from msckf_amd.scheduler import MultiMSCKF, StereoVIO
import aid_ref
import anchor_ref as A
from test_anchor_ref import anchors_for, params
from test_gpu_zupt import check_against, problem, put, same_state

pytestmark = pytest.mark.gpu

OBS_VAR = FilterConfig().observation_noise


def dev(prm):
    """The C-ABI parameters of an AnchorConfig with the filter's own observation noise."""
    return prm.params(OBS_VAR)


def reference(state, prm, anchors):
    """(oracle state after the update, applied, used, rows, status, gamma), the gates' margins asserted."""
    st = oracle_of(state)
    assert st.sigma2 == OBS_VAR
    _, gam, _ = A.anchor_gate(st, prm, anchors)
    gate = prm.gate()
    for g in gam[np.isfinite(gam)]:
        assert abs(g - gate) > 1e-6 * abs(gate), (g, gate)
    return (st,) + A.anchor_update(st, prm, anchors)


def run_one(ctx, b, prm, anchors):
    """One call for filter b -> (applied, used, rows, count, status, gamma)."""
    ctx.anchor_batch([b], [anchors], dev(prm))
    app, used, rows, cnt = ctx.anchor_results([b])
    status, gamma = ctx.anchor_status(b)
    return bool(app[0]), int(used[0]), int(rows[0]), int(cnt[0]), status, gamma


def compare_records(got, ref):
    """(applied, used, rows, status, gamma) of the device against the reference's."""
    app, used, rows, status, gamma = got
    r_app, r_used, r_rows, r_status, r_gamma = ref
    assert (app, used, rows) == (r_app, r_used, r_rows)
    assert status.tolist() == r_status.tolist()
    np.testing.assert_allclose(gamma, r_gamma, rtol=1e-9, equal_nan=True)


def check_one(ctx, b, prm, anchors, dtype, before=None, want_applied=True):
    before = State(*ctx.get_state(b)) if before is None else before
    st, *ref = reference(before, prm, anchors)
    assert ref[0] == want_applied
    app, used, rows, cnt, status, gamma = run_one(ctx, b, prm, anchors)
    compare_records((app, used, rows, status, gamma), ref)
    after = State(*ctx.get_state(b))
    if want_applied:
        check_against(after, st, dtype)
        np.testing.assert_array_equal(after.P, after.P.T)
    else:
        assert same_state(before, after)
    return after, cnt


# ------------------------------------------------------------------ ABI --

def test_argument_errors_enqueue_nothing():
    ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(2, 1))
        before = State(*ctx.get_state(0))
        prm = params()
        p, cov, z = anchors_for(oracle_of(before), 2, 0)
        nan, inf = float("nan"), float("inf")

        def anc(**kw):
            a = pack_anchors(p, cov, z)
            for k, v in kw.items():
                a[k][1, int(v[0])] = v[1]
            return a

        def raw(**kw):
            q = dev(prm)
            for k, v in kw.items():
                setattr(q, k, v)
            return q

        bad = [(anc(p_w=(0, nan)), raw()), (anc(p_w=(2, inf)), raw()), (anc(z=(3, nan)), raw()), (anc(z=(0, -inf)), raw()),
               (anc(cov=(1, nan)), raw()), (anc(cov=(0, -1e-6)), raw()), (anc(cov=(3, -1.0)), raw()),
               (anc(cov=(5, -1.0)), raw()), (anc(), raw(obs_var=0.0)), (anc(), raw(obs_var=nan)),
               (anc(), raw(min_depth=0.0)), (anc(), raw(min_depth=nan)), (anc(), raw(min_anchors=0)),
               (anc(), raw(chi2=nan))]
        for a, q in bad:
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.anchor_batch([0], [a], q)
        for fl in ([0, 0], [3], [-1]):
            with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):
                ctx.anchor_batch(fl, [anc()] * len(fl), raw())
        with pytest.raises(msckf_amd.MsckfError, match="rc=-1"):   # K = 65
            ctx.anchor_batch([0], [anchors_for(oracle_of(before), 65, 1)], raw())
        # the offsets, through the library itself
        import ctypes as C
        from msckf_amd._lib import MsckfAnchorT
        a2 = anc()
        q = raw()
        for off in ([1, 2], [0, -1], [0, 65]):
            fl, o = np.array([0], np.int32), np.array(off, np.int32)
            rc = ctx.lib.msckf_anchor_batch(ctx.h, 1, fl.ctypes.data_as(C.POINTER(C.c_int32)),
                                            o.ctypes.data_as(C.POINTER(C.c_int32)),
                                            a2.ctypes.data_as(C.POINTER(MsckfAnchorT)), C.byref(q))
            assert rc == -1, off
        rc = ctx.lib.msckf_anchor_batch(ctx.h, 1, np.array([0], np.int32).ctypes.data_as(C.POINTER(C.c_int32)),
                                        np.array([0, 2], np.int32).ctypes.data_as(C.POINTER(C.c_int32)), None,
                                        C.byref(q))
        assert rc == -1
        app, used, rows, cnt = ctx.anchor_results([0, 1, 2])   # the records' initial values
        assert not app.any() and (used == 0).all() and (rows == 0).all() and (cnt == 0).all()
        assert [len(x) for x in ctx.anchor_status(0)] == [0, 0]
        assert same_state(before, State(*ctx.get_state(0)))
        ctx.anchor_batch([], [], raw())   # nfilt == 0 is a no-op
        # legal: an indefinite off-diagonal, chi2 <= 0
        ctx.anchor_batch([0], [anc(cov=(1, 0.5))], raw(chi2=-1.0))
        assert not ctx.anchor_results([0])[0][0] and len(ctx.anchor_status(0)[0]) == 2
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
        _, cnt = check_one(ctx, 0, prm, anchors_for(oracle_of(before), 8, N), dtype, before)
        assert cnt == 1
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
        anchors = {b: anchors_for(oracle_of(before[b]), 8, cap + b) for b in range(2)}
        ctx.anchor_batch([1, 0], [anchors[1], anchors[0]], dev(prm))
        app, used, rows, _ = ctx.anchor_results([1, 0])
        for k, b in enumerate([1, 0]):
            st, *ref = reference(before[b], prm, anchors[b])
            compare_records((bool(app[k]), int(used[k]), int(rows[k])) + ctx.anchor_status(b), ref)
            assert ref[0]
            after = State(*ctx.get_state(b))
            check_against(after, st, dtype, "filter %d " % b)
            np.testing.assert_array_equal(after.P, after.P.T)
    finally:
        ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 16, 63, 64])
def test_anchor_counts(K, dtype):
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=7, dtype=dtype)
    try:
        put(ctx, 0, problem(7, 700 + K))
        before = State(*ctx.get_state(0))
        anchors = anchors_for(oracle_of(before), K, K)
        check_one(ctx, 0, prm, anchors, dtype, before)
        app, used, rows, _ = ctx.anchor_results([0])
        assert used[0] == K and rows[0] == min(4 * K, 12)
    finally:
        ctx.close()


def mixed_anchors(st):
    """One each of USED / GATED / DEPTH for the state ``st``."""
    p, cov, z = anchors_for(st, 3, 77)
    _, R0, t0, _, _ = A.geometry(st)
    p[1] = p[1] + 3.0 * R0[0]        # displaced across the viewing direction
    p[2] = t0 - 3.0 * R0[2]          # behind the camera
    return p, cov, z


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_mixed_batch(dtype):
    """Six slots, filters = [4, 1, 5, 0, 3] with K = 5, 0, 64, 1 and a filter
    whose anchors are one each of USED / GATED / DEPTH, in one call under the
    CHI2_95 gate.  Every record and per-anchor status is compared; the filter
    with K = 0 and the unlisted one keep every bit."""
    prm = params(chi2=None)
    ctx = Context(FilterConfig(), n_filters=6, n_cam_capacity=8, dtype=dtype)
    try:
        for b in range(6):
            put(ctx, b, problem(3 + b, 800 + b))
        before = [State(*ctx.get_state(b)) for b in range(6)]
        fl, counts = [4, 1, 5, 0, 3], [5, 0, 64, 1, None]
        anchors = [mixed_anchors(oracle_of(before[b])) if k is None else anchors_for(oracle_of(before[b]), k, 40 + b)
                   for b, k in zip(fl, counts)]
        refs = [reference(before[b], prm, a) for b, a in zip(fl, anchors)]
        assert [r[1] for r in refs] == [True, False, True, True, True]
        assert refs[4][4].tolist() == [A.USED, A.GATED, A.DEPTH]
        ctx.anchor_batch(fl, anchors, dev(prm))
        app, used, rows, cnt = ctx.anchor_results(fl)
        assert cnt.tolist() == [1, 0, 1, 1, 1]
        after = [State(*ctx.get_state(b)) for b in range(6)]
        for k, b in enumerate(fl):
            compare_records((bool(app[k]), int(used[k]), int(rows[k])) + ctx.anchor_status(b), refs[k][1:])
            if refs[k][1]:
                check_against(after[b], refs[k][0], dtype, "slot %d " % b)
                np.testing.assert_array_equal(after[b].P, after[b].P.T)
        assert rows.tolist() == [12, 0, 12, 4, 4] and used.tolist() == [5, 0, 64, 1, 1]
        for b in (1, 2):   # K = 0, and unlisted
            assert same_state(before[b], after[b]), b
        assert len(ctx.anchor_status(2)[0]) == 0
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
            anchors = [anchors_for(oracle_of(State(*ctx.get_state(b))), (64, 3)[b], 9 + b) for b in range(2)]
            ctx.anchor_batch([0, 1], anchors, dev(prm))
            outs.append([ctx.get_state(b) for b in range(2)] + [ctx.anchor_results([0, 1])]
                        + [ctx.anchor_status(b) for b in range(2)])
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
        p, cov, z = anchors_for(oracle_of(State(*ctx.get_state(0))), 6, 5)
        z = z + 0.02   # a common offset: the correction is not tiny
        assert run_one(ctx, 0, prm, (p, cov, z))[0]
        s = unpack_imu(ctx.get_state(0)[0])
        assert np.abs(s["p"] - before["p"]).max() > 1e-3 and s["alias"] == alias
        if alias:
            np.testing.assert_array_equal(s["v_null"], s["v"])
            np.testing.assert_array_equal(s["p_null"], s["p"])
        else:
            np.testing.assert_array_equal(s["v_null"], before["v_null"])
            np.testing.assert_array_equal(s["p_null"], before["p_null"])
    finally:
        ctx.close()


@pytest.mark.parametrize("kw", [dict(chi2=0.0), dict(chi2=-1.0), dict(chi2=None, min_anchors=6)])
def test_gate_and_min_anchors_write_nothing(kw):
    """A chi2 <= 0 uses no anchor; five used anchors do not reach min_anchors =
    6: the records say so and the state keeps every bit."""
    prm = params(**kw)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 960))
        before = State(*ctx.get_state(0))
        _, cnt = check_one(ctx, 0, prm, anchors_for(oracle_of(before), 5, 6), np.float64, before, want_applied=False)
        app, used, rows, _ = ctx.anchor_results([0])
        assert cnt == 0 and (used[0], rows[0]) == ((5, 12) if "min_anchors" in kw else (0, 0))
        assert ctx.anchor_status(0)[0].tolist() == [A.USED if "min_anchors" in kw else A.GATED] * 5
    finally:
        ctx.close()


def test_indefinite_covariance():
    """P[12, 12] strongly negative through set_state: every S_l is not positive
    definite, the statuses are NOT_PD with NaN gammas, nothing is applied or
    written, and that is no error."""
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        d = problem(4, 970)
        P = d["P"].copy()
        P[12, 12] = -10.0
        put(ctx, 0, d, P=P)
        before = State(*ctx.get_state(0))
        check_one(ctx, 0, prm, anchors_for(oracle_of(before), 4, 7), np.float64, before, want_applied=False)
        status, gamma = ctx.anchor_status(0)
        assert status.tolist() == [A.NOT_PD] * 4 and np.isnan(gamma).all()
    finally:
        ctx.close()


def test_kernels_have_stage_timers():
    prm = params()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=4)
    try:
        put(ctx, 0, problem(4, 980))
        ctx.set_profiling(True)
        run_one(ctx, 0, prm, anchors_for(oracle_of(State(*ctx.get_state(0))), 8, 8))
        times = ctx.kernel_times()
        assert times["anchor_gain"][1] == 1 and times["anchor_apply"][1] == 1
    finally:
        ctx.close()


# --------------------------------------------------------- host classes --

STREAM = dict(n_frames=40, static_s=1.2, seed=0)   # 64 frames, 44 published, a message at every 4th: 11
FIRST_BLIND = 36
T0 = 100.0 + STREAM["static_s"]
_short = None


def short():
    """(outage sequence, plain oracle records, alignment, sequence), computed once."""
    global _short
    if _short is None:
        seq = synth.make_sequence(**STREAM)
        plain = aid_ref.run_outage(A.O.OracleMSCKF(FilterConfig(), chi2_threshold), seq, FIRST_BLIND)
        _short = (aid_ref.outage_sequence(seq, FIRST_BLIND), plain, aid_ref.alignment(plain[0], seq), seq)
    return _short


def to_fix(msg):
    t, p, cov, z = msg
    return AnchorFix(t, p, z, cov)


def test_msckf_with_anchors_follows_the_oracle():
    """MSCKF(anchors=...) in fp64 on a 40-frame outage stream (no features from
    frame index 36 on, the accelerometer bias, eight anchors by the recipe at
    every 4th published frame) against OracleAnchor, frame by frame: the same
    decisions (the feature gates' and the stacked shapes too), and the pose
    within the sequence tolerance (1e-6 relative; the unit quaternion sets the
    scale).  The last message's gammas to atol 1e-4: gamma = |y|^2 with y = L^-1
    r, |y| <= 0.2 (gamma <= 0.04 on this stream), and a state held to 1e-6 moves
    r by <= 2e-6 and y by <= 2e-6 / sqrt(obs_var) = 6e-5: 2 x 0.2 x 6e-5."""
    oseq, plain, Al, seq = short()
    msgs, _, _ = A.anchor_messages(plain[:, 0], T0, Al, FilterConfig())
    orc = A.OracleAnchor(FilterConfig(), chi2_threshold, AnchorConfig())
    ref = A.run_outage(orc, seq, FIRST_BLIND, msgs)
    assert len(orc.anchor_log) == len(msgs) == 11 and orc.anchor_dropped == 0
    assert max(np.nanmax(g) for _, g in orc.anchor_records) < 0.04
    flt = msckf_amd.MSCKF(anchors=AnchorConfig())
    try:
        for m in msgs:
            flt.anchor_callback(to_fix(m))
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
        assert flt.anchor_log == orc.anchor_log and flt.anchor_dropped == 0
        assert flt.anchor_count == sum(a for *_, a in orc.anchor_log) == 11
        status, gamma = flt.anchor_status()
        assert status.tolist() == orc.anchor_records[-1][0].tolist()
        np.testing.assert_allclose(gamma, orc.anchor_records[-1][1], rtol=0, atol=1e-4)
        assert np.array(flt.gate_log).tolist() == np.array(orc.gate_log).tolist()
        assert np.array(flt.shape_log).tolist() == np.array(orc.shape_log).tolist()
        pose = [1, 2, 3, 7, 8, 9, 10]   # p, q
        for k in range(len(ref)):
            assert np.linalg.norm(rec[k, pose] - ref[k, pose]) <= 1e-6 * np.linalg.norm(ref[k, pose]), k
        with pytest.raises(ValueError):   # more than 64 anchors in a message
            flt.anchor_callback(AnchorFix(0.0, np.zeros((65, 3)), np.zeros((65, 4))))
    finally:
        flt.close()


def lane_messages():
    """Messages per lane of the scheduler test: at every 4th published frame,
    none, at every 2nd (another seed); the first two messages of lane 0 lie
    before the stream's first frame and between two frames: dropped."""
    _, plain, Al, _ = short()
    ft = plain[:24, 0]
    a = A.anchor_messages(ft, T0, Al, FilterConfig())[0]
    stray = [(ft[0] - 1.0,) + a[0][1:], (ft[1] + 0.01,) + a[0][1:]]
    return [stray + a, [], A.anchor_messages(ft, T0, Al, FilterConfig(), seed=201, every=2)[0]]


@pytest.mark.parametrize("on_device", [False, True])
def test_scheduler_with_anchors_equals_single_filters(on_device):
    """Three lanes on the first 44 frames of the stream, messages on lanes 0 and
    2 only: every lane equals its single filter bit for bit, with one "anchor"
    launch (and one read of the records) per frame step that has any message
    -- the 12 even published frames -- and none otherwise."""
    kw = dict(device_map=True, device_keyframes=True) if on_device else {}
    oseq = short()[0]
    cut = synth.Sequence([m for m in oseq.imu if m.vio_timestamp__ <= oseq.frames[43].timestamp], oseq.frames[:44],
                         oseq.gt_t[:44], oseq.gt_p[:44], oseq.gt_R[:44])
    st = FeatureStream.from_synthetic(cut)
    lanes = lane_messages()
    singles = []
    for msgs in lanes:
        flt = msckf_amd.MSCKF(anchors=AnchorConfig(), **kw)
        try:
            for m in msgs:
                flt.anchor_callback(to_fix(m))
            traj = replay(flt, st)
            singles.append((traj, list(flt.anchor_log), flt.anchor_count, flt.ctx.get_state(0), flt.anchor_dropped))
        finally:
            flt.close()
    assert [len(s[1]) for s in singles] == [6, 0, 12] and [s[4] for s in singles] == [2, 0, 0]
    assert all(a for *_, a in singles[0][1] + singles[2][1])
    multi = MultiMSCKF(3, anchors=AnchorConfig(), **kw)
    try:
        for i, msgs in enumerate(lanes):
            for m in msgs:
                multi.anchor_callback(i, to_fix(m))
        trajs = multi.run_streams([st, st, st])
        assert multi.launches["anchor"] == multi.launches["anchor_results"] == 12
        for i, ln in enumerate(multi.lanes):
            t1, log1, cnt1, state1, drop1 = singles[i]
            assert np.asarray(trajs[i].p).tobytes() == np.asarray(t1.p).tobytes(), i
            assert ln.anchor_log == log1 and ln.anchor_count == cnt1 and ln.anchor_dropped == drop1, i
            assert same_state(multi.ctx.get_state(i), state1), i
    finally:
        multi.close()


def test_option_off_makes_no_anchor_call():
    """Without the option, and with it but without a message, the launches and
    the trajectories are those of the plain scheduler."""
    oseq = short()[0]
    st = FeatureStream.from_synthetic(synth.Sequence([m for m in oseq.imu if m.vio_timestamp__ <= oseq.frames[29].timestamp],
                                                     oseq.frames[:30], oseq.gt_t[:30], oseq.gt_p[:30], oseq.gt_R[:30]))
    runs = []
    for kw in ({}, dict(anchors=AnchorConfig())):
        multi = MultiMSCKF(2, **kw)
        try:
            trajs = multi.run_streams([st, st])
            assert "anchor" not in multi.launches and "anchor_results" not in multi.launches
            assert multi.lanes[0].anchor_log == [] and multi.lanes[0].anchor_count == 0
            if not kw:
                with pytest.raises(ValueError):
                    multi.anchor_callback(0, AnchorFix(0.0, np.zeros((1, 3)), np.zeros((1, 4))))
            app, used, rows, cnt = multi.ctx.anchor_results([0, 1])   # the context never made the workspace
            assert not app.any() and (used == 0).all() and (rows == 0).all() and (cnt == 0).all()
            assert len(multi.ctx.anchor_status(0)[0]) == 0
            runs.append((dict(multi.launches), [np.asarray(t.p).tobytes() for t in trajs]))
        finally:
            multi.close()
    assert runs[0] == runs[1]


def test_stereo_vio_smoke():
    """StereoVIO(anchors=...) on tests/frontend_synth.py's rectified scene with
    three loosely surveyed anchors placed in front of the filter's own camera
    at every frame: the log fills, anchors are used and the poses are finite."""
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
    with StereoVIO(cfg, scene_config(g, name), anchors=AnchorConfig()) as vio:
        res = []
        for k, (imu, msg) in enumerate(frames):
            for m in imu:
                vio.imu_callback(m)
            p, cov, z = anchors_for(oracle_of(State(*vio.filter.ctx.get_state(0))), 3, k, sigma=0.5)
            vio.anchor_callback(AnchorFix(0.05 * k, p, z, cov))
            res.append(vio.stereo_callback(msg))
        pub = [r for r in res if r is not None]
        assert len(pub) > 1 and len(vio.anchor_log) == len(pub)
        assert all(n == 3 for _, n, _, _ in vio.anchor_log)
        assert vio.anchor_count == sum(a for *_, a in vio.anchor_log) > 0
        assert len(vio.anchor_status()[0]) == 3
        for r in pub:
            assert np.isfinite(r.pose._vio_t__).all() and np.isfinite(r.pose._vio_R__).all()
        assert vio.launches["filter"]["anchor"] == vio.launches["filter"]["anchor_results"] == len(vio.anchor_log)
