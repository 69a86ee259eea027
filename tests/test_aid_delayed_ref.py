"""The numpy restatement of include/msckf_aid_delayed.h (tests/aid_delayed_ref.py)
checked on the CPU: the Jacobian of the interpolated-clone measurement by central
differences through the oracle's apply_correction, the update against the
oracle's measurement_update, the routing of late messages on a hand-made clone
list, and the behaviour on the outage stream with fixes delivered 0.2 s late.
"""
import numpy as np
import pytest

from oracle import msckf_oracle as O
from msckf_amd import CHI2_95, AidingConfig, AidingFix, FilterConfig, chi2_threshold, synth
import aid_ref as A
import aid_delayed_ref as Dl
from test_aid_ref import FIRST_BLIND, STREAM, outage_runs, rot, stream_config
from test_zupt_ref import make_state

LEVER = (0.10, -0.05, 0.20)
MASKS = [Dl.POS, Dl.DIR, 0x04, Dl.POS | Dl.DIR]


def params(**kw):
    d = np.array([0.6, -0.64, 0.48])
    return AidingConfig(**{**dict(lever=LEVER, dir_w=tuple(d), chi2=1e30), **kw})


def set_clone_rotation(st, slot, phi):
    """Clone slot + 1's rotation becomes Exp(phi) R_slot; phi None copies the
    quaternion, so the two rotations are identical to the bit."""
    cams = list(st.cams.values())
    if phi is None:
        cams[slot + 1].q = cams[slot].q.copy()
    else:
        cams[slot + 1].q = O.to_quaternion(Dl.so3_exp(np.asarray(phi, float)) @ O.to_rotation(cams[slot].q))


def fix_for(st, prm, rows, slot, lam, seed, off=0.05):
    """A fix near the state's own prediction: z = h(x) + off * normal, var (0.02 .. 0.04)^2."""
    rng = np.random.default_rng(seed)
    z = Dl.predict(st, prm, slot, lam) + off * rng.standard_normal(6)
    return z, (0.02 + 0.02 * rng.random(6)) ** 2, slot, lam, rows


AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


@pytest.mark.parametrize("lever", [(0.0, 0.0, 0.0), LEVER])
@pytest.mark.parametrize("angle", [None, 1e-9, 0.3])
@pytest.mark.parametrize("lam", [0.0, 0.37, 0.999])
def test_jacobian_by_finite_differences(lam, angle, lever):
    """h(x [+] dx) = h(x) + H dx to first order, the correction being the
    oracle's apply_correction: central differences of all six predictions, step
    1e-6 (truncation ~1e-12, rounding ~1e-16 / 1e-6 ~ 1e-10), asserted at
    test_anchor_ref's atol 1e-7.  The clone-to-clone rotation is exactly 0 (the
    series branch at phi = 0), 1e-9 rad and 0.3 rad.  Found over the 18 cases:
    max |H - J| between 8.8e-11 and 1.5e-10, so the header's formula for
    dtheta_c holds as derived.  H is exactly 0 outside 15:21 and the clones'
    columns, and outside clone s's with lambda = 0."""
    prm = params(lever=lever)
    st = make_state(N=4)
    slot = 1
    set_clone_rotation(st, slot, None if angle is None else angle * AXIS)
    fix = fix_for(st, prm, 0x3f, slot, lam, 1)
    H, r, nz = Dl.rows_of(st, prm, fix)
    D = st.P.shape[0]
    assert H.shape == (6, D) and r.shape == nz.shape == (6,)
    h = 1e-6
    J = np.zeros_like(H)
    for c in range(D):
        dx = np.zeros(D)
        dx[c] = h
        sp, sm = st.copy(), st.copy()
        O.apply_correction(sp, dx)
        O.apply_correction(sm, -dx)
        J[:, c] = (Dl.predict(sp, prm, slot, lam) - Dl.predict(sm, prm, slot, lam)) / (2 * h)
    print("lam %g angle %s lever %s: max |H| %.3f  max |H - J| %.2e" % (lam, angle, lever, np.abs(H).max(),
                                                                        np.abs(H - J).max()))
    assert np.isfinite(H).all()
    np.testing.assert_allclose(H, J, atol=1e-7)
    c0 = 21 + 6 * slot
    touched = list(range(15, 21)) + list(range(c0, c0 + (6 if lam == 0.0 else 12)))
    assert np.abs(H[:, [c for c in range(D) if c not in touched]]).max() == 0.0


def test_interpolation_ends():
    """dtheta_c is dtheta_s at lambda = 0 and tends to dtheta_{s+1} at lambda = 1."""
    st = make_state(N=4)
    set_clone_rotation(st, 1, 0.3 * AXIS)
    _, _, A0, A1 = Dl.interpolate(st, 1, 0.0)
    assert (A0 == np.eye(3)).all() and (A1 == 0).all()
    Rc, pc, A0, A1 = Dl.interpolate(st, 1, 1.0 - 1e-12)
    cams = list(st.cams.values())
    np.testing.assert_allclose(A0, 0, atol=1e-11)
    np.testing.assert_allclose(A1, np.eye(3), atol=1e-11)
    np.testing.assert_allclose(Rc, O.to_rotation(cams[2].q), atol=1e-11)
    np.testing.assert_allclose(pc, cams[2].p, atol=1e-11)
    for phi in (np.zeros(3), 1e-9 * AXIS, 0.3 * AXIS, 2.0 * AXIS):
        np.testing.assert_allclose(Dl.so3_log(Dl.so3_exp(phi)), phi, rtol=1e-12, atol=1e-25)
        np.testing.assert_allclose(Dl.so3_jl(phi) @ Dl.so3_jl_inv(phi), np.eye(3), atol=1e-14)


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.37])
@pytest.mark.parametrize("rows", MASKS)
def test_update_is_measurement_update_of_whitened_rows(rows, lam, alias):
    """The oracle's own update is the yardstick, as in test_aid_ref."""
    prm = params()
    st = make_state(alias=alias)
    fix = fix_for(st, prm, rows, 2, lam, 2 + rows)
    ref = st.copy()
    H, r, nz = Dl.rows_of(ref, prm, fix)
    Wh = np.sqrt(ref.sigma2 / nz)
    O.measurement_update(ref, Wh[:, None] * H, Wh * r)
    app, gam, status = Dl.update(st, prm, fix)
    assert app and np.isfinite(gam) and status == Dl.APPLIED
    assert np.linalg.norm(st.P - ref.P) <= 1e-12 * np.linalg.norm(ref.P)
    np.testing.assert_array_equal(st.P, st.P.T)
    for f in ("q", "p", "v", "bg", "ba", "R_imu_cam0", "t_cam0_imu", "v_null", "p_null"):
        np.testing.assert_allclose(getattr(st.imu, f), getattr(ref.imu, f), atol=1e-13, err_msg=f)
    for c, cr in zip(st.cams.values(), ref.cams.values()):
        np.testing.assert_allclose(c.q, cr.q, atol=1e-13)
        np.testing.assert_allclose(c.p, cr.p, atol=1e-13)


def test_not_applied_leaves_the_state_alone():
    st = make_state()
    before = st.copy()
    fix = fix_for(st, params(), 0x3f, 1, 0.5, 3)
    for prm, f, want in ((params(chi2=0.0), fix, Dl.GATED), (params(), fix[:2] + (4, 0.0, 0x3f), Dl.BAD_SLOT),
                         (params(), fix[:2] + (3, 0.5, 0x3f), Dl.BAD_SLOT)):
        app, gam, status = Dl.update(st, prm, f)
        assert not app and status == want and np.isnan(gam) == (want == Dl.BAD_SLOT)
        np.testing.assert_array_equal(st.P, before.P)
    st.P[21 + 6 + 3, 21 + 6 + 3] = -10.0
    app, gam, status = Dl.update(st, params(), fix)
    assert not app and np.isnan(gam) and status == Dl.NOT_PD
    np.testing.assert_array_equal(st.imu.p, before.imu.p)
    assert Dl.update(st, params(), fix[:2] + (3, 0.0, 0x3f))[0]   # lambda = 0 on the last clone is legal


def test_abi_symbols_and_structs():
    """include/msckf_aid_delayed.h's entry points are exported by the library and
    typed one to one by the binding, in a list of their own."""
    import ctypes
    import os
    import re
    from msckf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "msckf_aid_delayed.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(msckf_aid_delayed_[a-z]+)\s*\(", src)))
    assert syms == sorted(_lib.AID_DELAYED_EXPORTED) == ["msckf_aid_delayed_batch", "msckf_aid_delayed_results"]
    assert not set(syms) & (set(_lib.EXPORTED) | set(_lib.AID_EXPORTED) | set(_lib.ANCHOR_EXPORTED))
    lib = _lib.load_library()
    for s in syms:
        assert getattr(lib, s).restype is ctypes.c_int
    F = _lib.MsckfAidDelayedFixT
    assert ctypes.sizeof(F) == 14 * 8 and (F.lam.offset, F.rows.offset, F.slot.offset) == (96, 104, 108)
    for name, val in re.findall(r"#define MSCKF_AID_DELAYED_([A-Z_]+)\s+\(?(-?(?:0x)?[0-9a-f]+)\)?", src):
        assert getattr(_lib, "AID_DELAYED_" + name) == int(val, 0) == getattr(Dl, name), name
    assert (_lib.AID_DELAYED_POS, _lib.AID_DELAYED_DIR, _lib.AID_DELAYED_BAD_SLOT) == (0x07, 0x38, 3)


# ---------------------------------------------------------------- routing --

CAM_TIMES = [10.00, 10.05, 10.10, 10.30, 10.35]   # a 0.2 s hole between slots 2 and 3


@pytest.mark.parametrize("which", ["ref", "config"])
def test_routing_covers_every_branch(which):
    cfg = AidingConfig(delayed=True)
    assert (cfg.max_age, cfg.max_delay, cfg.max_gap) == (0.05, 1.0, 0.15) and not AidingConfig().delayed

    def route(t, rows, t_frame, times=CAM_TIMES, cfg=cfg):
        return Dl.route(t, rows, t_frame, times, cfg) if which == "ref" else cfg.route(t, rows, t_frame, times)

    tf = 10.40
    assert route(10.36, A.POS, tf) == ("current",)                        # age <= max_age: today's path
    assert route(10.05 + 5e-10, A.POS | A.VEL, tf) == ("delayed", 1, 0.0, Dl.POS, A.VEL)   # a clone's own time
    assert route(10.35, A.POS, 10.45) == ("delayed", 4, 0.0, Dl.POS, 0)   # the newest clone, lambda = 0
    kind, s, lam, rows, other = route(10.07, A.POS | A.DIR | A.BVEL, tf)  # inside a gap
    assert (kind, s, rows, other) == ("delayed", 0 + 1, Dl.POS | Dl.DIR, A.BVEL) and abs(lam - 0.4) < 1e-9
    kind, s, lam, rows, other = route(10.32, 0x004 | 0x400, tf)           # single axes keep their bits
    assert (kind, s, rows) == ("delayed", 3, 0x04 | 0x10) and abs(lam - 0.4) < 1e-9
    assert route(10.2, A.POS, tf) == ("drop", "clones too far apart")     # gap > max_gap
    assert route(9.99, A.POS, tf) == ("drop", "older than the window")
    assert route(9.30, A.POS, tf, [9.0] + CAM_TIMES) == ("drop", "older than max_delay")
    assert route(10.2, A.VEL | A.BVEL, tf) == ("drop", "no delayed rows")  # a VEL-only stale fix
    assert route(10.38, A.POS, 10.45) == ("wait",)                        # newer than the newest clone: waits ...
    kind, s, lam, _, _ = route(10.38, A.POS, 10.50, CAM_TIMES + [10.45])  # ... and the next frame brackets it
    assert (kind, s) == ("delayed", 4) and abs(lam - 0.3) < 1e-9
    assert route(10.2, A.POS, tf, [], cfg) == ("drop", "older than the window")
    off = AidingConfig()
    for t in (10.07, 10.05, 10.38, 10.2):                                 # delayed=False: dropped, as on the parent
        got = Dl.route(t, A.POS, 10.45, CAM_TIMES, off) if which == "ref" else off.route(t, A.POS, 10.45, CAM_TIMES)
        assert got == ("drop", "stale")
    for bad in (dict(max_delay=-1.0), dict(max_gap=0.0), dict(max_gap=float("nan"))):
        with pytest.raises(ValueError):
            AidingConfig(**bad).params()


def test_oracle_class_routes_waits_and_drops():
    """OracleAidDelayed on a short stream with hand-placed messages: one at a
    clone's time, one in a gap, one that waits a frame, a VEL-only stale one and
    one older than the window."""
    seq = synth.make_sequence(n_frames=12, static_s=1.2, seed=1)
    cfg = AidingConfig(delayed=True, chi2=1e30, max_age=0.01)
    orc = Dl.OracleAidDelayed(FilterConfig(), chi2_threshold, cfg)
    ft = [f.timestamp for f in seq.frames]
    pub = [t for t in ft if t >= seq.imu[199].vio_timestamp__]   # gravity is set at the 200th sample
    z, var = np.zeros(12), np.ones(12)
    late = [(pub[5], (pub[3], z, var, A.POS)),                    # a clone's own time
            (pub[5], (0.5 * (pub[3] + pub[4]), z, var, A.POS | A.VEL)),   # inside a gap
            (pub[5] - 0.001, (pub[4] + 0.02, z, var, A.POS)),     # stale at pub[5], newer than clone 4: waits
            (pub[5], (pub[4], z, var, A.VEL)),                    # VEL only
            (pub[6], (pub[0] - 0.3, z, var, A.POS))]              # older than the window
    Dl.run_outage_late(orc, seq, len(seq.frames), late)
    log = [(f, r, a, s, round(l, 6), st) for f, r, a, _, s, l, st in orc.aid_delayed_log]
    frames = sorted(set(f for f, *_ in log))
    assert len(log) == 3 and len(frames) == 2 and frames[1] == frames[0] + 1
    assert [e[1:] for e in log] == [(Dl.POS, True, 3, 0.0, Dl.APPLIED), (Dl.POS, True, 3, 0.5, Dl.APPLIED),
                                    (Dl.POS, True, 4, 0.4, Dl.APPLIED)]
    assert sorted(r for _, _, r in orc.aid_dropped) == ["no delayed rows", "older than the window"]
    assert orc.aid_log == [] and orc.aid_buffer == []


# ------------------------------------------------------------ the outage --

LATENCY = 0.2


@pytest.fixture(scope="module")
def late_runs():
    seq, Al, out = outage_runs(STREAM, FIRST_BLIND, {"POS": A.POS})
    plain = out["plain"][1]
    t0 = 100.0 + STREAM["static_s"]
    late = Dl.late_messages(plain[:, 0], t0, Al, A.POS, LATENCY)
    res = {"plain": out["plain"], "c": out["POS"]}
    for name, cfg, cls in (("a", stream_config(), Dl.OracleAidDelayed),
                           ("b", AidingConfig(lever=A.LEVER, dir_w=tuple(A.DIR_W), max_age=A.MAX_AGE, delayed=True),
                            Dl.OracleAidDelayed),
                           ("d", AidingConfig(lever=A.LEVER, dir_w=tuple(A.DIR_W), max_age=0.25), A.OracleAid)):
        orc = cls(FilterConfig(), chi2_threshold, cfg)
        rec = Dl.run_outage_late(orc, seq, FIRST_BLIND, late)
        res[name] = (orc, rec, A.position_errors(rec, seq, Al))
    return late, res


def test_late_fixes_on_the_outage_stream(late_runs):
    """test_aid_ref's outage stream (4.7 s without vision under the
    accelerometer bias), POS fixes by fix_messages' recipe (26, stamped 12 ms
    before every 4th published frame) handed to the filter 0.2 s after their
    stamp.  The 26th arrives after the last frame and is never delivered, in any
    run; the first is stamped 12 ms BEFORE the first clone, so no clone pair
    brackets it and (b) drops it as older than the window -- the other 24 go to
    the delayed path and all are applied (largest gamma 7.47 against 7.81).
    Measured with the oracle, position error against the truth:

        run                                      end error  max error  fixes applied
        plain (no fixes)                         0.3106 m   0.3106 m   -
        (a) delayed off                          0.3106 m   0.3106 m   0, 25 dropped as stale
        (b) delayed on                           0.0250 m   0.0850 m   24 of 24 (1 dropped)
        (c) zero latency, existing path          0.0304 m   0.0658 m   24 of 26
        (d) existing path, max_age 0.25 (-dt v)  0.0254 m   0.0880 m   24 of 25

    (b) ends at 0.82 x (c): the same information 0.2 s later costs nothing at the
    end of this stream, and the larger maximum is the 0.2 s of extra dead
    reckoning before each correction.  (d) ends level with (b) (0.0254 against
    0.0250 m) with a slightly larger maximum, although the trajectory's
    acceleration peaks at 3.0 m/s^2; one of its fixes is rejected at gamma 21.7
    where (b) applies all, and its largest accepted gamma is 7.04.  Why the end
    errors coincide was not examined further."""
    late, res = late_runs
    plain = res["plain"]
    for name in ("plain", "a", "b", "c", "d"):
        orc, rec, err = res[name]
        log = getattr(orc, "aid_log", [])
        dlog = getattr(orc, "aid_delayed_log", [])
        print("%-5s end %.4f max %.4f  aid %d of %d  delayed %d of %d  dropped %d  largest gamma %.2f (applied %.2f)" % (
            name, err[-1], err[FIRST_BLIND - 20:].max(), sum(e[2] for e in log), len(log), sum(e[2] for e in dlog),
            len(dlog), len(getattr(orc, "aid_dropped", [])), max([e[3] for e in log + dlog] or [np.nan]),
            max([e[3] for e in log + dlog if e[2]] or [np.nan])))
    t_end, t_first = plain[1][-1, 0], plain[1][0, 0]
    delivered = [m for arrival, m in late if arrival <= t_end]
    assert len(late) == 26 and len(delivered) == 25 and [m[0] < t_first for m in delivered] == [True] + [False] * 24
    # (a): the plain run exactly, every fix dropped
    orc, rec, err = res["a"]
    np.testing.assert_array_equal(rec, plain[1])
    assert orc.aid_log == [] and orc.aid_delayed_log == [] and len(orc.aid_dropped) == 25
    assert all(r == "stale" for _, _, r in orc.aid_dropped)
    # (b): every fix a clone pair can bracket is routed to the delayed path and applied
    orc, rec, err_b = res["b"]
    assert orc.aid_log == [] and len(orc.aid_delayed_log) == 24
    assert [(t, r) for _, t, r in orc.aid_dropped] == [(delivered[0][0], "older than the window")]
    assert all(a and st == Dl.APPLIED and r == Dl.POS for _, r, a, _, _, _, st in orc.aid_delayed_log)
    assert all(0.0 < lam < 1.0 for *_, lam, _ in orc.aid_delayed_log)
    err_c = res["c"][2]
    assert err_b[-1] < err[-1]
    assert err_b[-1] <= 2 * err_c[-1]
