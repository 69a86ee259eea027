"""The numpy restatement of include/msckf_aid.h (tests/aid_ref.py) checked on the
CPU against the oracle's own functions: the Jacobian by finite differences
through apply_correction, the update against measurement_update fed the whitened
rows, and the behaviour on a stream that loses vision.
"""
import numpy as np
import pytest

from oracle import msckf_oracle as O
from msckf_amd import CHI2_95, AidingConfig, AidingFix, FilterConfig, chi2_threshold, synth
import aid_ref as A
from test_zupt_ref import make_state

# masks: each group alone, single axes (POS z: a barometer; BVEL y + z: a non-holonomic constraint), m = 1 .. 12
MASKS = [A.POS, A.VEL, A.BVEL, A.DIR, 0x004, 0x180, A.POS | A.VEL, 0x001, 0xfff]


def rot(axis, ang):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = O.skew(axis)
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def params(**kw):
    d = np.array([0.6, -0.64, 0.48])
    return AidingConfig(**{**dict(lever=(0.10, -0.05, 0.20), R_body=rot([1, 2, -1], 0.7), dir_w=tuple(d), chi2=1e30),
                           **kw})


def fix_for(st, prm, rows, seed, dt=0.03, off=0.05):
    """A fix near the state's own prediction: z = h(x) + off * normal, var (0.02 .. 0.04)^2."""
    rng = np.random.default_rng(seed)
    z = A.aid_predict(st, prm, dt) + off * rng.standard_normal(12)
    return z, (0.02 + 0.02 * rng.random(12)) ** 2, dt, rows


@pytest.mark.parametrize("rows", [A.POS, A.VEL, A.BVEL, A.DIR, 0xfff])
def test_jacobian_by_finite_differences(rows):
    """h(x [+] dx) = h(x) + H dx to first order, the correction being the
    oracle's apply_correction: central differences of the prediction, step 1e-6
    (h is at most cubic in dx over that step: truncation ~1e-12, rounding
    ~1e-16 / 1e-6 ~ 1e-10), with a non-zero lever arm and age and a
    non-identity R_body."""
    prm = params()
    st = make_state()
    fix = fix_for(st, prm, rows, 1)
    H, r, nz = A.aid_rows(st, prm, fix)
    D = st.P.shape[0]
    k = A.kept(rows)
    assert H.shape == (len(k), D) and r.shape == nz.shape == (len(k),)
    h = 1e-6
    J = np.zeros_like(H)
    for c in range(D):
        dx = np.zeros(D)
        dx[c] = h
        sp, sm = st.copy(), st.copy()
        O.apply_correction(sp, dx)
        O.apply_correction(sm, -dx)
        J[:, c] = (A.aid_predict(sp, prm, fix[2])[k] - A.aid_predict(sm, prm, fix[2])[k]) / (2 * h)
    np.testing.assert_allclose(H, J, atol=1e-7)
    for sl in (slice(3, 6), slice(9, 12), slice(15, None)):
        assert np.abs(H[:, sl]).max() == 0.0


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("rows", MASKS)
def test_update_is_measurement_update_of_whitened_rows(rows, alias):
    """The oracle's own update is the yardstick: with W = sigma R^-1/2 the rows
    W H, W r have noise sigma^2 I, and measurement_update (m <= 12 <= D: no QR)
    must give the same state and covariance."""
    prm = params()
    st = make_state(alias=alias)
    fix = fix_for(st, prm, rows, 2 + rows)
    ref = st.copy()
    H, r, nz = A.aid_rows(ref, prm, fix)
    Wh = np.sqrt(ref.sigma2 / nz)
    assert H.shape[0] == bin(rows).count("1") <= H.shape[1]
    O.measurement_update(ref, Wh[:, None] * H, Wh * r)
    v_null0 = st.imu.v_null.copy()
    app, gam = A.aid_update(st, prm, fix)
    assert app and np.isfinite(gam)
    assert np.linalg.norm(st.P - ref.P) <= 1e-12 * np.linalg.norm(ref.P)
    np.testing.assert_array_equal(st.P, st.P.T)
    for f in ("q", "p", "v", "bg", "ba", "R_imu_cam0", "t_cam0_imu", "v_null", "p_null"):
        np.testing.assert_allclose(getattr(st.imu, f), getattr(ref.imu, f), atol=1e-13, err_msg=f)
    for c, cr in zip(st.cams.values(), ref.cams.values()):
        np.testing.assert_allclose(c.q, cr.q, atol=1e-13)
        np.testing.assert_allclose(c.p, cr.p, atol=1e-13)
    if alias:   # quirk Q5
        np.testing.assert_array_equal(st.imu.v_null, st.imu.v)
    else:
        np.testing.assert_array_equal(st.imu.v_null, v_null0)


def test_masked_rows_are_ignored():
    prm = params()
    st, st2 = make_state(), make_state()
    z, var, dt, _ = fix_for(st, prm, 0xfff, 5)
    z2, var2 = z.copy(), var.copy()
    z2[3:] = np.nan
    var2[3:] = -1.0
    assert A.aid_update(st, prm, (z, var, dt, A.POS)) == A.aid_update(st2, prm, (z2, var2, dt, A.POS))
    np.testing.assert_array_equal(st.P, st2.P)


def test_gate_rejection_and_indefinite_S_leave_the_state_alone():
    st = make_state()
    before = st.copy()
    prm = params(chi2=0.0)
    fix = fix_for(st, prm, 0xfff, 3)
    app, gam = A.aid_update(st, prm, fix)
    assert not app and np.isfinite(gam) and gam > 0
    np.testing.assert_array_equal(st.P, before.P)
    np.testing.assert_array_equal(st.imu.p, before.imu.p)
    st.P[12, 12] = -10.0   # S not positive definite
    app, gam = A.aid_update(st, params(), fix)
    assert not app and np.isnan(gam)
    np.testing.assert_array_equal(st.imu.p, before.imu.p)
    np.testing.assert_array_equal(st.imu.q, before.imu.q)


def test_abi_symbols_and_structs():
    """include/msckf_aid.h's entry points are exported by the library and typed
    one to one by the binding, in a list of their own."""
    import ctypes
    import os
    import re
    from msckf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "msckf_aid.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(msckf_aid_[a-z]+)\s*\(", src)))
    assert syms == sorted(_lib.AID_EXPORTED) == ["msckf_aid_batch", "msckf_aid_results"]
    assert not set(syms) & set(_lib.EXPORTED) and not set(syms) & set(_lib.ZUPT_EXPORTED)
    lib = _lib.load_library()
    for s in syms:
        assert getattr(lib, s).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.MsckfAidParamsT) == 27 * 8          # 3 + 9 + 3 + 12 doubles
    assert ctypes.sizeof(_lib.MsckfAidFixT) == 26 * 8             # 12 + 12 + 1 doubles, an int32, padded to 8
    assert _lib.MsckfAidFixT.dt.offset == 192 and _lib.MsckfAidFixT.rows.offset == 200
    for name, val in re.findall(r"#define MSCKF_AID_([A-Z]+)\s+(0x[0-9a-f]+)", src):
        assert getattr(_lib, "AID_" + name) == int(val, 16) == getattr(A, name)
    assert (_lib.AID_POS, _lib.AID_VEL, _lib.AID_BVEL, _lib.AID_DIR) == (0x007, 0x038, 0x1c0, 0xe00)


def test_config_checks():
    assert len(CHI2_95) == 12
    np.testing.assert_allclose(CHI2_95[:3], [3.841459, 5.991465, 7.814728], atol=5e-7)
    np.testing.assert_allclose(CHI2_95[-1], 21.026070, atol=5e-7)
    assert all(CHI2_95[m - 1] > chi2_threshold(m) for m in range(1, 13))   # the upper tail, not the lower
    c = AidingConfig()
    assert c.gates() == tuple(CHI2_95) and c.max_age == 0.05 and tuple(c.lever) == (0, 0, 0)
    assert AidingConfig(chi2=5.0).gates() == (5.0,) * 12
    c.params()
    for bad in (dict(R_body=2 * np.eye(3)), dict(dir_w=(1.0, 1.0, 0.0)), dict(max_age=-1.0),
                dict(chi2=float("nan")), dict(world_from_ext=(np.ones((3, 3)), np.zeros(3))),
                dict(lever=(0.0, float("nan"), 0.0))):
        with pytest.raises(ValueError):
            AidingConfig(**bad).params()
    # world_from_ext moves positions and rotates velocities; axes select rows; the newest message wins per group
    Rz = rot([0, 0, 1], np.pi / 2)
    c = AidingConfig(world_from_ext=(Rz, np.array([1.0, 2.0, 3.0])), max_age=0.1)
    z, var, mask = c.rows_of(AidingFix(1.0, position=[1, 0, 0], velocity=[0, 1, 0], position_axes=(0, 0, 1),
                                       velocity_var=(1e-2, 2e-2, 3e-2)))
    np.testing.assert_allclose(z[:6], [1, 3, 3, -1, 0, 0], atol=1e-15)
    assert mask == 0x004 | 0x038 and var[3:6].tolist() == [1e-2, 2e-2, 3e-2]
    old = AidingFix(0.95, position=[0, 0, 0], direction=[1, 0, 0])
    new = AidingFix(0.98, position=[1, 0, 0])
    stale = AidingFix(0.85, body_velocity=[1, 0, 0])
    late = AidingFix(1.01, velocity=[1, 0, 0])
    z, var, dt, mask = c.merge([old, stale, new, late], 1.0)
    assert mask == A.POS | A.DIR and abs(dt - 0.02) < 1e-12
    np.testing.assert_allclose(z[:3], [1, 3, 3], atol=1e-15)
    assert c.merge([stale, late], 1.0) is None


def test_option_off_is_the_oracle():
    """OracleAid without a config is OracleMSCKF to the bit."""
    from zupt_ref import run_oracle
    seq = synth.make_sequence(n_frames=4, static_s=1.2, seed=1)
    a = run_oracle(A.OracleAid(FilterConfig(), chi2_threshold, None), seq)
    b = run_oracle(O.OracleMSCKF(FilterConfig(), chi2_threshold), seq)
    np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------ the outage --

STREAM = dict(n_frames=100, static_s=1.2, seed=0)
FIRST_BLIND = 30
CASES = {"POS": A.POS, "POS+VEL": A.POS | A.VEL, "BVEL": A.BVEL, "all": 0xfff}


def stream_config():
    return AidingConfig(lever=A.LEVER, dir_w=tuple(A.DIR_W), max_age=A.MAX_AGE)


def outage_runs(stream, first_blind, cases):
    """The plain oracle and OracleAid per case on the outage stream ->
    (seq, alignment, {name: (oracle, records, errors)})."""
    seq = synth.make_sequence(**stream)
    orc = O.OracleMSCKF(FilterConfig(), chi2_threshold)
    plain = A.run_outage(orc, seq, first_blind)
    Al = A.alignment(plain[0], seq)
    out = {"plain": (orc, plain, A.position_errors(plain, seq, Al))}
    t0 = 100.0 + stream["static_s"]
    for name, rows in cases.items():
        orc = A.OracleAid(FilterConfig(), chi2_threshold, stream_config())
        rec = A.run_outage(orc, seq, first_blind, A.fix_messages(plain[:, 0], t0, Al, rows))
        out[name] = (orc, rec, A.position_errors(rec, seq, Al))
    return seq, Al, out


@pytest.fixture(scope="module")
def runs():
    return outage_runs(STREAM, FIRST_BLIND, CASES)


def test_outage_stream(runs):
    """synth.make_sequence(n_frames=100, static_s=1.2, seed=0) with a constant
    accelerometer bias of [0.08, -0.06, 0.05] m/s^2 and every feature message
    from frame index 30 on emptied (4.7 s without vision); 104 frames are
    published, a fix 12 ms before every 4th of them (26), noise
    default_rng(100).  Measured with the oracle; the plain oracle ends 0.3106 m
    from the truth:

        rows      end error  max error  applied   largest gamma  gate
        POS       0.0304 m   0.0658 m   24 of 26   8.66           7.81
        POS+VEL   0.0163 m   0.0168 m   26 of 26  11.30          12.59
        BVEL      0.0495 m   0.0602 m   26 of 26   6.65           7.81
        all four  0.0082 m   0.0151 m   26 of 26  19.98          21.03

    (POS alone loses two fixes to the 95 % gate, as one in twenty should be.)"""
    seq, Al, out = runs
    plain = out["plain"][2]
    for name in CASES:
        orc, rec, err = out[name]
        log = orc.aid_log
        gate = CHI2_95[bin(CASES[name]).count("1") - 1]
        print("%-8s end %.4f max %.4f applied %d of %d largest gamma %.2f gate %.2f (plain end %.4f)"
              % (name, err[-1], err[FIRST_BLIND - 20:].max(), sum(a for _, _, a, _ in log), len(log),
                 max(g for _, _, _, g in log), gate, plain[-1]))
        assert len(rec) == len(out["plain"][1]) == 104 and len(log) == 26
        assert [r for _, r, _, _ in log] == [CASES[name]] * len(log)
        assert sum(a for _, _, a, _ in log) >= 0.8 * len(log)
    assert out["POS+VEL"][2][-1] <= plain[-1] / 5
    assert out["BVEL"][2][-1] <= plain[-1] / 3


def test_displaced_fix_is_rejected(runs):
    """A position fix 1 m off the truth at the end of the POS+VEL run: gamma is
    far beyond the gate and the state keeps every bit."""
    seq, Al, out = runs
    orc = out["POS+VEL"][0]
    st = orc.st.copy()
    t = out["POS+VEL"][1][-1, 0]
    z = A.truth_rows(t, 100.0 + STREAM["static_s"], Al) + np.r_[1.0, np.zeros(11)]
    prm = stream_config()
    app, gam = A.aid_update(st, prm, (z, A.SIG ** 2, 0.0, A.POS))
    assert not app and gam > 100 * CHI2_95[2]
    np.testing.assert_array_equal(st.P, orc.st.P)
    for f in ("q", "p", "v", "bg", "ba"):
        np.testing.assert_array_equal(getattr(st.imu, f), getattr(orc.st.imu, f))
