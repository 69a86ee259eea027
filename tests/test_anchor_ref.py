"""The numpy restatement of include/msckf_anchor.h (tests/anchor_ref.py) checked
on the CPU against the oracle's own functions: the Jacobians by finite
differences through apply_correction, the compressed update against
measurement_update fed the whitened uncompressed rows, the statuses, and the
behaviour on a stream that loses vision.
"""
import numpy as np
import pytest

from oracle import msckf_oracle as O
from msckf_amd import CHI2_95, AnchorConfig, AnchorFix, FilterConfig, chi2_threshold, synth
import aid_ref
import anchor_ref as A
from test_aid_ref import rot
from test_zupt_ref import make_state


def params(**kw):
    return AnchorConfig(**{**dict(chi2=1e30), **kw})


def anchors_for(st, K, seed, depth=(2.0, 8.0), noise=0.002, sigma=0.01):
    """K anchors ``depth`` metres in front of the state's own cam0, inside the
    field of view (|u| < 0.5, |v| < 0.35), z = zhat + noise * normal, and a
    full covariance (sigma .. 2 sigma)^2 per axis, rotated."""
    rng = np.random.default_rng(seed)
    _, R0, t0, _, _ = A.geometry(st)
    d = depth[0] + (depth[1] - depth[0]) * rng.random(K)
    uv = (rng.random((K, 2)) - 0.5) * [1.0, 0.7]
    p = t0 + (np.column_stack([uv * d[:, None], d])) @ R0
    z = np.array([A.anchor_predict(st, q)[0] for q in p]).reshape(K, 4) + noise * rng.standard_normal((K, 4))
    cov = np.empty((K, 3, 3))
    for l in range(K):
        Q = rot(rng.standard_normal(3), rng.random() * np.pi)
        cov[l] = Q @ np.diag((sigma * (1 + rng.random(3))) ** 2) @ Q.T
        cov[l] = (cov[l] + cov[l].T) / 2
    return p, cov, z


def test_jacobians_by_finite_differences():
    """zhat(x [+] dx) = zhat(x) + H_l dx to first order, the correction being
    the oracle's apply_correction: central differences, step 1e-6, atol 1e-7
    (truncation ~1e-12, rounding ~1e-16 / 1e-6); the columns outside C are
    exactly 0; Hf against central differences in p_w."""
    st = make_state()
    p, cov, z = anchors_for(st, 3, 1)
    D = st.P.shape[0]
    h = 1e-6
    for l in range(3):
        H, r, N, Hf = A.anchor_rows(st, p[l], cov[l], z[l], 1e-3)
        assert H.shape == (4, D) and r.shape == (4,) and N.shape == (4, 4) and Hf.shape == (4, 3)
        J = np.zeros_like(H)
        for c in range(D):
            dx = np.zeros(D)
            dx[c] = h
            sp, sm = st.copy(), st.copy()
            O.apply_correction(sp, dx)
            O.apply_correction(sm, -dx)
            J[:, c] = (A.anchor_predict(sp, p[l])[0] - A.anchor_predict(sm, p[l])[0]) / (2 * h)
        print("anchor %d: max |H| %.3f  max |H - J| %.2e" % (l, np.abs(H).max(), np.abs(H - J).max()))
        np.testing.assert_allclose(H, J, atol=1e-7)
        outside = [c for c in range(D) if c not in A.COLS]
        assert np.abs(H[:, outside]).max() == 0.0 and np.abs(H[:, A.COLS]).min() > 0.0
        Jf = np.zeros((4, 3))
        for c in range(3):
            e = np.zeros(3)
            e[c] = h
            Jf[:, c] = (A.anchor_predict(st, p[l] + e)[0] - A.anchor_predict(st, p[l] - e)[0]) / (2 * h)
        np.testing.assert_allclose(Hf, Jf, atol=1e-7)
        np.testing.assert_allclose(N, 1e-3 * np.eye(4) + Hf @ cov[l] @ Hf.T, atol=0, rtol=1e-15)


@pytest.mark.parametrize("alias", [True, False])
@pytest.mark.parametrize("K", [1, 3, 4, 8, 64])
def test_compressed_update_is_measurement_update_of_whitened_rows(K, alias):
    """The oracle's own update is the yardstick: the whitened rows have noise I,
    so measurement_update with sigma2 = 1 fed all 4 K of them (it compresses by
    its own QR of the full-width block when 4 K > D) must give the state and the
    covariance of the update compressed in the twelve columns C.  K = 3 is the
    last case without QR, 4 the first with it.  P to 1e-12 relative (norm), the
    state to rtol 1e-12 (atol 1e-13 for its entries near 0, test_aid_ref's)."""
    prm = params()
    st = make_state(alias=alias)
    anchors = anchors_for(st, K, 10 + K)
    ref = st.copy()
    status, gamma, rows = A.anchor_gate(ref, prm, anchors)
    assert (status == A.USED).all() and np.isfinite(gamma).all() and len(rows) == K
    ref.sigma2 = 1.0
    O.measurement_update(ref, np.vstack([h for h, _ in rows]), np.concatenate([r for _, r in rows]))
    unc = st.copy()
    v_null0 = st.imu.v_null.copy()
    app, used, m, _, _ = A.anchor_update(st, prm, anchors, compressed=True)
    assert app and used == K and m == min(4 * K, 12)
    assert A.anchor_update(unc, prm, anchors)[:3] == (True, K, m)
    for got in (st, unc):
        assert np.linalg.norm(got.P - ref.P) <= 1e-12 * np.linalg.norm(ref.P)
        np.testing.assert_array_equal(got.P, got.P.T)
        for f in ("q", "p", "v", "bg", "ba", "R_imu_cam0", "t_cam0_imu", "v_null", "p_null"):
            np.testing.assert_allclose(getattr(got.imu, f), getattr(ref.imu, f), rtol=1e-12, atol=1e-13, err_msg=f)
        for c, cr in zip(got.cams.values(), ref.cams.values()):
            np.testing.assert_allclose(c.q, cr.q, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(c.p, cr.p, rtol=1e-12, atol=1e-13)
    if alias:   # quirk Q5
        np.testing.assert_array_equal(st.imu.v_null, st.imu.v)
    else:
        np.testing.assert_array_equal(st.imu.v_null, v_null0)


def same(a, b):
    return all(np.array_equal(getattr(a.imu, f), getattr(b.imu, f)) for f in
               ("q", "p", "v", "bg", "ba", "R_imu_cam0", "t_cam0_imu", "v_null", "p_null")) \
        and np.array_equal(a.P, b.P) and all(np.array_equal(c.q, d.q) and np.array_equal(c.p, d.p)
                                             for c, d in zip(a.cams.values(), b.cams.values()))


def test_statuses():
    st = make_state()
    before = st.copy()
    prm = params(chi2=None)
    p, cov, z = anchors_for(st, 5, 3)
    _, R0, t0, _, _ = A.geometry(st)
    p[1] = t0 - 3.0 * R0[2]              # behind the camera
    p[3] = p[3] + 3.0 * R0[0]            # displaced by 3 m across the viewing direction (gamma 19 against 9.49)
    cov[4] = np.diag([1e-4, 1e-4, -1.0])  # an indefinite covariance: N_l is not positive definite
    app, used, m, status, gamma = A.anchor_update(st, prm, (p, cov, z))
    assert status.tolist() == [A.USED, A.DEPTH, A.USED, A.GATED, A.NOT_PD]
    assert app and used == 2 and m == 8 and not same(st, before)
    assert np.isnan(gamma[[1, 4]]).all() and gamma[3] > prm.gate() > gamma[[0, 2]].max()
    # fewer used anchors than min_anchors, or a chi2 of 0: every bit stays
    for kw, want in ((dict(chi2=None, min_anchors=3), 2), (dict(chi2=0.0), 0), (dict(chi2=-1.0), 0)):
        st = before.copy()
        app, used, m, status, gamma = A.anchor_update(st, params(**kw), (p, cov, z))
        assert not app and used == want and m == 4 * want and same(st, before), kw
    st = before.copy()
    st.P[12, 12] = -10.0   # S_l not positive definite
    app, used, m, status, gamma = A.anchor_update(st, prm, (p, cov, z))
    assert not app and used == 0 and m == 0 and status.tolist() == [3, 2, 3, 3, 3] and np.isnan(gamma).all()
    assert A.anchor_update(st, prm, (p[:0], cov[:0], z[:0]))[:3] == (False, 0, 0)


def test_abi_symbols_and_structs():
    """include/msckf_anchor.h's entry points are exported by the library and
    typed one to one by the binding, in a list of their own."""
    import ctypes
    import os
    import re
    from msckf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "msckf_anchor.h")).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(msckf_anchor_[a-z]+)\s*\(", src)))
    assert syms == sorted(_lib.ANCHOR_EXPORTED) == ["msckf_anchor_batch", "msckf_anchor_results",
                                                    "msckf_anchor_status"]
    assert not set(syms) & (set(_lib.EXPORTED) | set(_lib.ZUPT_EXPORTED) | set(_lib.AID_EXPORTED))
    lib = _lib.load_library()
    for s in syms:
        assert getattr(lib, s).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.MsckfAnchorT) == 13 * 8 == _lib.ANCHOR_DTYPE.itemsize     # 3 + 6 + 4 doubles
    assert ctypes.sizeof(_lib.MsckfAnchorParamsT) == 32                                 # 3 doubles, an int32, padded
    assert _lib.MsckfAnchorT.cov.offset == 24 and _lib.MsckfAnchorT.z.offset == 72
    assert _lib.MsckfAnchorParamsT.min_anchors.offset == 24
    assert int(re.search(r"#define MSCKF_ANCHOR_MAX\s+(\d+)", src).group(1)) == _lib.ANCHOR_MAX == A.MAX == 64
    for name, val in re.findall(r"#define MSCKF_ANCHOR_(USED|GATED|DEPTH|NOT_PD)\s+(\d+)", src):
        assert getattr(_lib, "ANCHOR_" + name) == int(val) == getattr(A, name)
    a = _lib.pack_anchors([[1, 2, 3]], [np.arange(9.).reshape(3, 3)], [[4, 5, 6, 7]])
    assert a.tobytes() == np.array([1, 2, 3, 0, 1, 2, 4, 5, 8, 4, 5, 6, 7], float).tobytes()


def test_config_checks():
    c = AnchorConfig()
    assert c.gate() == CHI2_95[3] and c.min_depth == 0.1 and c.min_anchors == 1 and c.time_tol == 1e-6
    assert c.obs_var is None and AnchorConfig(chi2=5.0).gate() == 5.0
    prm = c.params(FilterConfig().observation_noise)
    assert (prm.obs_var, prm.chi2, prm.min_depth, prm.min_anchors) == (0.035 ** 2, CHI2_95[3], 0.1, 1)
    assert AnchorConfig(obs_var=1e-4).params().obs_var == 1e-4
    with pytest.raises(ValueError):
        c.params()
    for bad in (dict(obs_var=0.0), dict(obs_var=float("nan")), dict(chi2=float("nan")), dict(min_depth=0.0),
                dict(min_anchors=0), dict(min_anchors=1.5), dict(time_tol=-1.0),
                dict(world_from_ext=(np.ones((3, 3)), np.zeros(3))), dict(world_from_ext=(np.eye(3), np.zeros(2)))):
        with pytest.raises(ValueError):
            AnchorConfig(**bad).params(1e-3)
    # world_from_ext moves the points and rotates their covariances; the three forms of cov
    Rz = rot([0, 0, 1], np.pi / 2)
    c = AnchorConfig(world_from_ext=(Rz, np.array([1.0, 2.0, 3.0])))
    p, cov, z = c.in_world(AnchorFix(1.0, [[1, 0, 0], [0, 1, 0]], np.zeros((2, 4)),
                                     [np.diag([1.0, 2.0, 3.0]), np.diag([4.0, 5.0, 6.0])]))
    np.testing.assert_allclose(p, [[1, 3, 3], [0, 2, 3]], atol=1e-15)
    np.testing.assert_allclose(cov, [np.diag([2.0, 1.0, 3.0]), np.diag([5.0, 4.0, 6.0])], atol=1e-15)
    assert z.shape == (2, 4)
    np.testing.assert_array_equal(AnchorFix(0.0, np.zeros((2, 3)), np.zeros((2, 4)), 4.0).arrays()[2],
                                  [4 * np.eye(3)] * 2)
    np.testing.assert_array_equal(AnchorFix(0.0, np.zeros((2, 3)), np.zeros((2, 4)), [1.0, 2.0]).arrays()[2],
                                  [np.eye(3), 2 * np.eye(3)])
    for bad in (dict(z=np.zeros((3, 4))), dict(cov=np.zeros(3)), dict(cov=np.zeros((2, 2, 2)))):
        with pytest.raises(ValueError):
            AnchorFix(**{**dict(timestamp=0.0, p=np.zeros((2, 3)), z=np.zeros((2, 4))), **bad}).arrays()


def test_option_off_is_the_oracle():
    """OracleAnchor without a config is OracleMSCKF to the bit."""
    from zupt_ref import run_oracle
    seq = synth.make_sequence(n_frames=4, static_s=1.2, seed=1)
    a = run_oracle(A.OracleAnchor(FilterConfig(), chi2_threshold, None), seq)
    b = run_oracle(O.OracleMSCKF(FilterConfig(), chi2_threshold), seq)
    np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------ the outage --

STREAM = dict(n_frames=100, static_s=1.2, seed=0)   # test_aid_ref.py's stream
FIRST_BLIND = 30
T0 = 100.0 + STREAM["static_s"]


@pytest.fixture(scope="module")
def runs():
    """(seq, alignment, plain (oracle, records, errors), anchored (oracle, records, errors), declared anchors)."""
    seq = synth.make_sequence(**STREAM)
    orc = O.OracleMSCKF(FilterConfig(), chi2_threshold)
    plain = aid_ref.run_outage(orc, seq, FIRST_BLIND)
    Al = aid_ref.alignment(plain[0], seq)
    msgs, declared, L = A.anchor_messages(plain[:, 0], T0, Al, FilterConfig())
    anc = A.OracleAnchor(FilterConfig(), chi2_threshold, AnchorConfig())
    rec = A.run_outage(anc, seq, FIRST_BLIND, msgs)
    return (seq, Al, (orc, plain, aid_ref.position_errors(plain, seq, Al)),
            (anc, rec, aid_ref.position_errors(rec, seq, Al)), (declared, L), msgs)


def test_outage_stream(runs):
    """synth.make_sequence(n_frames=100, static_s=1.2, seed=0) with a constant
    accelerometer bias of [0.08, -0.06, 0.05] m/s^2 and every feature message
    from frame index 30 on emptied (4.7 s without vision); 104 frames are
    published.  Eight anchors from default_rng(200), surveyed to 5 mm and
    declared so, a message at every 4th published frame (26) with the visible
    ones, pixel noise 0.5 / 458.654; obs_var is the filter's observation_noise
    (about 30 times that pixel noise, hence the small gammas).  Measured with
    the oracle:

        run       end error  max error (from frame 10)  applied   anchors used  largest gamma  gate
        plain     0.3106 m   0.3106 m                   -         -             -              -
        anchors   0.0172 m   0.0278 m                   26 of 26  190 of 190    0.04           9.49

    (7 to 8 of the eight anchors are visible per message.)
    """
    seq, Al, (_, plain, perr), (anc, rec, err), _, msgs = runs
    log = anc.anchor_log
    n_all, n_used = sum(n for _, n, _, _ in log), sum(u for _, _, u, _ in log)
    gmax = max(np.nanmax(g) for _, g in anc.anchor_records)
    print("plain   end %.4f max %.4f" % (perr[-1], perr[10:].max()))
    print("anchors end %.4f max %.4f applied %d of %d used %d of %d (%d..%d per frame) largest gamma %.2f gate %.2f"
          % (err[-1], err[10:].max(), sum(a for *_, a in log), len(log), n_used, n_all,
             min(n for _, n, _, _ in log), max(n for _, n, _, _ in log), gmax, CHI2_95[3]))
    assert len(rec) == len(plain) == 104 and len(log) == len(msgs) == 26 and anc.anchor_dropped == 0
    assert [f for f, *_ in log] == list(range(0, 104, 4))
    assert err[-1] <= perr[-1] / 5
    assert n_used >= 0.8 * n_all and sum(a for *_, a in log) >= 0.8 * len(log)


def test_displaced_anchor_is_gated(runs):
    """At the end of the anchored run: one visible anchor displaced by 1 m along
    the filter world's z (then y) goes GATED with gamma > 4 x the gate, the
    others are used.  (Along x, the viewing direction, 1 m moves the
    projections too little to be caught.)"""
    seq, Al, _, (anc, rec, _), (declared, L), msgs = runs
    vis, uv = A.visible(L, rec[-1, 0], T0, FilterConfig())   # the noise-free view from the last published frame
    p, z = declared[vis], uv[vis]
    cov = np.broadcast_to(A.SURVEY_SIGMA ** 2 * np.eye(3), (len(p), 3, 3))
    prm = AnchorConfig()
    assert len(p) >= 2
    for axis in (2, 1):
        st = anc.st.copy()
        q = p.copy()
        q[0, axis] += 1.0
        app, used, m, status, gamma = A.anchor_update(st, prm, (q, cov, z))
        print("axis %d: gamma %.1f (gate %.2f), others at most %.3f" % (axis, gamma[0], prm.gate(), gamma[1:].max()))
        assert status.tolist() == [A.GATED] + [A.USED] * (len(p) - 1)
        assert gamma[0] > 4 * prm.gate() and app and used == len(p) - 1
