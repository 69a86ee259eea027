"""GPU parity tests: the HIP path (through the C-ABI) against the golden
fixtures generated from the reference and against the CPU oracle.

Tolerances (fp64 path): per-stage results to <= 1e-9 relative (the kernels
differ from LAPACK only in summation order and in the orthogonal basis used
for the nullspace / QR, to which the update is invariant -- quirk Q4); the
full 200-frame sequence to <= 1e-6 relative on the state vector and on the
covariance Frobenius norm (BASELINE.json north star) with every gating
decision identical.  fp32 path: per-update covariance <= 1e-4 relative.
"""
from collections import OrderedDict

import numpy as np
import pytest

from conftest import golden, rel
from helpers import oracle_state_from_arrays, problem_to_dict, feature_obs, oracle_update, rounded, sequence_config
from lifecycle import propagate_batch_vs_oracle
from oracle import msckf_oracle as O
import msckf_amd
from msckf_amd import synth, FilterConfig, CHI2_05, chi2_threshold
from msckf_amd._lib import Context, pack_imu, pack_cams, unpack_imu

pytestmark = pytest.mark.gpu


def imu_record(d, alias=True):
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"],
                    gravity=d["gravity"], alias=alias)


def make_ctx(ds, dtype=np.float64, cap=None):
    ds = ds if isinstance(ds, list) else [ds]
    N = max(int(d["N"]) for d in ds)
    ctx = Context(FilterConfig(), n_filters=len(ds), n_cam_capacity=cap or N + 2, dtype=dtype)
    for b, d in enumerate(ds):
        ctx.set_state(b, imu_record(d), pack_cams(d["cam_q"], d["cam_p"], d["cam_q_null"]), d["P"])
    return ctx


def chi2_for(M):
    return np.array([CHI2_05[m - 2] for m in M])


# ------------------------------------------------------------------ stages --

def test_state_roundtrip():
    d = golden("augment")
    ctx = make_ctx(d)
    imu, cams, P = ctx.get_state(0)
    np.testing.assert_array_equal(P, d["P"])
    np.testing.assert_array_equal(cams[:, 0:4], d["cam_q"])
    np.testing.assert_array_equal(imu[0:4], d["imu_q"])


def test_propagate_golden():
    g = golden("process_model")
    n = len(g["cam_q"])
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=n + 2)
    imu = pack_imu(q=g["init_q"], p=g["init_p"], v=g["init_v"], bg=g["init_bg"], ba=g["init_ba"],
                   q_null=g["init_q_null"], p_null=g["init_p"], v_null=g["init_v"],
                   R_imu_cam0=g["R_imu_cam0"], t_cam0_imu=g["t_cam0_imu"], gravity=g["gravity"], alias=True)
    ctx.set_state(0, imu, pack_cams(g["cam_q"], g["cam_p"], g["cam_q_null"]), g["init_P"])
    ts = np.concatenate([[g["t0"]], g["ts"]])
    # first 7 samples one by one, the rest in one batched launch
    for k in range(7):
        ctx.propagate(0, [ts[k + 1] - ts[k]], g["gyro"][k:k + 1], g["acc"][k:k + 1])
        s = unpack_imu(ctx.get_state(0, want_P=False)[0])
        np.testing.assert_allclose(s["q"], g["q"][k], atol=1e-13)
        np.testing.assert_allclose(s["v"], g["v"][k], atol=1e-12)
        np.testing.assert_allclose(s["p"], g["p"][k], atol=1e-12)
    ctx.propagate(0, np.diff(ts)[7:], g["gyro"][7:], g["acc"][7:])
    imu, _, P = ctx.get_state(0)
    s = unpack_imu(imu)
    np.testing.assert_allclose(s["q"], g["q"][-1], atol=1e-13)
    np.testing.assert_allclose(s["v"], g["v"][-1], atol=1e-12)
    np.testing.assert_allclose(s["p"], g["p"][-1], atol=1e-12)
    assert rel(P, g["P"]) < 1e-12
    np.testing.assert_array_equal(P, P.T)


@pytest.mark.parametrize("N,dtype", [(30, np.float64), (50, np.float64), (80, np.float64), (30, np.float32)])
def test_propagate_batch_vs_oracle(N, dtype):
    """IMU propagation (msckf.py:291-368, jit_utils.py:6-135) at the bench
    windows D = 201 / 321 / 501: two filters x ten samples in ONE batched
    launch (the bench's propagation leg), against the oracle's per-sample
    process_model.  fp64: P <= 1e-12, q / v / p <= 1e-12; fp32 (the context
    rounds state and P to fp32 and runs the recursion in fp32): P <= 1e-5,
    q / v / p <= 1e-5 relative."""
    B, n = 2, 10
    problems = [synth.make_update_problem(N, 4, seed=400 + b) for b in range(B)]
    ds = [problem_to_dict(p) for p in problems]
    if dtype == np.float32:
        ds = [rounded(d) for d in ds]
    ctx = make_ctx(ds, dtype=dtype, cap=N)
    propagate_batch_vs_oracle(ctx, ds, [n] * B, dtype, seed=N)


def test_augment_golden():
    d = golden("augment")
    ctx = make_ctx(d)
    ctx.augment(0)
    imu, cams, P = ctx.get_state(0)
    assert cams.shape[0] == int(d["N"]) + 1
    np.testing.assert_allclose(cams[-1, 0:4], d["new_q"], atol=1e-15)
    np.testing.assert_allclose(cams[-1, 4:7], d["new_p"], atol=1e-15)
    np.testing.assert_allclose(cams[-1, 7:11], d["new_q"], atol=1e-15)
    assert rel(P, d["P_out"]) < 1e-14
    np.testing.assert_array_equal(P, P.T)


def test_prune_golden():
    d = golden("prune")
    ctx = make_ctx(d)
    ctx.prune(0, [int(c) for c in d["rm"]])
    imu, cams, P = ctx.get_state(0)
    np.testing.assert_array_equal(P, d["P_out"])
    keep = [i for i in range(int(d["N"])) if i not in set(int(c) for c in d["rm"])]
    np.testing.assert_array_equal(cams[:, 0:4], d["cam_q"][keep])


@pytest.mark.parametrize("name", ["update_n10_f40", "update_n20_f100"])
def test_triangulate_golden(name):
    d = golden(name)
    ctx = make_ctx(d)
    p, ok = ctx.triangulate(0, d["obs_off"], d["obs_cam"], d["obs_z"])
    np.testing.assert_array_equal(ok, d["tri_ok"])
    np.testing.assert_allclose(p, d["tri_p"], rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("name", ["update_n10_f40", "update_n20_f100"])
def test_update_golden(name):
    d = golden(name)
    ctx = make_ctx(d)
    F = int(d["F"])
    sel = [f for f in range(F) if d["tri_ok"][f]]
    off = [0]
    cams, zs = [], []
    for f in sel:
        a, b = int(d["obs_off"][f]), int(d["obs_off"][f + 1])
        cams.extend(d["obs_cam"][a:b])
        zs.extend(d["obs_z"][a:b])
        off.append(len(cams))
    M = np.diff(off)
    acc, gam, rows = ctx.update(0, off, cams, zs, d["tri_p"][sel], chi2_for(M), row_cap=0)
    np.testing.assert_allclose(gam, d["gamma"][sel], rtol=1e-9)
    np.testing.assert_array_equal(acc, d["accept"][sel])
    assert rows == int(d["stacked_rows"])
    imu, cams_o, P = ctx.get_state(0)
    s = unpack_imu(imu)
    assert rel(P, d["P_out"]) < 1e-9
    np.testing.assert_array_equal(P, P.T)
    np.testing.assert_allclose(s["q"], d["imu_q_out"], atol=1e-11)
    np.testing.assert_allclose(s["p"], d["imu_p_out"], atol=1e-11)
    np.testing.assert_allclose(s["v"], d["imu_v_out"], atol=1e-11)
    np.testing.assert_allclose(s["bg"], d["imu_bg_out"], atol=1e-11)
    np.testing.assert_allclose(s["R_imu_cam0"], d["R_imu_cam0_out"], atol=1e-11)
    np.testing.assert_allclose(cams_o[:, 0:4], d["cam_q_out"], atol=1e-11)
    np.testing.assert_allclose(cams_o[:, 4:7], d["cam_p_out"], atol=1e-11)


def test_update_row_cap_vs_oracle():
    """msckf.py:676-679: stop after the first feature that pushes the stacked
    rows past the cap; later features are neither gated nor stacked."""
    d = golden("update_n20_f100")
    st, acc_o, _, _, _ = oracle_update(d, row_cap=300, triangulate=False)
    ctx = make_ctx(d)
    sel = [f for f in range(int(d["F"])) if d["tri_ok"][f]]
    obs = [feature_obs(d, f) for f in sel]
    off = np.concatenate([[0], np.cumsum([len(o) for o in obs])])
    cams = [c for o in obs for c, _ in o]
    zs = [z for o in obs for _, z in o]
    acc, gam, rows = ctx.update(0, off, cams, zs, d["tri_p"][sel], chi2_for(np.diff(off)), row_cap=300)
    assert 300 < rows < 300 + 4 * 20
    np.testing.assert_array_equal(acc, acc_o[sel])
    imu, _, P = ctx.get_state(0)
    assert rel(P, st.P) < 1e-9


def test_load_rejects_duplicate_cam_slots():
    """k_info keys a feature's records by cam slot: a feature observing one
    slot twice is refused at load time (msckf_batch_load returns < 0)."""
    d = golden("update_n10_f40")
    ctx = make_ctx(d)
    with pytest.raises(RuntimeError, match="twice"):
        ctx.update(0, [0, 3], [1, 2, 1], d["obs_z"][:3], d["tri_p"][:1], np.array([10.0]))


@pytest.mark.parametrize("corrupt", ["indefinite", "nan"])
def test_update_rejects_corrupted_covariance(corrupt):
    """Stage A floors only rounding-level pivots (down to -1e-6 x the largest
    cam variance, msckf_rchol.h pivot_floored): a P_cc set through set_state
    with a clearly negative eigenvalue, or a NaN, still fails the update with
    -3 instead of being silently regularised."""
    d = golden("update_n10_f40")
    P = d["P"].copy()
    if corrupt == "indefinite":
        v = np.zeros(P.shape[0])
        v[27:33] = 1.0 / np.sqrt(6.0)
        P -= 10.0 * np.abs(np.diag(P)[21:]).max() * np.outer(v, v)
    else:
        P[30, 30] = np.nan
    assert corrupt == "nan" or np.linalg.eigvalsh(P[21:, 21:]).min() < -1e-3 * np.abs(np.diag(P)[21:]).max()
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=int(d["N"]) + 2)
    try:
        ctx.set_state(0, imu_record(d), pack_cams(d["cam_q"], d["cam_p"], d["cam_q_null"]), P)
        sel = [f for f in range(int(d["F"])) if d["tri_ok"][f]]
        obs = [feature_obs(d, f) for f in sel]
        off = np.concatenate([[0], np.cumsum([len(o) for o in obs])])
        cams = [c for o in obs for c, _ in o]
        zs = [z for o in obs for _, z in o]
        with pytest.raises(RuntimeError, match="rc=-3"):
            ctx.update(0, off, cams, zs, d["tri_p"][sel], np.full(len(sel), 1e30))
    finally:
        ctx.close()


def test_update_empty_is_noop():
    d = golden("update_n10_f40")
    ctx = make_ctx(d)
    chi = np.zeros(3)          # everything rejected
    off = [0, 3, 6, 9]
    acc, gam, rows = ctx.update(0, off, [0, 1, 2] * 3, d["obs_z"][:9], d["tri_p"][:3], chi)
    assert rows == 0 and not acc.any()
    _, _, P = ctx.get_state(0)
    np.testing.assert_array_equal(P, d["P"])


def _debug_call(ctx, name, *args):
    import ctypes as C
    fn = getattr(ctx.lib, name)
    if name == "msckf_debug_set_workspace":
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.c_size_t]
    else:
        fn.argtypes = [C.c_void_p]
    fn.restype = C.c_int
    ctx._check(fn(ctx.h, *args))


@pytest.mark.parametrize("ncams,chol", [(10, "tiles"), (10, "mfma"), (34, "tiles")])
@pytest.mark.parametrize("depth,fails", [(1e-12, False), (1e-6, True)])
def test_stage_c_pivot_bound_every_path(ncams, chol, depth, fails, monkeypatch):
    """Stage C floors a pivot of T = s2 I + Lc^T A Lc at s2 only down to
    -1e-9 x max diag(T), and fails the update below that (rc -3, "innovation
    covariance"), on every path: register tiles (k_kal_c1), fp64 MFMA
    (k_kal_mchol) and the global-memory Cholesky of windows over 32 cams
    (k_gchol_diag<1>, 34 cams).  T is driven through the debug hooks: with
    P = diag(p), Lc = diag(sqrt(p_cc)), and A = Lc^-T (D - s2 I) Lc^-1 makes
    T = D to rounding; D = I but one entry -depth (-1e-12: rounding level,
    floored; -1e-6: a corrupted T)."""
    import ctypes as C
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", chol)
    pr = synth.make_update_problem(ncams, 40, seed=77)
    d = problem_to_dict(pr)
    Cn, D = 6 * ncams, 21 + 6 * ncams
    p = 1e-3 * (1.0 + np.random.default_rng(5).random(D))
    P = np.diag(p)
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=ncams, dtype=np.float64)
    try:
        imu, cams = imu_record(d), pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null)
        ctx.set_state(0, imu, cams, P)
        ctx.batch_load([0, pr.F], pr.obs_off, pr.obs_cam, pr.obs_z, None, np.full(pr.F, 1e30))
        ctx.batch_update(row_cap=0, triangulate=True)
        rows = ctx.batch_results()[4]
        assert rows[0] > 0
        s2 = FilterConfig().observation_noise
        dg = np.ones(Cn)
        dg[Cn // 2] = -depth
        H = np.zeros((Cn, Cn + 1))
        H[:, :Cn] = np.diag((dg - s2) / p[21:])
        H[:, Cn] = 1e-3
        ctx.set_state(0, imu, cams, P)   # the pre-update state again
        _debug_call(ctx, "msckf_debug_set_workspace", 6, H.ctypes.data_as(C.POINTER(C.c_double)), H.size)
        _debug_call(ctx, "msckf_debug_kalman")
        if fails:
            with pytest.raises(RuntimeError, match="innovation covariance not positive definite.*rc=-3"):
                ctx.batch_results()
        else:
            ctx.batch_results()
            _, _, P1 = ctx.get_state(0)
            assert np.isfinite(P1).all()
            # P+_cc = s2 Lc T^-1 Lc^T = s2 diag(p_cc / T_ii): the floored pivot (s2 in
            # place of -1e-12) leaves its variance unchanged, the others shrink by s2
            dd = np.diag(P1)[21:]
            k = Cn // 2
            assert abs(dd[k] - p[21 + k]) < 1e-9 * p[21 + k]
            other = np.arange(Cn) != k
            np.testing.assert_allclose(dd[other], s2 * p[21:][other], rtol=1e-9)
    finally:
        ctx.close()


# --------------------------------------------------- full-size batched mode --

def _batched(problems, dtype, triangulate=True, row_cap=0, cap=None):
    ds = [problem_to_dict(p) for p in problems]
    ctx = make_ctx(ds, dtype=dtype, cap=cap)
    feat_off = np.concatenate([[0], np.cumsum([p.F for p in problems])])
    obs_off, cams, zs, chi = [0], [], [], []
    for p in problems:
        base = obs_off[-1]
        obs_off.extend(list(base + p.obs_off[1:]))
        cams.extend(p.obs_cam)
        zs.extend(p.obs_z)
        chi.extend(chi2_for(p.track_lengths()))
    ctx.batch_load(feat_off, obs_off, cams, np.array(zs), None, np.array(chi))
    ctx.batch_update(row_cap=row_cap, triangulate=triangulate)
    acc, gam, pw, valid, rows = ctx.batch_results()
    return ctx, ds, feat_off, acc, gam, pw, valid, rows


@pytest.mark.parametrize("N,F,B,cap", [(30, 200, 2, 30), (30, 200, 1, 32), (32, 80, 1, None), (20, 480, 1, None),
                                       (34, 60, 1, None), (50, 120, 1, None), (50, 120, 1, 50), (80, 40, 1, None),
                                       (100, 20, 1, None)])
def test_batched_fp64_vs_oracle(N, F, B, cap):
    """cap = cam capacity of the context (default N + 2, make_ctx).  Paths exercised:
    30 -- register-tile Kalman stages, the fused information assembly
    (k_info_fused, A stored as its lower triangle), one-wave gating for every
    size class; 30 in cap 32 -- the largest register-tile Kalman window (12 x 12
    tiles) with 30 live cams; 32 (cap 34) -- the smallest global-memory Kalman
    window (32 live cams in the register-tile window, C = 192 with no padding
    row: test_gpu_track_sweep);
    20 x 480 -- more features per filter than the fused assembly's LDS holds
    (> 453): Gram records through k_info_mfma (lower triangle of A) into the same stage B;
    34 (cap 36) -- the one-workgroup-per-tile-row k_info; 50 (cap 50: four staged features per k_info
    batch, cap 52: three) -- multi-workgroup assembly, global-memory Kalman stages A / C,
    k_gate_mfma_wt on fp64 MFMA; 80 -- tracks longer than 64 observations (two
    per lane in k_feature, cam masks beyond bit 63), the MFMA assembly over six
    workgroups per filter (k_info_big);
    100 -- the longest tracks the reference chi2 table (dof <= 99,
    msckf.py:121-123) can gate."""
    problems = [synth.make_update_problem(N, F, seed=100 + b) for b in range(B)]
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float64, cap=cap)
    for b, d in enumerate(ds):
        st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
        sl = slice(feat_off[b], feat_off[b + 1])
        np.testing.assert_array_equal(valid[sl], tri_ok)
        np.testing.assert_allclose(pw[sl], tri_p, rtol=1e-9, atol=1e-10)
        np.testing.assert_array_equal(acc[sl], acc_o)
        imu, cams, P = ctx.get_state(b)
        assert rel(P, st.P) < 1e-9
        np.testing.assert_allclose(cams[:, 4:7], np.stack([c.p for c in st.cams.values()]), atol=1e-10)
        np.testing.assert_allclose(unpack_imu(imu)["p"], st.imu.p, atol=1e-10)


@pytest.mark.parametrize("kal", ["mfma", "tiles"])
@pytest.mark.parametrize("N,F,B,cap", [(30, 200, 2, 30), (32, 80, 1, None), (20, 120, 3, None),
                                       (13, 60, 2, None), (27, 100, 2, None)])
def test_kalman_cholesky_paths_vs_oracle(kal, N, F, B, cap, monkeypatch):
    """Both implementations of the Kalman stages A / C1 on the same inputs
    (MSCKF_KALMAN_CHOL forces one; by default batches of >= 64 filters take
    the fp64 MFMA partial Cholesky k_kal_mchol, smaller ones the register
    tiles of msckf_rchol.h): fp64 context against the oracle, P <= 1e-9.
    N = 13 / 27 give odd 16-column tile counts (C = 78 / 162: 5 / 11 tiles) on
    k_kal_b's two launch shapes (8 and 16 waves), whose LDS row strides depend
    on that parity."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", kal)
    problems = [synth.make_update_problem(N, F, seed=300 + b) for b in range(B)]
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float64, cap=cap)
    for b, d in enumerate(ds):
        st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
        sl = slice(feat_off[b], feat_off[b + 1])
        np.testing.assert_array_equal(acc[sl], acc_o)
        imu, cams, P = ctx.get_state(b)
        assert rel(P, st.P) < 1e-9
        np.testing.assert_allclose(cams[:, 4:7], np.stack([c.p for c in st.cams.values()]), atol=1e-10)


def check_fp32_batch(problems, cap):
    """fp32 context (P, state, triangulation and gating in fp32; Jacobians,
    assembly and Kalman in fp64) against the oracle, in two parts:

    1. decisions: triangulation validity and chi2 decisions against the plain
       fp64 oracle run; a decision may differ only where the oracle's gamma
       lies within 5 % of the threshold (fp32 gamma: median relative error
       ~1e-5, test_gate_fp32_gamma_vs_oracle);
    2. update: the oracle rerun on the GPU's OWN triangulated positions and
       accept set, from the problem rounded to fp32 as the context holds it --
       so a flipped decision never disables the covariance check.  Every
       input of the fp64 stages is then identical, and the covariance and
       the state correction must agree to fp32 rounding: P <= 1e-5 relative,
       the correction of every cam position and of the IMU position to 1e-4
       relative (the fp32 state absorbs dx at ~1e-7 of |p|).
    Returns the worst relative P deviation."""
    from msckf_amd import chi2_threshold
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float32, cap=cap)
    s2 = float(np.float32(FilterConfig().observation_noise))
    worst = 0.0
    for b, d in enumerate(ds):
        sl = slice(feat_off[b], feat_off[b + 1])
        st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
        assert (valid[sl] == tri_ok).mean() > 0.99
        both = valid[sl] & tri_ok
        np.testing.assert_allclose(pw[sl][both], tri_p[both], rtol=2e-3, atol=1e-4)
        thr = np.array([chi2_threshold(m - 1) for m in problems[b].track_lengths()])
        flip = both & (acc[sl] != acc_o)
        assert (np.abs(gam_o[flip] / thr[flip] - 1) < 0.05).all(), (gam_o[flip], thr[flip])
        assert flip.mean() <= 0.01
        d32 = rounded(d)
        st_f, acc_f, _, _, _ = oracle_update(d32, tri=(pw[sl], valid[sl]), accept=acc[sl] & valid[sl], sigma2=s2)
        imu, cams, P = ctx.get_state(b)
        e = rel(P, st_f.P)
        assert e < 1e-5, e
        worst = max(worst, e)
        dp = cams[:, 4:7] - d32["cam_p"]
        dp_o = np.stack([c.p for c in st_f.cams.values()]) - d32["cam_p"]
        assert rel(dp, dp_o) < 1e-4, rel(dp, dp_o)
        di = unpack_imu(imu)["p"] - d32["imu_p"]
        assert rel(di, st_f.imu.p - d32["imu_p"]) < 1e-4
    return worst


@pytest.mark.parametrize("cap", [30, 32])
def test_batched_fp32_vs_oracle(cap):
    """BASELINE config 2 (30 cams x 200 features, fp32) on three filters."""
    problems = [synth.make_update_problem(30, 200, seed=200 + b) for b in range(3)]
    check_fp32_batch(problems, cap)


def test_batched_fp32_50x400_vs_oracle():
    """BASELINE config 3 shape (50 cams x 400 features, fp32) at the bench's
    cam capacity 50: four-wave MFMA gating for tracks of 41..50 observations,
    global-memory Kalman stages A / C, four staged features per k_info batch."""
    problems = [synth.make_update_problem(50, 400, seed=240 + b) for b in range(2)]
    check_fp32_batch(problems, 50)


def test_batched_fp32_80x1000_vs_oracle():
    """BASELINE config 5 shape (80 cams x 1000 features, fp32): tracks up to
    80 observations (two per lane in k_feature), 16-block workgroup gating."""
    problems = [synth.make_update_problem(80, 1000, seed=260 + b) for b in range(2)]
    check_fp32_batch(problems, 80)


@pytest.mark.parametrize("N,F,B,cap", [(30, 200, 2, 30), (40, 150, 2, None), (82, 50, 1, None), (100, 70, 1, None)])
def test_gate_fp32_gamma_vs_oracle(N, F, B, cap):
    """fp32 gating on MFMA tiles against the oracle's fp64 gamma
    (msckf.py:606-614).  N = 30 (cam capacity 30, the bench's workload);
    N = 40: every one-wave size class (1..8 16-row blocks,
    single- and multi-pass Y staging); N = 82: also the multi-wave workgroup
    kernel k_gate_mfma_wt for 41 < M <= 82 (9 .. 16 blocks on two, four or
    eight waves, Y staged in passes; M = 41, 8 blocks, still one wave); N = 100:
    also the list beyond 82 observations (the global-memory workgroup kernel
    k_gate, fed by k_feature's compact QR factors and the (4M)^2 scratch that
    only such a batch allocates), up to the longest
    track the chi2 table gates.  Tolerance:
    fp32 with the saddle point's conditioning (~1e3) -- median relative error
    <= 1e-4, 99th percentile <= 1e-3; decisions: at most 1 % of the features
    differ, and only where the oracle's gamma is within 5 % of the threshold."""
    from msckf_amd import chi2_threshold
    problems = [synth.make_update_problem(N, F, seed=300 + b) for b in range(B)]
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float32, cap=cap)
    errs, nlong = [], 0
    for b, d in enumerate(ds):
        st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
        sl = slice(feat_off[b], feat_off[b + 1])
        ok = valid[sl] & tri_ok
        g, go = gam[sl][ok], gam_o[ok]
        assert np.isfinite(g).all()
        errs.append(np.abs(g - go) / np.maximum(np.abs(go), 1e-6))
        nlong += int((problems[b].track_lengths()[ok] > 82).sum())
        thr = np.array([chi2_threshold(m - 1) for m in problems[b].track_lengths()])[ok]
        flip = acc[sl][ok].astype(bool) != acc_o[ok].astype(bool)
        assert flip.mean() <= 0.01, flip.mean()
        assert (np.abs(go[flip] / thr[flip] - 1) < 0.05).all()
    e = np.concatenate(errs)
    assert e.size > 40
    if N > 82:
        assert nlong >= 8, nlong   # the M > 82 class is really exercised
    print("fp32 gamma rel err: median %.2e p99 %.2e max %.2e (%d tracks with M > 82)"
          % (np.median(e), np.quantile(e, 0.99), e.max(), nlong))
    assert np.median(e) < 1e-4, np.median(e)
    assert np.quantile(e, 0.99) < 1e-3, np.quantile(e, 0.99)


@pytest.mark.parametrize("N,F,B,nmin", [(40, 150, 2, 200), (50, 120, 1, 60), (82, 50, 1, 40)])
def test_gate_fp64_gamma_vs_oracle(N, F, B, nmin):
    """fp64 gating against the oracle's gamma (msckf.py:606-614), relative
    1e-9: the one-wave fp64 MFMA kernel (v_mfma_f64_16x16x4_f64, its own
    accumulator row layout) for every class up to 7 blocks (M <= 36, single- and
    multi-pass Y staging), and k_gate_mfma_wt (fp64 MFMA, four waves up to 10
    blocks, eight beyond) for 37 <= M <= 82 (N = 50: classes up to 50
    observations, the 50x400 bench shape; N = 82: up to 16 blocks); decisions
    identical."""
    problems = [synth.make_update_problem(N, F, seed=700 + b) for b in range(B)]
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float64)
    n = 0
    for b, d in enumerate(ds):
        st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
        sl = slice(feat_off[b], feat_off[b + 1])
        np.testing.assert_array_equal(valid[sl], tri_ok)
        ok = tri_ok.astype(bool)
        np.testing.assert_allclose(gam[sl][ok], gam_o[ok], rtol=1e-9)
        np.testing.assert_array_equal(acc[sl], acc_o)
        n += int(ok.sum())
    assert n > nmin, n


def test_gate_fp32_scrambled_observation_order():
    """gamma is invariant under a permutation of a feature's observations (an
    orthogonal row map of the stacked system, quirk Q4), so scrambling them
    must reproduce the oracle's gamma.  With slots out of order, the one-wave
    MFMA gating (k_gate_mfma) stages pair blocks Ht_a P_ab Ht_b^T with a > b
    as well as a < b, i.e. it reads P_cc blocks on both sides of the diagonal
    (the sorted case is every other fp32 test).  Tolerance as the fp32 gamma
    test: median <= 1e-4, 99th percentile <= 1e-3."""
    rng = np.random.default_rng(11)
    problems = [synth.make_update_problem(30, 200, seed=500 + b) for b in range(2)]
    ref = [oracle_update(problem_to_dict(p)) for p in problems]
    for p in problems:   # scramble in place: obs_cam / obs_z rows within each feature
        for f in range(p.F):
            o0, o1 = p.obs_off[f], p.obs_off[f + 1]
            perm = o0 + rng.permutation(o1 - o0)
            p.obs_cam[o0:o1] = p.obs_cam[perm]
            p.obs_z[o0:o1] = p.obs_z[perm]
    ctx, ds, feat_off, acc, gam, pw, valid, rows = _batched(problems, np.float32)
    errs = []
    for b, (st, acc_o, tri_p, tri_ok, gam_o) in enumerate(ref):
        sl = slice(feat_off[b], feat_off[b + 1])
        ok = valid[sl] & tri_ok
        g, go = gam[sl][ok], gam_o[ok]
        assert np.isfinite(g).all()
        errs.append(np.abs(g - go) / np.maximum(np.abs(go), 1e-6))
    e = np.concatenate(errs)
    assert e.size > 300
    assert np.median(e) < 1e-4, np.median(e)
    assert np.quantile(e, 0.99) < 1e-3, np.quantile(e, 0.99)


def test_restore_repeats_identically():
    problems = [synth.make_update_problem(20, 60, seed=7 + b) for b in range(2)]
    ds = [problem_to_dict(p) for p in problems]
    ctx = make_ctx(ds, dtype=np.float32)
    feat_off = np.concatenate([[0], np.cumsum([p.F for p in problems])])
    obs_off, cams, zs, chi = [0], [], [], []
    for p in problems:
        obs_off.extend(list(obs_off[-1] + p.obs_off[1:]))
        cams.extend(p.obs_cam)
        zs.extend(p.obs_z)
        chi.extend(chi2_for(p.track_lengths()))
    ctx.batch_load(feat_off, obs_off, cams, np.array(zs), None, np.array(chi))
    ctx.snapshot()
    outs = []
    for _ in range(3):
        ctx.restore()
        ctx.batch_update()
        ctx.sync()
        outs.append(ctx.get_state(1)[2])
    np.testing.assert_array_equal(outs[0], outs[1])
    np.testing.assert_array_equal(outs[0], outs[2])


# ------------------------------------------------------------ whole filter --

def _run_sequence(flt, seq):
    recs = []
    for kind, m in seq.events():
        if kind == 0:
            flt.imu_callback(m)
            continue
        res = flt.feature_callback(m)
        if res is None:
            continue
        s = flt.imu_state()
        P = flt.state_cov()
        recs.append(np.concatenate([
            [m.timestamp], s["q"], s["p"], s["v"], s["bg"], s["ba"], s["R_imu_cam0"].ravel(), s["t_cam0_imu"],
            [np.linalg.norm(P), np.trace(P), P.shape[0], len(flt.cam_ids), len(flt.map_server)],
            res.cam0_pose._vio_R__.ravel(), res.cam0_pose._vio_t__]))
    return np.array(recs)


@pytest.mark.parametrize("name", ["sequence_s1", "sequence_s2", "sequence_s3"])
def test_sequence_golden(name):
    """The reference filter's runs, reproduced through the drop-in MSCKF
    class: identical gating decisions, stacked-H shapes and online-reset
    frames, state and covariance norm within 1e-6 relative (north star
    tolerance).  s1: EuRoC config, 200 frames; s2: check_motion at translation
    threshold 0.2 (feature.py:124-165); s3: online_reset firing at position
    std 0.11 m (msckf.py:859-886).  (s4: test_sequence_s4_degenerate.)"""
    _check_sequence(name)


def test_sequence_s1_mfma_cholesky(monkeypatch):
    """s1 with the Kalman stages A / C1 forced onto k_kal_mchol (a batch of
    one takes the register tiles by default)."""
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", "mfma")
    _check_sequence("sequence_s1")


def test_sequence_s4_mfma_cholesky(monkeypatch):
    """s4 on k_kal_mchol: after its degenerate frame-3 update the reference's
    non-Joseph covariance update leaves P_cc indefinite, the first partial
    Cholesky fails and the filter is factored again with a shifted P_cc by the
    retry launch (its parallel scan of the failed filters).  The stream must
    run to the end, frames 0-2 on the reference (<= 1e-6), and the trajectory
    as close to the ground truth as the reference's own."""
    from msckf_amd.trajectory import Trajectory, ate
    from msckf_amd.replay import FeatureStream
    monkeypatch.setenv("MSCKF_KALMAN_CHOL", "mfma")
    g = golden("sequence_s4")
    seq = synth.make_sequence(int(g["n_frames"]), int(g["seed"]))
    flt = msckf_amd.MSCKF(sequence_config(g))
    rec = _run_sequence(flt, seq)
    flt.close()
    ref = g["rec"]
    assert rec.shape == ref.shape
    for k in range(3):
        assert np.linalg.norm(rec[k, 1:29] - ref[k, 1:29]) <= 1e-6 * np.linalg.norm(ref[k, 1:29]), k
    gt = FeatureStream.from_synthetic(seq).gt
    ate_gpu = ate(Trajectory(rec[:, 0], rec[:, 5:8]), gt)
    ate_ref = ate(Trajectory(ref[:, 0], ref[:, 5:8]), gt)
    print("s4 (mfma Cholesky): ATE vs ground truth: device %.4f m, reference %.4f m" % (ate_gpu, ate_ref))
    assert ate_gpu <= 2 * ate_ref + 0.01


def _check_sequence(name):
    g = golden(name)
    seq = synth.make_sequence(int(g["n_frames"]), int(g["seed"]))
    flt = msckf_amd.MSCKF(sequence_config(g))
    rec = _run_sequence(flt, seq)
    np.testing.assert_array_equal(np.array(flt.gate_log), g["gates"])
    np.testing.assert_array_equal(np.array(flt.shape_log), g["shapes"])
    assert rec.shape == g["rec"].shape
    ref = g["rec"]
    # record: t | q p v bg ba R_ic t_ci (cols 1..28) | |P|_F trace(P) | D #cams #features | cam0 pose
    for k in range(len(ref)):
        x, xr = rec[k, 1:29], ref[k, 1:29]
        assert np.linalg.norm(x - xr) <= 1e-6 * np.linalg.norm(xr), k
        assert abs(rec[k, 29] - ref[k, 29]) <= 1e-6 * ref[k, 29], k     # |P|_F
    np.testing.assert_array_equal(rec[:, 31:34], ref[:, 31:34])          # D, #cams, #features
    worst = max(np.linalg.norm(rec[k, 1:29] - ref[k, 1:29]) / np.linalg.norm(ref[k, 1:29]) for k in range(len(ref)))
    print("sequence: worst per-frame state deviation %.3e" % worst)
    assert rel(flt.state_cov(), g["P_final"]) < 1e-6
    np.testing.assert_array_equal(flt.reset_log, g["resets"] if "resets" in g else [])


def test_gate_fp32_unordered_tracks():
    """Tracks whose cam slots do not ascend (the reference always lists a
    feature's observations in cam order, but the C-ABI takes any order):
    gamma is invariant to the order of a feature's observations, so the
    reversed tracks must gate like the ordered ones."""
    p = synth.make_update_problem(20, 120, seed=411)
    d = problem_to_dict(p)
    st, acc_o, tri_p, tri_ok, gam_o = oracle_update(d)
    sel = [f for f in range(p.F) if tri_ok[f]]
    res = {}
    for order in (1, -1):
        obs = [feature_obs(d, f)[::order] for f in sel]
        off = np.concatenate([[0], np.cumsum([len(o) for o in obs])])
        cams = [c for o in obs for c, _ in o]
        zs = [z for o in obs for _, z in o]
        ctx = make_ctx(d, dtype=np.float32)
        acc, gam, rows = ctx.update(0, off, cams, zs, tri_p[sel], chi2_for(np.diff(off)))
        res[order] = gam
        ctx.close()
    e = np.abs(res[-1] - gam_o[sel]) / np.maximum(np.abs(gam_o[sel]), 1e-6)
    assert np.median(e) < 1e-4 and np.quantile(e, 0.99) < 1e-3, (np.median(e), np.quantile(e, 0.99))
    np.testing.assert_allclose(res[-1], res[1], rtol=1e-3, atol=1e-6)


def test_gate_degenerate_exact():
    """A gating case where the reference's own arithmetic is rounding noise
    (tests/golden/degenerate_gate.npz, tools/gen_degenerate_gate.py): a
    landmark 0.86 mm in front of the camera on golden sequence s4, so
    S = H P H^T + s2 I (msckf.py:606-609) has condition ~5e18.  The reference
    formula in fp64 gives gamma = 0.00187 (and 0.0004, 0.00025 or 'singular'
    in other, equally valid nullspace bases); the 50-digit value is 0.0052820.
    The device's saddle-point elimination must give the exact value (1e-6),
    and the well-conditioned second feature must match both."""
    g = golden("degenerate_gate")
    n = (g["P"].shape[0] - 21) // 6
    ctx = Context(FilterConfig(), n_filters=1, n_cam_capacity=n + 2, dtype=np.float64)
    ctx.set_state(0, g["imu"], g["cams"], g["P"])
    acc, gam, rows = ctx.update(0, g["obs_off"], g["obs_cam"], g["obs_z"], g["p_w"], g["chi2"])
    ctx.close()
    np.testing.assert_allclose(gam, g["gamma_exact"], rtol=1e-6)
    assert g["cond_S"][0] > 1e18 and abs(g["gamma_ref_fp64"][0] / g["gamma_exact"][0] - 1) > 0.5
    assert abs(g["gamma_ref_fp64"][1] / g["gamma_exact"][1] - 1) < 1e-8


def test_sequence_s4_degenerate():
    """Golden sequence s4 (180 frames, seed 307): landmarks triangulated
    millimetres from the camera make the reference's S singular in fp64
    (test_gate_degenerate_exact), and its non-Joseph covariance update leaves
    P_cc indefinite at rounding level from frame 2 on.  What the HIP path is
    held to:

    1. it runs the whole stream -- stage A's pivot floor (msckf_rchol.h,
       pivot_floored) instead of a non-PD abort;
    2. every frame before the first one that leaves the north-star band is
       within it: state vector and |P|_F <= 1e-6 relative, gating decisions
       and stacked shapes identical;
    3. that first frame k0 (frame 3) is an update the reference itself does not
       determine to 1e-6: replayed with the reference's formulas
       (msckf.py:500-604) from the device's pre-update state, it moves by more
       than 1e-6 -- and by more than the device's own deviation -- when the
       SVD nullspace basis (msckf.py:535-539) is swapped for another
       orthonormal basis of the same nullspace (exactly equivalent in exact
       arithmetic, quirk Q4), because it accepts a feature whose gamma changes
       by more than 50 % under that swap (a degenerate feature);
    4. the decisions that differ afterwards follow from that frame (the first
       one is recorded), and the trajectory stays as close to the ground truth
       as the reference's own (ATE <= 2 x the reference's + 1 cm)."""
    from msckf_amd.trajectory import Trajectory, ate
    from msckf_amd.replay import FeatureStream
    from helpers import oracle_state_from_device, gamma_basis_spread
    g = golden("sequence_s4")
    seq = synth.make_sequence(int(g["n_frames"]), int(g["seed"]))
    flt = msckf_amd.MSCKF(sequence_config(g))
    trace = []
    orig_update, orig_serve = flt._update, flt._serve

    def traced_update(feats, cam_lists, dofs, row_cap, to_init=()):
        trace.append(dict(frame=flt._n_published, ids=[f.id for f in feats]))
        return (yield from orig_update(feats, cam_lists, dofs, row_cap, to_init))

    class _Traced:
        def __init__(self, pend, entry):
            self.pend, self.entry = pend, entry

        def get(self):
            res = self.pend.get()
            self.entry["res"] = res
            return res

    def traced_serve(req):
        if req[0] != "update":
            return orig_serve(req)
        e = trace[-1]
        e["pre"] = flt.ctx.get_state(flt.slot)
        e["req"] = req[1:]
        pend = orig_serve(req)
        e["post"] = flt.ctx.get_state(flt.slot)
        return _Traced(pend, e)

    flt._update, flt._serve = traced_update, traced_serve
    rec = _run_sequence(flt, seq)
    flt.close()
    assert rec.shape == g["rec"].shape
    ref = g["rec"]

    def dev(k):
        return np.linalg.norm(rec[k, 1:29] - ref[k, 1:29]) / np.linalg.norm(ref[k, 1:29])

    k0 = next((k for k in range(len(ref)) if dev(k) > 1e-6 or abs(rec[k, 29] - ref[k, 29]) > 1e-6 * ref[k, 29]),
              len(ref))
    assert k0 < len(ref), "s4 stays within 1e-6: it should then pass test_sequence_golden's bounds"
    # the departure frame is pinned: frames 0-2 carry no degenerate accepted
    # feature and must stay on the reference (an earlier departure is a regression)
    assert k0 >= 3, "s4 leaves the 1e-6 band at frame %d, before the degenerate frame 3" % k0
    gl, ref_gl = [tuple(x) for x in flt.gate_log], [tuple(x) for x in g["gates"]]
    assert [x for x in gl if x[0] < k0] == [x for x in ref_gl if x[0] < k0]
    assert [tuple(x) for x in flt.shape_log if x[0] < k0] == [tuple(x) for x in g["shapes"] if x[0] < k0]
    np.testing.assert_array_equal(rec[:k0, 31:34], ref[:k0, 31:34])
    worst = max([dev(k) for k in range(k0)] + [0.0])
    # frame k0's update, replayed with the reference's formulas from the device's pre-update state
    ups = [e for e in trace if e["frame"] == k0]
    assert ups, "frame %d leaves the band without an update" % k0
    e = ups[0]
    st0 = oracle_state_from_device(*e["pre"])
    off, cams, zs, _, chi2, _ = e["req"]
    acc, gam, p, valid, rows = e["res"]
    obs = [[(int(cams[o]), zs[o]) for o in range(off[j], off[j + 1])] for j in range(len(off) - 1)]

    def replay(seed):
        st = st0.copy()
        rng = None if seed is None else np.random.default_rng(seed)
        Hs, rs = [], []
        for j in range(len(obs)):
            if not valid[j]:
                continue
            H, r = O.feature_jacobian(st, p[j], obs[j])
            if rng is not None:
                Q, _ = np.linalg.qr(rng.standard_normal((len(r), len(r))))
                H, r = Q @ H, Q @ r
            if O.gating_gamma(st, H, r) < chi2[j]:
                Hs.append(H)
                rs.append(r)
        if Hs:
            O.measurement_update(st, np.vstack(Hs), np.concatenate(rs))
        return np.concatenate([st.imu.q, st.imu.p, st.imu.v, st.imu.bg, st.imu.ba, st.imu.R_imu_cam0.ravel(),
                               st.imu.t_cam0_imu])

    s_svd = replay(None)
    spread = max(np.linalg.norm(replay(sd) - s_svd) / np.linalg.norm(s_svd) for sd in range(4))
    s = _lib_unpack(e["post"][0])
    dev_k0 = np.linalg.norm(s - s_svd) / np.linalg.norm(s_svd)
    degenerate = []
    for j in range(len(obs)):
        if valid[j] and acc[j]:
            g_ref, sp = gamma_basis_spread(st0, p[j], obs[j])
            if sp > 0.5:
                degenerate.append((e["ids"][j], g_ref, sp))
    i = next((k for k in range(min(len(gl), len(ref_gl))) if gl[k] != ref_gl[k]), None)
    print("s4: frames 0..%d within %.2e of the reference; frame %d leaves the band (device %.2e from the reference): "
          "its update moves by %.2e under another nullspace basis (device vs SVD-basis replay %.2e); degenerate "
          "accepted features (id, gamma, basis spread): %s; first differing decision: device %s vs reference %s"
          % (k0 - 1, worst, k0, dev(k0), spread, dev_k0, degenerate,
             gl[i] if i is not None else None, ref_gl[i] if i is not None else None))
    assert spread > 1e-6 and dev_k0 <= spread, (spread, dev_k0)
    assert degenerate
    gt = FeatureStream.from_synthetic(seq).gt
    ate_gpu = ate(Trajectory(rec[:, 0], rec[:, 5:8]), gt)
    ate_ref = ate(Trajectory(g["rec"][:, 0], g["rec"][:, 5:8]), gt)
    print("s4: ATE vs ground truth: device %.4f m, reference %.4f m" % (ate_gpu, ate_ref))
    assert ate_gpu <= 2 * ate_ref + 0.01


def _lib_unpack(imu_rec):
    u = unpack_imu(imu_rec)
    return np.concatenate([u["q"], u["p"], u["v"], u["bg"], u["ba"], u["R_imu_cam0"].ravel(), u["t_cam0_imu"]])
