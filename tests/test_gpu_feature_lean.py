"""The lean feature-Jacobian kernel of the fused path (k_feature_lean: factored
Jacobian, QR on the rotated 3M x 3 rows, if_rcp / if_rsq) against
the full kernel k_feature on the same inputs -- MSCKF_FEATURE=full|lean, read
per call -- and both against the CPU oracle.

Bounds are the project's own against the oracle (tests/track_sweep.py
check_sweep and test_gpu_parity.py: fp64 gamma rtol 1e-9, rel(P) < 1e-9,
positions atol 1e-10; fp32 gamma median < 1e-4 / p99 < 1e-3 / FP32_GAMMA_CAP,
rel(P) < 1e-5, position corrections < 1e-4); decisions, valid flags and stacked
rows of the lean path must equal the full path's exactly.  Features the lean
kernel finds ill-conditioned (FQR_RMAX / FQR_KAPPA, csrc/msckf_common.h) go
through the full kernel in a second pass, so their gamma is bit-identical.

Measured on an MI355X (profiles/feature_lean/README.md), deviation from the
oracle, full / lean: N = 32 sweep fp64 rel(P) 4.4e-14 / 3.7e-14 and 3.6e-14 /
3.2e-14 (the two filters), worst gamma error 5.4e-14 / 6.9e-14; fp32 rel(P)
2.6e-8 and worst gamma error 9.1e-6 in both, gamma and P of the two paths
bit-identical; small windows fp64 rel(P) 1.0e-14 / 7.5e-15 (with ill features)
and 2.0e-14 / 1.2e-14 (without), fp32 2.7e-8 / 2.7e-8.  Lean against full in
fp64: gamma within 4.0e-14, P within 2.9e-14.
"""
import ctypes
import dataclasses
from collections import OrderedDict

import numpy as np
import pytest

from helpers import oracle_state_from_arrays, oracle_update, problem_to_dict, rounded
from oracle import msckf_oracle as O
from track_sweep import SWEEP_SEEDS, cached_sweep, check_sweep, state_arrays
from msckf_amd import synth, FilterConfig, CHI2_05
from msckf_amd._lib import Context, pack_imu, pack_cams, unpack_imu

pytestmark = pytest.mark.gpu

FQR_RMAX, FQR_KAPPA = 1e3, 1e4   # csrc/msckf_common.h


def _imu(pr):
    d = problem_to_dict(pr)
    return pack_imu(q=d["imu_q"], p=d["imu_p"], v=d["imu_v"], bg=d["imu_bg"], ba=d["imu_ba"],
                    q_null=d["imu_q_null"], p_null=d["imu_p_null"], v_null=d["imu_v_null"],
                    R_imu_cam0=d["imu_R_imu_cam0"], t_cam0_imu=d["imu_t_cam0_imu"], gravity=d["gravity"], alias=True)


def _update(monkeypatch, mode, problems, chi2s, p_ws, dtype, cap, lanes=None):
    """One batched update on a fresh context under MSCKF_FEATURE=mode.  p_ws: per
    filter the host's positions (NaN rows are triangulated on the device) or
    None for all (then every feature is triangulated).  Returns the raw results
    and per filter the dict check_sweep takes."""
    monkeypatch.setenv("MSCKF_FEATURE", mode)
    if lanes:
        monkeypatch.setenv("MSCKF_SUBBATCH", str(lanes))
    ctx = Context(FilterConfig(), n_filters=len(problems), n_cam_capacity=cap, dtype=dtype)
    try:
        for b, pr in enumerate(problems):
            ctx.set_state(b, _imu(pr), pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P)
        feat_off = np.concatenate([[0], np.cumsum([p.F for p in problems])])
        obs_off = np.concatenate([[0], np.cumsum(np.concatenate([p.track_lengths() for p in problems]))])
        cams = np.concatenate([p.obs_cam for p in problems])
        zs = np.concatenate([p.obs_z for p in problems])
        p_w = None if p_ws is None else np.concatenate(p_ws)
        ctx.batch_load(feat_off, obs_off, cams, zs, p_w, np.concatenate(chi2s))
        ctx.batch_update(row_cap=0, triangulate=True)
        if lanes:   # the split was taken (debug hook of the library, as test_gpu_subbatch.py)
            fn = ctx.lib.msckf_debug_lanes
            fn.argtypes, fn.restype = [ctypes.c_void_p], ctypes.c_int
            assert ctx._check(fn(ctx.h)) == lanes
        acc, gam, pw, valid, rows = ctx.batch_results()
        got = []
        for b in range(len(problems)):
            sl = slice(feat_off[b], feat_off[b + 1])
            imu, cam, P = ctx.get_state(b)
            got.append(dict(valid=valid[sl], p_w=pw[sl], gamma=gam[sl], accept=acc[sl], rows=int(rows[b]), P=P,
                            cam_p=cam[:, 4:7], imu_p=unpack_imu(imu)["p"], imu=imu, cams=cam))
        return (acc, gam, pw, valid, rows), got
    finally:
        ctx.close()


def _same_decisions(lean, full, label):
    for key in ("valid", "accept", "rows"):
        np.testing.assert_array_equal(lean[key], full[key], err_msg="%s: %s" % (label, key))
    np.testing.assert_array_equal(lean["p_w"], full["p_w"], err_msg=label)   # triangulation is not touched


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - b) / np.linalg.norm(b)


# ------------------------------------------------- 1. old against new: the sweep --

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_full_vs_lean_track_sweep(dtype, monkeypatch):
    """The N = 32 sweep of test_gpu_track_sweep (one feature for every M = 2 ..
    32, shuffled, contiguous and gapped cam slots alternating; the segment
    boundaries 8|9 and 16|17 and the largest track the fused path's window
    allows, M = 32 -- the S = 64 class and tracks of 33+ observations need more
    than 32 cams, where the fused assembly and with it the lean kernel do not
    run).  Classes: S = 8 holds 7 features (not a multiple of 64 / 8), S = 16
    eight, S = 32 sixteen.  Two filters (flip 0 / 1) in one context."""
    N = 32
    filters = [cached_sweep(N, SWEEP_SEEDS[N] + flip, flip) for flip in (0, 1)]
    problems, chi2s = [pr for pr, _ in filters], [ref.chi2 for _, ref in filters]
    _, full = _update(monkeypatch, "full", problems, chi2s, None, dtype, N)
    _, lean = _update(monkeypatch, "lean", problems, chi2s, None, dtype, N)
    for b, (pr, ref) in enumerate(filters):
        label = "N=32 %s filter %d" % (np.dtype(dtype).name, b)
        _same_decisions(lean[b], full[b], label)
        state = None
        if dtype == np.float32:   # the oracle rerun on the device's own positions and decisions (check_fp32_batch)
            d32 = rounded(problem_to_dict(pr))
            s2 = float(np.float32(FilterConfig().observation_noise))
            st = oracle_update(d32, tri=(lean[b]["p_w"], lean[b]["valid"]),
                               accept=lean[b]["accept"] & lean[b]["valid"], sigma2=s2)[0]
            state = state_arrays(st) + (d32["cam_p"], d32["imu_p"])
        for mode, got in (("full", full[b]), ("lean", lean[b])):
            out = check_sweep(ref, got, dtype, "%s %s" % (label, mode), state=state)
            print("%s %s: rel(P) %.3e, worst gamma error %.3e" % (label, mode, out["rel_P"],
                                                                  max(out["route_worst"].values())))
        print("%s lean against full: gamma %.3e, P %.3e" % (
            label, np.nanmax(np.abs(lean[b]["gamma"] / full[b]["gamma"] - 1)), _rel(lean[b]["P"], full[b]["P"])))


# ------------------------------------- 2. small windows: M = 0, ill routing, lanes --

def _project(pr, L, c):
    R0 = O.to_rotation(pr.cam_q[c])
    pc0 = R0 @ (L - pr.cam_p[c])
    R1 = pr.R_cam0_cam1 @ R0
    pc1 = R1 @ (L - (pr.cam_p[c] - R1.T @ pr.t_cam0_cam1))
    return pc0, pc1


def _append(pr, L, cams, z):
    """The problem with one more feature: landmark L seen from the cam slots `cams` at z."""
    return dataclasses.replace(pr, F=pr.F + 1, landmarks=np.vstack([pr.landmarks, L]),
                               obs_off=np.append(pr.obs_off, pr.obs_off[-1] + len(cams)).astype(np.int32),
                               obs_cam=np.append(pr.obs_cam, cams).astype(np.int32), obs_z=np.vstack([pr.obs_z, z]))


def _with_near_landmark(pr, c, depth=1e-3):
    """A landmark `depth` metres in front of cam slot c, seen by c and by the (up
    to two) other cams it lies deepest in front of, in both eyes; None if it is
    in front of no other cam (the cams stand almost in one plane)."""
    L = pr.cam_p[c] + O.to_rotation(pr.cam_q[c]).T @ np.array([0.0, 0.0, depth])
    d = np.array([min(p[2] for p in _project(pr, L, k)) for k in range(pr.N)])
    others = [k for k in np.argsort(d)[::-1] if k != c and d[k] > 0.5 * depth][:2]
    if not others or d[c] <= 0:
        return None
    cams = np.sort(np.append(others, c))
    z = np.array([[p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]]
                  for p0, p1 in (_project(pr, L, k) for k in cams)])
    return _append(pr, L, cams, z)


def _trips(pr, p_w, f):
    """k_feature's ill test on the oracle's H_f of feature f (R of its QR)."""
    d = problem_to_dict(pr)
    st = oracle_state_from_arrays(d)
    a, b = int(pr.obs_off[f]), int(pr.obs_off[f + 1])
    Hf = np.vstack([O.measurement_jacobian(st, st.cams[int(c)], p_w, z)[1]
                    for c, z in zip(pr.obs_cam[a:b], pr.obs_z[a:b])])
    rd = np.abs(np.diag(np.linalg.qr(Hf)[1]))
    return not rd.max() <= FQR_RMAX or not rd.max() <= FQR_KAPPA * rd.min()


def _small_problem(seed, n_near, behind=False, gapped=False):
    """8 cams, 12 synthetic features (tracks of 3 .. 8) with positions given by the
    host (the oracle's triangulation), then optionally: a gapped track (slots 0,
    2, 5, 7 of a synthetic landmark), a landmark behind the cams whose position
    the device must triangulate and reject (the M = 0 path), and a landmark 1 mm
    in front of each of the first `n_near` cams that allow it (host-given, never accepted: chi2 = 0).
    Returns (problem, chi2, p_w with a NaN row where the device triangulates,
    ill mask)."""
    pr = synth.make_update_problem(8, 12, seed=seed)
    d = problem_to_dict(pr)
    st = oracle_state_from_arrays(d)
    p_w = [O.triangulate(OrderedDict((int(c), z) for c, z in zip(pr.obs_cam[a:b], pr.obs_z[a:b])), st.cams,
                         st.R_cam0_cam1, st.t_cam0_cam1)[0] for a, b in zip(pr.obs_off[:-1], pr.obs_off[1:])]
    chi2 = [CHI2_05[m - 2] for m in pr.track_lengths()]
    ill = [False] * pr.F
    if gapped:
        cams = np.array([0, 2, 5, 7])
        L = pr.landmarks[0]
        z = np.array([[p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]]
                      for p0, p1 in (_project(pr, L, k) for k in cams)])
        z += (0.5 / 458.654) * np.random.default_rng([seed, 1]).standard_normal(z.shape)   # synth's pixel noise
        pr = _append(pr, L, cams, z)
        p_w.append(L), chi2.append(CHI2_05[2]), ill.append(False)
    if behind:
        L = np.array([0.2, 0.1, -4.0])
        cams = np.array([1, 2, 3])
        z = np.array([[p0[0] / p0[2], p0[1] / p0[2], p1[0] / p1[2], p1[1] / p1[2]]
                      for p0, p1 in (_project(pr, L, k) for k in cams)])
        pr = _append(pr, L, cams, z)
        ok = O.triangulate(OrderedDict((int(c), zz) for c, zz in zip(cams, z)), st.cams, st.R_cam0_cam1,
                           st.t_cam0_cam1)[1]
        assert not ok, "the landmark behind the cams must fail the oracle's triangulation"
        p_w.append(np.full(3, np.nan)), chi2.append(CHI2_05[1]), ill.append(False)
    for c in range(pr.N):
        near = _with_near_landmark(pr, c) if sum(ill) < n_near else None
        if near is not None:
            pr = near
            p_w.append(pr.landmarks[-1]), chi2.append(0.0), ill.append(True)
    assert sum(ill) == n_near
    p_w, ill = np.array(p_w), np.array(ill)
    # shuffle the features, so that ill ones sit among the others in every list
    perm = np.random.default_rng(seed).permutation(pr.F)
    M = pr.track_lengths()
    rows = np.concatenate([np.arange(pr.obs_off[f], pr.obs_off[f + 1]) for f in perm])
    pr = dataclasses.replace(pr, landmarks=pr.landmarks[perm], obs_cam=pr.obs_cam[rows], obs_z=pr.obs_z[rows],
                             obs_off=np.concatenate([[0], np.cumsum(M[perm])]).astype(np.int32))
    p_w, ill, chi2 = p_w[perm], ill[perm], np.array(chi2)[perm]
    for f in range(pr.F):   # the premise, on the CPU: exactly the near landmarks trip k_feature's test
        if np.isfinite(p_w[f]).all():
            assert _trips(pr, p_w[f], f) == bool(ill[f]), (f, ill[f])
    return pr, chi2, p_w, ill


def _check_small(pr, p_w, ill, got, dtype, label):
    """Against the oracle on the host's positions: decisions of the
    well-conditioned features, and the update on the device's own decisions (an
    ill feature is never accepted, chi2 = 0) within the parity bounds."""
    d = problem_to_dict(pr)
    giv = np.isfinite(p_w).all(1)
    np.testing.assert_array_equal(got["valid"], giv, err_msg=label)   # the landmark behind the cams fails
    assert not got["accept"][ill].any() and not got["accept"][~giv].any(), label
    tri = (np.where(giv[:, None], p_w, 0.0), giv & ~ill)   # the oracle skips what no path may accept
    if dtype == np.float64:
        _, acc_o, _, _, gam_o = oracle_update(d, tri=tri)
        ok = tri[1]
        np.testing.assert_array_equal(got["accept"][ok], acc_o[ok], err_msg=label)
        np.testing.assert_allclose(got["gamma"][ok], gam_o[ok], rtol=1e-9, err_msg=label)
        st = oracle_update(d, tri=tri, accept=got["accept"])[0]
        e = _rel(got["P"], st.P)
        print("%s: rel(P) %.3e" % (label, e))
        assert e < 1e-9, (label, e)
        np.testing.assert_allclose(got["cam_p"], np.stack([c.p for c in st.cams.values()]), atol=1e-10, err_msg=label)
        np.testing.assert_allclose(got["imu_p"], st.imu.p, atol=1e-10, err_msg=label)
    else:
        d32 = rounded(d)
        s2 = float(np.float32(FilterConfig().observation_noise))
        tri32 = (tri[0].astype(np.float32).astype(np.float64), tri[1])
        st = oracle_update(d32, tri=tri32, accept=got["accept"], sigma2=s2)[0]
        e = _rel(got["P"], st.P)
        print("%s: rel(P) %.3e" % (label, e))
        assert e < 1e-5, (label, e)
        dp, dp_o = got["cam_p"] - d32["cam_p"], np.stack([c.p for c in st.cams.values()]) - d32["cam_p"]
        assert _rel(dp, dp_o) < 1e-4, (label, _rel(dp, dp_o))


@pytest.fixture(scope="module")
def small():
    """Filter 0: three near landmarks, a gapped track and a failing triangulation;
    filter 1: no ill feature.  8 live cams in capacity 10."""
    return [_small_problem(700, n_near=3, behind=True, gapped=True),
            _small_problem(701, n_near=0, behind=False, gapped=True)]


@pytest.mark.parametrize("which", ["ill", "none"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ill_routing(small, dtype, which, monkeypatch):
    """Landmarks 1 mm in front of a cam (|R| > FQR_RMAX: H_f scales as 1 / depth)
    among well-conditioned features: under `lean` their gamma is bit-identical to
    `full` (they ran k_feature in the second pass), every decision is the full
    path's, the update is within the oracle bounds.  `none`: no ill feature -- the
    count is zero and the second pass is a no-op."""
    pr, chi2, p_w, ill = small[0 if which == "ill" else 1]
    assert ill.sum() == (3 if which == "ill" else 0)
    _, full = _update(monkeypatch, "full", [pr], [chi2], [p_w], dtype, 10)
    _, lean = _update(monkeypatch, "lean", [pr], [chi2], [p_w], dtype, 10)
    label = "small %s %s" % (which, np.dtype(dtype).name)
    _same_decisions(lean[0], full[0], label)
    np.testing.assert_array_equal(lean[0]["gamma"][ill], full[0]["gamma"][ill], err_msg=label)
    assert np.isfinite(lean[0]["gamma"][lean[0]["valid"]]).all(), label
    for mode, got in (("full", full[0]), ("lean", lean[0])):
        _check_small(pr, p_w, ill, got, dtype, "%s %s" % (label, mode))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ill_features_in_both_lanes(dtype, monkeypatch):
    """Eight filters as two lanes (filters 0..3 and 4..7) with near landmarks in
    filters of both: bitwise the one-lane run of the same batch, as
    test_gpu_subbatch.py compares lanes (the ill lists and counts are per lane)."""
    sets = [_small_problem(710 + b, n_near=2 if b in (1, 2, 5, 7) else 0, behind=b == 6, gapped=b % 2 == 0)
            for b in range(8)]
    problems, chi2s, p_ws = [s[0] for s in sets], [s[1] for s in sets], [s[2] for s in sets]
    assert sum(s[3].sum() for s in sets[:4]) > 0 and sum(s[3].sum() for s in sets[4:]) > 0
    two = _update(monkeypatch, "lean", problems, chi2s, p_ws, dtype, 10, lanes=2)
    one = _update(monkeypatch, "lean", problems, chi2s, p_ws, dtype, 10, lanes=1)
    for name, a, b in zip(("accepted", "gamma", "p_w", "valid", "rows"), two[0], one[0]):
        np.testing.assert_array_equal(a, b, err_msg=name)
    for b, (g2, g1) in enumerate(zip(two[1], one[1])):
        for key in ("imu", "cams", "P"):
            np.testing.assert_array_equal(g2[key], g1[key], err_msg="%s of filter %d" % (key, b))
    full = _update(monkeypatch, "full", problems, chi2s, p_ws, dtype, 10, lanes=2)
    for b, s in enumerate(sets):
        _same_decisions(two[1][b], full[1][b], "filter %d" % b)
        np.testing.assert_array_equal(two[1][b]["gamma"][s[3]], full[1][b]["gamma"][s[3]])
