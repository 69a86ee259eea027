"""Track-length sweep through the EKF update: one feature for every
observation count M = 2 .. N, the oracle reference, and the comparison of a
device run against it.  Pure numpy + the oracle (no GPU import): the builder
and the comparator are themselves tested on the CPU (test_track_sweep_ref.py)
and used by the GPU parity sweep (test_gpu_track_sweep.py).

The per-feature kernels are chosen by M: SegClasses for triangulation and the
Jacobians, and for the gate the one table of csrc/msckf_gate_routes.h (a feature
list per block count, M >= 83 last).  ``route_of`` groups results by the gate
kernel that produced them; it is finer than the device's lists in one place (41
apart from 37..40), and test_track_sweep_ref.py compares it with the header.
"""
import copy
import functools
from collections import OrderedDict, namedtuple

import numpy as np

from helpers import feature_obs, oracle_state_from_arrays, oracle_update, problem_to_dict
from oracle import msckf_oracle as O
from msckf_amd import synth
from msckf_amd.geometry import to_rotation

# Gate routes, by index into ROUTE_BOUNDS.  A track of M <= 82 observations
# fills nb = ceil((3M + 4) / 16) 16-row blocks:
#   0 .. 7   the lists of 1 .. 8 blocks up to M = 40: M <= 4, 5..9, 10..14, 15..20,
#            21..25, 26..30, 31..36, 37..40
#   8        M = 41, the last track of 8 blocks (on the device in the list of 37..40)
#   9 .. 16  the lists of 9 .. 16 blocks: 42..46 | 47..52 | 53..57 | 58..62 |
#            63..68 | 69..73 | 74..78 | 79..82
#   17       M >= 83
ROUTE_BOUNDS = [(2, 4), (5, 9), (10, 14), (15, 20), (21, 25), (26, 30), (31, 36), (37, 40),
                (41, 41), (42, 46), (47, 52), (53, 57), (58, 62), (63, 68), (69, 73), (74, 78), (79, 82),
                (83, 128)]
SEG_EDGES = (8, 9, 16, 17, 32, 33, 64, 65, 128)


def route_of(M):
    """Index into ROUTE_BOUNDS of a track of M observations (from the block
    count, as the device computes it -- not from the table above, which the CPU
    test compares with it)."""
    M = int(M)
    if M > 82:
        return 17
    nb = (3 * M + 4 + 15) // 16
    return nb - 1 if M <= 40 else nb


def route_name(r):
    lo, hi = ROUTE_BOUNDS[r]
    return "M=%d" % lo if lo == hi else "M=%d..%d" % (lo, hi)


# fp32 per-feature cap on the relative gamma error: 10 x the worst value measured
# on an MI355X over both windows and steps 1 and 2 of test_gpu_track_sweep
# (8.96e-5, a track of 69..73 observations at N = 128; per route in that test's
# docstring).  The margin is for the worst of ~500 samples of a rounding-error
# distribution moving with the seed; the project's p99 bound is 1e-3.
FP32_GAMMA_CAP = 9.0e-4

SweepRef = namedtuple("SweepRef", "M route gapped tri_p tri_ok gamma chi2 acc rows P cam_p imu_p cam_p0 imu_p0")


def sweep_problem(N, seed, flip):
    """UpdateProblem with one feature for every M in 2 .. N on the state (cams,
    IMU, P) of synth.make_update_problem(N, 4, seed).  A track is a contiguous
    window of cam slots when M + flip is even, else M distinct slots drawn
    without replacement (ascending); the features are shuffled."""
    base = synth.make_update_problem(N, 4, seed)
    rng = np.random.default_rng([int(seed), int(flip), int(N), 2128])
    Ms = np.arange(2, N + 1)
    rng.shuffle(Ms)
    F = len(Ms)
    # landmarks, projection and noise as synth.make_update_problem
    lo, hi = np.array([-1.5, -1.5, 3.0]), np.array([3.0, 1.5, 8.0])
    L = lo + (hi - lo) * rng.random((F, 3))
    Rcc, tcc = base.R_cam0_cam1, base.t_cam0_cam1
    cam_R = [to_rotation(q) for q in base.cam_q]
    slots = []
    for m in Ms:
        if (m + flip) % 2 == 0 or m == N:
            s = int(rng.integers(0, N - m + 1))
            slots.append(np.arange(s, s + m))
        else:
            slots.append(np.sort(rng.choice(N, size=m, replace=False)))
    off = np.zeros(F + 1, np.int32)
    off[1:] = np.cumsum(Ms)
    cams = np.concatenate(slots).astype(np.int32)
    z = np.empty((len(cams), 4))
    for f in range(F):
        for r in range(off[f], off[f + 1]):
            c = cams[r]
            R0 = cam_R[c]
            pc0 = R0 @ (L[f] - base.cam_p[c])
            R1 = Rcc @ R0
            pc1 = R1 @ (L[f] - (base.cam_p[c] - R1.T @ tcc))
            z[r] = [pc0[0] / pc0[2], pc0[1] / pc0[2], pc1[0] / pc1[2], pc1[1] / pc1[2]]
    z += (0.5 / 458.654) * rng.standard_normal(z.shape)
    pr = copy.copy(base)
    pr.F, pr.landmarks, pr.obs_off, pr.obs_cam, pr.obs_z = F, L, off, cams, z
    pr.flip = int(flip)
    return pr


def is_gapped(pr):
    """Per feature: the cam slots are not one contiguous window."""
    out = np.zeros(pr.F, bool)
    for f in range(pr.F):
        c = np.sort(pr.obs_cam[pr.obs_off[f]:pr.obs_off[f + 1]])
        out[f] = bool((np.diff(c) != 1).any())
    return out


def scrambled(pr, seed=0):
    """The same problem with the observations of every gapped track permuted
    (never the identity) and every contiguous track reversed (obs_cam and obs_z
    rows together)."""
    rng = np.random.default_rng([int(seed), 4711])
    out = copy.copy(pr)
    out.obs_cam, out.obs_z = pr.obs_cam.copy(), pr.obs_z.copy()
    gap = is_gapped(pr)
    for f in range(pr.F):
        a, b = int(pr.obs_off[f]), int(pr.obs_off[f + 1])
        perm = rng.permutation(b - a) if gap[f] else np.arange(b - a)[::-1]
        if (perm == np.arange(b - a)).all():   # a short track drew the identity
            perm = perm[::-1]
        perm = a + perm
        out.obs_cam[a:b] = pr.obs_cam[perm]
        out.obs_z[a:b] = pr.obs_z[perm]
    return out


def state_arrays(st):
    return st.P, np.stack([c.p for c in st.cams.values()]), st.imu.p.copy()


def sweep_reference(pr):
    """The oracle, once per feature (triangulate, feature_jacobian,
    gating_gamma), the thresholds chi2 = gamma_ref x (0.5 or 2: a fixed 2 x
    margin on either side, alternating with M // 2 + flip) with the decisions
    they imply, and the oracle's post-update state on those decisions."""
    d = problem_to_dict(pr)
    st = oracle_state_from_arrays(d)
    F, flip = pr.F, pr.flip
    M = pr.track_lengths().astype(int)
    tri_p, tri_ok, gam = np.zeros((F, 3)), np.zeros(F, bool), np.full(F, np.nan)
    for f in range(F):
        obs = feature_obs(d, f)
        p, ok, _ = O.triangulate(OrderedDict(obs), st.cams, st.R_cam0_cam1, st.t_cam0_cam1)
        tri_p[f], tri_ok[f] = p, ok
        if ok:
            H, r = O.feature_jacobian(st, p, obs)
            gam[f] = O.gating_gamma(st, H, r)
    factor = np.where((M // 2 + flip) % 2 == 1, 0.5, 2.0)
    chi2 = gam * factor
    acc = tri_ok & (gam < chi2)
    st_u = oracle_update(d, tri=(tri_p, tri_ok), accept=acc)[0]
    P, cam_p, imu_p = state_arrays(st_u)
    return SweepRef(M=M, route=np.array([route_of(m) for m in M]), gapped=is_gapped(pr), tri_p=tri_p, tri_ok=tri_ok,
                    gamma=gam, chi2=chi2, acc=acc, rows=int((4 * M[acc] - 3).sum()), P=P, cam_p=cam_p, imu_p=imu_p,
                    cam_p0=np.asarray(d["cam_p"], float), imu_p0=np.asarray(d["imu_p"], float))


# The pinned sweeps: window N -> seed of filter 0 (flip 0); filter 1 is seed + 1,
# flip 1.  test_track_sweep_ref.py checks the builder conditions on them.
SWEEP_SEEDS = {128: 900, 32: 920}


@functools.lru_cache(maxsize=None)
def cached_sweep(N, seed, flip):
    """(problem, reference) computed once per process and shared by every test
    that needs it; callers must not modify either."""
    pr = sweep_problem(N, seed, flip)
    return pr, sweep_reference(pr)


def got_from_ref(ref):
    """A device result that equals the reference (the comparator's self-test)."""
    return dict(valid=ref.tri_ok.copy(), p_w=ref.tri_p.copy(), gamma=ref.gamma.copy(), accept=ref.acc.copy(),
                rows=ref.rows, P=ref.P.copy(), cam_p=ref.cam_p.copy(), imu_p=ref.imu_p.copy())


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, float) - b) / max(np.linalg.norm(b), 1e-300)


def gamma_errors(ref, got):
    """(relative gamma error per feature, mask of the features valid in both)."""
    both = np.asarray(got["valid"], bool) & ref.tri_ok
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got["gamma"], float) - ref.gamma) / np.abs(ref.gamma)
    return e, both


def route_worst(ref, got):
    """{route index: worst relative gamma error} over the features valid in both."""
    e, both = gamma_errors(ref, got)
    return {int(r): float(e[both & (ref.route == r)].max()) for r in np.unique(ref.route[both])}


def check_sweep(ref, got, dtype, label="", state=None):
    """The whole comparison of one filter's device results with its reference.

    ``ref``: SweepRef.  ``got``: dict with valid, p_w, gamma, accept (per
    feature), rows, P, cam_p, imu_p.  ``state`` = (P, cam_p, imu_p, cam_p0,
    imu_p0) replaces the reference's post- and pre-update state (fp32: the
    oracle rerun on the device's own decisions from the rounded problem).

    fp64: valid == tri_ok; p_w rtol 1e-9 / atol 1e-10; gamma rtol 1e-9 for every
    feature; accept == acc; rows == sum(4M - 3) over accepted; rel(P) < 1e-9,
    P symmetric; cam / IMU positions atol 1e-10.
    fp32: at most one feature whose valid differs (left out of the gamma
    checks); p_w rtol 2e-3 / atol 1e-4; every gamma finite; relative gamma
    error median < 1e-4 and p99 < 1e-3 over the filter, median < 1e-4 per gate
    route, every feature below FP32_GAMMA_CAP; accept == acc where valid in
    both; rows == sum(4M - 3) over the device's accepted valid features;
    rel(P) < 1e-5, P symmetric; cam / IMU position corrections < 1e-4 relative.
    Returns a dict of the measured figures."""
    dtype = np.dtype(dtype)
    valid, acc = np.asarray(got["valid"], bool), np.asarray(got["accept"], bool)
    gam, pw = np.asarray(got["gamma"], float), np.asarray(got["p_w"], float)
    F = len(ref.M)
    assert valid.shape == (F,) and acc.shape == (F,) and gam.shape == (F,) and pw.shape == (F, 3), label
    P_r, cam_r, imu_r, cam0, imu0 = state if state is not None else (ref.P, ref.cam_p, ref.imu_p, ref.cam_p0,
                                                                    ref.imu_p0)
    P = np.asarray(got["P"], float)
    e, both = gamma_errors(ref, got)
    out = dict(rel_P=_rel(P, P_r), route_worst=route_worst(ref, got))
    if dtype == np.float64:
        np.testing.assert_array_equal(valid, ref.tri_ok, err_msg=label)
        np.testing.assert_allclose(pw[both], ref.tri_p[both], rtol=1e-9, atol=1e-10, err_msg=label)
        np.testing.assert_allclose(gam[both], ref.gamma[both], rtol=1e-9, err_msg=label)
        np.testing.assert_array_equal(acc, ref.acc, err_msg=label)
        assert int(got["rows"]) == ref.rows, (label, int(got["rows"]), ref.rows)
        assert out["rel_P"] < 1e-9, (label, out["rel_P"])
        np.testing.assert_array_equal(P, P.T, err_msg=label)
        np.testing.assert_allclose(got["cam_p"], cam_r, atol=1e-10, err_msg=label)
        np.testing.assert_allclose(got["imu_p"], imu_r, atol=1e-10, err_msg=label)
        return out
    assert int((valid != ref.tri_ok).sum()) <= 1, (label, np.flatnonzero(valid != ref.tri_ok))
    np.testing.assert_allclose(pw[both], ref.tri_p[both], rtol=2e-3, atol=1e-4, err_msg=label)
    assert np.isfinite(gam[valid]).all(), label
    eb = e[both]
    out.update(gamma_median=float(np.median(eb)), gamma_p99=float(np.quantile(eb, 0.99)), gamma_max=float(eb.max()))
    assert out["gamma_median"] < 1e-4, (label, out["gamma_median"])
    assert out["gamma_p99"] < 1e-3, (label, out["gamma_p99"])
    for r in np.unique(ref.route[both]):
        med = float(np.median(e[both & (ref.route == r)]))
        assert med < 1e-4, (label, "route %s" % route_name(r), med)
    worst = int(np.argmax(np.where(both, e, 0.0)))
    assert eb.max() < FP32_GAMMA_CAP, (label, "M = %d" % ref.M[worst], float(eb.max()))
    np.testing.assert_array_equal(acc[both], ref.acc[both], err_msg=label)
    assert not acc[~valid].any(), label
    rows = int((4 * ref.M[acc & valid] - 3).sum())
    assert int(got["rows"]) == rows, (label, int(got["rows"]), rows)
    assert out["rel_P"] < 1e-5, (label, out["rel_P"])
    np.testing.assert_array_equal(P, P.T, err_msg=label)
    out["rel_dcam"] = _rel(np.asarray(got["cam_p"], float) - cam0, cam_r - cam0)
    out["rel_dimu"] = _rel(np.asarray(got["imu_p"], float) - imu0, imu_r - imu0)
    assert out["rel_dcam"] < 1e-4, (label, out["rel_dcam"])
    assert out["rel_dimu"] < 1e-4, (label, out["rel_dimu"])
    return out
