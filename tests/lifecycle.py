"""The filter window's grow / shrink life cycle: the reference driver.

The Kalman and assembly kernels are chosen by the context's cam CAPACITY
(launch_kalman_chol, launch_gchol, the k_info variants), while the live window
C_b = 6 n_cams of a filter grows by one clone per frame and shrinks by prunes:
far below the capacity, over whatever an earlier, larger update left in P past
D and in the workspaces.  This module drives a context through such a life
cycle and compares it with the oracle STEP BY STEP: before every operation the
state is read from the context (get_state), the oracle state is built from
exactly those values (an fp32 context reads back the fp32 values it holds),
the oracle applies the one operation, the context applies it, and the two are
compared.  Nothing accumulates, so the project's per-operation tolerances hold
unchanged at every step.

Pure numpy + the oracle (no GPU import).  ``OracleContext`` puts the oracle
behind the Context methods the driver uses: test_lifecycle_ref.py runs every
script on it to pin the driver's conditions on the CPU, and runs subtly wrong
variants of it to show that every check_* fails on a subtly wrong device.
test_gpu_lifecycle.py runs the same scripts on the HIP path.

Tolerances (the project's own, per operation):
  prune      P, cam records, n_cams and the IMU record bit-equal to
             P[np.ix_(keep, keep)] / cams[keep], both dtypes.
  augment    fp64 rel(P) < 1e-14, new cam record atol 1e-15, P == P.T exactly
             (test_augment_golden); fp32 rel(P) < 1e-5 (21-term fp32 dot
             products: the project's fp32 propagation bound), P == P.T exactly,
             new cam record atol 4e-6 (32 fp32 roundings of O(1) values: a 3 x 3
             rotation product, the quaternion's square root and division, the
             lever arm added to a position of a few metres).
  propagate  fp64 1e-12, fp32 1e-5 on P, q, v, p (test_propagate_batch_vs_oracle);
             an empty sample range leaves the filter bit-unchanged.
  update     fp64: valid, accept, rows equal; gamma rtol 1e-9; rel(P) < 1e-9;
             P == P.T; cam and IMU positions atol 1e-10.  fp32: valid, accept and
             rows equal (thresholds at 2 x / 0.5 x the oracle's gamma), then the
             oracle rerun on the device's own positions and decisions with the
             fp32 sigma2 and the observations rounded to fp32, as the context
             holds them (check_fp32_batch, part 2): rel(P) < 1e-5, P == P.T,
             position corrections < 1e-4 relative.
"""
from collections import OrderedDict, namedtuple

import numpy as np

from helpers import oracle_state_from_arrays, oracle_state_from_device
from oracle import msckf_oracle as O
from msckf_amd import synth, FilterConfig
from msckf_amd._lib import CAM_LEN, IMU_LEN, pack_cams, pack_imu, unpack_imu

State = namedtuple("State", "imu cams P")          # what Context.get_state returns
Obs = namedtuple("Obs", "off cam z")               # one filter's features: offsets, cam slots, (u0, v0, u1, v1)
UpdateRef = namedtuple("UpdateRef", "tri_p tri_ok gamma chi2 acc rows M")

SIGMA2 = FilterConfig().observation_noise
PIX_SIGMA = 0.5 / 458.654                         # synth.make_update_problem's pixel noise
MAX_TRACK = 12
FP32_CAM_ATOL = 4e-6

# The pinned scripts: capacity -> seed of filter 0 (filter b: seed + b).
# test_lifecycle_ref.py checks the driver's conditions for them on the oracle.
WINDOW_CAPS = (21, 32, 34, 52)
LIFECYCLE_SEEDS = {21: 2100, 32: 3200, 34: 3410, 52: 5200, 128: 12856}
WINDOW_FEATURES, CAP128_FEATURES = 24, 12
# Growth targets of filter 0 (step 7), as live cam counts n with C_b = 6 n:
#   register-tile windows (cap <= 32): 30 | 36 lie on either side of the 16-column
#     tile edge 32 (2 | 3 tiles of k_kal_b / k_kal_c2); 30 % 4 == 2.
#   global-memory windows (cap > 32): 60 | 66 lie on either side of 64, which is
#     both a 16-column tile edge and the GNB = 64 pivot panel / GT = 64 tile edge of
#     k_gchol_* (one short panel | one full panel and a 2-pivot one); 66 % 4 == 2.
GROWTH = {21: (5, 6), 32: (5, 6), 34: (10, 11), 52: (10, 11)}


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _maxabs(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max()) if a.size else 0.0


# ------------------------------------------------------------- oracle glue --

def oracle_of(state, sigma2=SIGMA2):
    """Oracle FilterState of one get_state() result, null-space fields included."""
    st = oracle_state_from_device(state.imu, state.cams, state.P, sigma2=sigma2)
    s = unpack_imu(np.asarray(state.imu))
    st.imu.nulls_alias, st.imu.p_null, st.imu.v_null = s["alias"], s["p_null"], s["v_null"]
    st.imu.timestamp = 0.0
    return st


def record_of(st):
    """get_state() form of an oracle state."""
    i = st.imu
    imu = pack_imu(q=i.q, p=i.p, v=i.v, bg=i.bg, ba=i.ba, q_null=i.q_null,
                   p_null=i.p if i.nulls_alias else i.p_null, v_null=i.v if i.nulls_alias else i.v_null,
                   R_imu_cam0=i.R_imu_cam0, t_cam0_imu=i.t_cam0_imu, gravity=st.gravity, alias=i.nulls_alias)
    cams = np.zeros((len(st.cams), CAM_LEN))
    for k, c in enumerate(st.cams.values()):
        cams[k] = np.concatenate([c.q, c.p, c.q_null])
    return State(imu, cams, st.P.copy())


def start_state(cap, seed, F):
    """(State, landmarks): cams and P of synth.make_update_problem(cap, F, seed),
    the IMU pose replaced so that a clone made by augment continues the cam
    track -- cam0 centre 0.05 m further along x than the last cam, orientation
    within ~0.02 rad of the track's (with the problem's own IMU pose the EuRoC
    extrinsics make the clone look away from the landmarks).

    The world origin is moved to the last cam (one translation of cams and
    landmarks alike: the problem is the same).  The track runs 0.05 m per cam
    along x, so at 52 cams the IMU would sit 2.6 m out, where an fp32 context
    holds a position to 1.2e-7 (half an ulp): 1.7e-4 of the ~1 mm IMU position
    corrections these updates make, above the 1e-4 bound they are held to.
    With the origin at the growing end, the IMU and the new clones sit within
    ~0.1 m of it and their stored positions are exact to ~4e-9."""
    pr = synth.make_update_problem(cap, F, seed)
    origin = pr.cam_p[-1].copy()
    pr.cam_p = pr.cam_p - origin
    pr.landmarks = pr.landmarks - origin
    rng = np.random.default_rng([int(seed), int(cap), 1707])
    R_wc = O.to_rotation(O.small_angle_quaternion(0.01 * rng.standard_normal(3)))
    p_c = pr.cam_p[-1] + np.array([0.05, 0.0, 0.0]) + 0.005 * rng.standard_normal(3)
    imu = dict(pr.imu)
    R_wi = imu["R_imu_cam0"].T @ R_wc
    imu["q"] = O.to_quaternion(R_wi)
    imu["p"] = p_c - R_wi.T @ imu["t_cam0_imu"]
    imu["q_null"] = imu["q"].copy()
    rec = pack_imu(gravity=pr.gravity, alias=True, **{**imu, "p_null": imu["p"], "v_null": imu["v"]})
    return State(rec, pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P.copy()), pr.landmarks.copy()


def make_samples(state, n, key, dt=0.02):
    """n IMU samples (dt, gyro, acc) for a filter at rest in ``state``: the
    accelerometer reads minus gravity in the IMU frame, plus the biases and
    noise, so the clone stays on the cam track."""
    rng = np.random.default_rng([int(k) for k in key])
    s = unpack_imu(np.asarray(state.imu))
    R_wi = O.to_rotation(s["q"])
    gyro = s["bg"] + 0.3 * rng.standard_normal((n, 3))
    acc = R_wi @ (-s["gravity"]) + s["ba"] + 0.3 * rng.standard_normal((n, 3))
    return np.full(n, dt), gyro, acc


def make_observations(st, landmarks, key):
    """The features of one filter for its current live cams: the ground-truth
    landmarks projected into the oracle state's cams (both cameras of the
    stereo pair) plus the synth pixel noise.  Tracks are contiguous runs of
    2 .. min(n, 12) live slots; every third feature ends at the newest slot.
    Fewer than 2 cams: no features."""
    n, F = len(st.cams), len(landmarks)
    if n < 2:
        return Obs(np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 4)))
    rng = np.random.default_rng([int(k) for k in key])
    cams = list(st.cams.values())
    M = rng.integers(2, min(n, MAX_TRACK) + 1, size=F)
    start = np.array([n - m if f % 3 == 0 else rng.integers(0, n - m + 1) for f, m in enumerate(M)])
    off = np.zeros(F + 1, np.int32)
    off[1:] = np.cumsum(M)
    slot = np.concatenate([np.arange(s, s + m) for s, m in zip(start, M)]).astype(np.int32)
    z = np.empty((len(slot), 4))
    for f in range(F):
        for r in range(off[f], off[f + 1]):
            c = cams[slot[r]]
            R0 = O.to_rotation(c.q)
            pc0 = R0 @ (landmarks[f] - c.p)
            R1 = st.R_cam0_cam1 @ R0
            pc1 = R1 @ (landmarks[f] - (c.p - R1.T @ st.t_cam0_cam1))
            z[r] = [pc0[0] / pc0[2], pc0[1] / pc0[2], pc1[0] / pc1[2], pc1[1] / pc1[2]]
    z += PIX_SIGMA * rng.standard_normal(z.shape)
    return Obs(off, slot, z)


def _feature(obs, f):
    a, b = int(obs.off[f]), int(obs.off[f + 1])
    return [(int(c), obs.z[r]) for r, c in zip(range(a, b), obs.cam[a:b])]


def gate_features(st, obs):
    """The oracle per feature: (positions, valid, gamma; NaN where invalid)."""
    F = len(obs.off) - 1
    tri_p, tri_ok, gam = np.zeros((F, 3)), np.zeros(F, bool), np.full(F, np.nan)
    for f in range(F):
        o = _feature(obs, f)
        p, ok, _ = O.triangulate(OrderedDict(o), st.cams, st.R_cam0_cam1, st.t_cam0_cam1)
        tri_p[f], tri_ok[f] = p, ok
        if ok:
            H, r = O.feature_jacobian(st, p, o)
            gam[f] = O.gating_gamma(st, H, r)
    return tri_p, tri_ok, gam


def apply_update(st, obs, tri_p, take):
    """The oracle's EKF update of ``st`` (in place) with the features ``take``
    at the positions ``tri_p``."""
    Hs, rs = [], []
    for f in np.flatnonzero(take):
        H, r = O.feature_jacobian(st, np.asarray(tri_p[f], float), _feature(obs, f))
        Hs.append(H)
        rs.append(r)
    if Hs:
        O.measurement_update(st, np.vstack(Hs), np.concatenate(rs))
    return st


def update_reference(st, obs, flip):
    """Oracle gamma per feature and the thresholds chi2 = gamma x (2 or 0.5,
    alternating with the feature index + flip: a 2 x margin either way, so the
    decisions must be the same in fp32) with the decisions they imply."""
    tri_p, tri_ok, gam = gate_features(st, obs)
    F = len(gam)
    M = np.diff(obs.off).astype(int)
    factor = np.where((np.arange(F) + flip) % 2 == 0, 2.0, 0.5)
    chi2 = np.where(tri_ok, gam * factor, 1.0)
    acc = tri_ok & (gam < chi2)
    return UpdateRef(tri_p, tri_ok, gam, chi2, acc, int((4 * M[acc] - 3).sum()), M)


def prune_reference(P, cams, rm):
    """(P[np.ix_(keep, keep)], cams[keep], kept slots) for the removed slots rm
    (any order, repeats allowed)."""
    n = len(cams)
    keep = [c for c in range(n) if c not in set(int(s) for s in rm)]
    idx = np.concatenate([np.arange(21)] + [21 + 6 * c + np.arange(6) for c in keep]).astype(int)
    return P[np.ix_(idx, idx)].copy(), np.asarray(cams)[keep].copy(), keep


# ---------------------------------------------------------------- checkers --

def _assert_state_equal(a, b, label):
    np.testing.assert_array_equal(a.imu, b.imu, err_msg=label)
    np.testing.assert_array_equal(a.cams, b.cams, err_msg=label)
    np.testing.assert_array_equal(a.P, b.P, err_msg=label)


def check_prune(before, rm, after, label=""):
    P_ref, cams_ref, keep = prune_reference(before.P, before.cams, rm)
    dev = max(_maxabs(after.P, P_ref) if after.P.shape == P_ref.shape else np.inf,
              _maxabs(after.cams, cams_ref) if after.cams.shape == cams_ref.shape else np.inf)
    print("%s prune %d -> %d cams: max |diff| %.3e" % (label, len(before.cams), len(keep), dev))
    assert len(after.cams) == len(keep), (label, len(after.cams), len(keep))
    np.testing.assert_array_equal(after.P, P_ref, err_msg=label)
    np.testing.assert_array_equal(after.cams, cams_ref, err_msg=label)
    np.testing.assert_array_equal(after.imu, before.imu, err_msg=label)
    return dev


def check_augment(before, after, dtype, label=""):
    n = len(before.cams)
    st = oracle_of(before)
    O.state_augmentation(st, float(n), n)
    ref = record_of(st)
    assert len(after.cams) == n + 1, (label, len(after.cams))
    e_P, e_cam = _rel(after.P, ref.P), _maxabs(after.cams[n], ref.cams[n])
    print("%s augment %d -> %d cams: rel(P) %.3e, new cam record %.3e" % (label, n, n + 1, e_P, e_cam))
    fp64 = np.dtype(dtype) == np.float64
    assert e_P < (1e-14 if fp64 else 1e-5), (label, e_P)
    np.testing.assert_array_equal(after.P, after.P.T, err_msg=label)
    np.testing.assert_allclose(after.cams[n], ref.cams[n], rtol=0, atol=1e-15 if fp64 else FP32_CAM_ATOL, err_msg=label)
    np.testing.assert_array_equal(after.cams[n, 7:11], after.cams[n, 0:4], err_msg=label)   # q_null is the clone's q
    np.testing.assert_array_equal(after.cams[:n], before.cams, err_msg=label)
    np.testing.assert_array_equal(after.imu, before.imu, err_msg=label)
    return e_P


def propagate_oracle(st, dt, gyro, acc):
    """The oracle's process_model, once per sample, on ``st`` (in place)."""
    st.imu.timestamp = 0.0
    for k in range(len(dt)):
        t_k = st.imu.timestamp + dt[k]
        O.process_model(st, t_k, gyro[k], acc[k])
        st.imu.timestamp = t_k
    return st


def compare_propagated(st, imu, P, dtype, label=""):
    """The comparison of test_propagate_batch_vs_oracle: P <= tol relative and
    symmetric, q / v / p <= tol x max(1, |.|), tol = 1e-12 (fp64) / 1e-5 (fp32)."""
    tol = 1e-12 if np.dtype(dtype) == np.float64 else 1e-5
    s = unpack_imu(np.asarray(imu))
    e = _rel(P, st.P)
    print("%s propagate D = %d: rel(P) %.3e" % (label, P.shape[0], e))
    assert e < tol, (label, e)
    np.testing.assert_array_equal(P, P.T, err_msg=label)
    for key, ref_v in (("q", st.imu.q), ("v", st.imu.v), ("p", st.imu.p)):
        assert np.abs(s[key] - ref_v).max() <= tol * max(1.0, np.abs(ref_v).max()), (label, key)
    return e


def check_propagate(before, dt, gyro, acc, after, dtype, label=""):
    if len(dt) == 0:
        print("%s propagate: empty sample range" % label)
        _assert_state_equal(after, before, label)
        return 0.0
    st = propagate_oracle(oracle_of(before), dt, gyro, acc)
    e = compare_propagated(st, after.imu, after.P, dtype, label)
    np.testing.assert_array_equal(after.cams, before.cams, err_msg=label)
    for a, b in ((10, 16), (26, 41)):              # bg, ba; extrinsics, gravity: untouched
        np.testing.assert_array_equal(after.imu[a:b], before.imu[a:b], err_msg=label)
    assert after.imu[41] == 1.0, label             # the null-space fields alias p / v from here on
    return e


def propagate_batch_vs_oracle(ctx, ds, counts, dtype, seed):
    """The body of test_propagate_batch_vs_oracle for any sample counts: the
    filters of ``ctx`` hold the problems ``ds`` (dicts, rounded for fp32); one
    propagate_batch launch with counts[b] samples for filter b, against the
    oracle's per-sample process_model.  Returns [(oracle state, imu, cams, P)]."""
    B, total = len(ds), int(sum(counts))
    rng = np.random.default_rng(seed)
    dt = np.full(total, 0.005)
    gyro = 0.3 * rng.standard_normal((total, 3))
    acc = rng.standard_normal((total, 3)) + np.array([0.0, 0.0, 9.81])
    if np.dtype(dtype) == np.float32:
        gyro, acc = gyro.astype(np.float32).astype(float), acc.astype(np.float32).astype(float)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    ctx.propagate_batch(list(range(B)), off, dt, gyro, acc)
    out = []
    for b, d in enumerate(ds):
        st = oracle_state_from_arrays(d)
        st.imu.nulls_alias = True
        sl = slice(off[b], off[b + 1])
        propagate_oracle(st, dt[sl], gyro[sl], acc[sl])
        imu, cams, P = ctx.get_state(b)
        compare_propagated(st, imu, P, dtype, "[N=%d %s filter %d, %d samples]" % (int(d["N"]), np.dtype(dtype).name, b, counts[b]))
        out.append((st, imu, cams, P))
    return out


def check_update(before, obs, ref, got, after, dtype, label=""):
    """``got``: dict(valid, accept, gamma, p_w, rows) of this filter's features."""
    valid, acc = np.asarray(got["valid"], bool), np.asarray(got["accept"], bool)
    gam = np.asarray(got["gamma"], float)
    F = len(ref.M)
    assert valid.shape == (F,) and acc.shape == (F,) and gam.shape == (F,), label
    fp64 = np.dtype(dtype) == np.float64
    ok = ref.tri_ok & valid
    e_g = float(np.abs(gam[ok] / ref.gamma[ok] - 1).max()) if ok.any() else 0.0
    if F == 0:
        print("%s update C_b = %d: no features" % (label, 6 * len(before.cams)))
        assert int(got["rows"]) == 0, (label, got["rows"])
        _assert_state_equal(after, before, label)
        return dict(rel_P=0.0, gamma=0.0)
    if fp64:
        st = apply_update(oracle_of(before), obs, ref.tri_p, ref.acc)
    else:   # the oracle on the device's own positions and decisions, fp32 sigma2
        st = apply_update(oracle_of(before, sigma2=float(np.float32(SIGMA2))), obs, got["p_w"], acc & valid)
    r = record_of(st)
    out = dict(rel_P=_rel(after.P, r.P), gamma=e_g)
    d_cam, d_imu = after.cams[:, 4:7] - before.cams[:, 4:7], after.imu[4:7] - before.imu[4:7]
    out["rel_dcam"] = _rel(d_cam, r.cams[:, 4:7] - before.cams[:, 4:7])
    out["rel_dimu"] = _rel(d_imu, r.imu[4:7] - before.imu[4:7])
    out["abs_p"] = max(_maxabs(after.cams[:, 4:7], r.cams[:, 4:7]), _maxabs(after.imu[4:7], r.imu[4:7]))
    print("%s update C_b = %d, %d features (%d valid, %d accepted, %d rows): rel(P) %.3e, gamma %.3e, "
          "positions %.3e, corrections cam %.3e imu %.3e"
          % (label, 6 * len(before.cams), F, int(valid.sum()), int(acc.sum()), int(got["rows"]), out["rel_P"], e_g,
             out["abs_p"], out["rel_dcam"], out["rel_dimu"]))
    np.testing.assert_array_equal(valid, ref.tri_ok, err_msg=label)
    np.testing.assert_array_equal(acc, ref.acc, err_msg=label)
    assert int(got["rows"]) == ref.rows, (label, int(got["rows"]), ref.rows)
    assert len(after.cams) == len(before.cams), label
    if fp64:
        np.testing.assert_allclose(gam[ok], ref.gamma[ok], rtol=1e-9, err_msg=label)
        assert out["rel_P"] < 1e-9, (label, out["rel_P"])
        np.testing.assert_array_equal(after.P, after.P.T, err_msg=label)
        np.testing.assert_allclose(after.cams[:, 4:7], r.cams[:, 4:7], rtol=0, atol=1e-10, err_msg=label)
        np.testing.assert_allclose(after.imu[4:7], r.imu[4:7], rtol=0, atol=1e-10, err_msg=label)
    else:
        assert np.isfinite(gam[valid]).all(), label
        assert out["rel_P"] < 1e-5, (label, out["rel_P"])
        np.testing.assert_array_equal(after.P, after.P.T, err_msg=label)
        assert out["rel_dcam"] < 1e-4, (label, out["rel_dcam"])
        assert out["rel_dimu"] < 1e-4, (label, out["rel_dimu"])
    return out


def check_readback(ctx, B, label=""):
    """cov_diag_batch and readback(cov=...) against get_state: the diagonal
    range every filter has, each filter's whole diagonal, the IMU and cam
    records, in a filter order that is not a run of consecutive slots."""
    order = list(range(B))[::-1] if B < 3 else [2, 0, 1] + list(range(3, B))
    states = [State(*ctx.get_state(b)) for b in range(B)]
    n = min(s.P.shape[0] for s in states)
    diag = ctx.cov_diag_batch(order, 0, n)
    imu, cl, cv = ctx.readback(order, cov=(0, n))
    tail = ctx.cov_diag_batch(order, n - 6, 6)
    for w, b in enumerate(order):
        s = states[b]
        np.testing.assert_array_equal(diag[w], np.diag(s.P)[:n], err_msg=label)
        np.testing.assert_array_equal(cv[w], np.diag(s.P)[:n], err_msg=label)
        np.testing.assert_array_equal(tail[w], np.diag(s.P)[n - 6:n], err_msg=label)
        np.testing.assert_array_equal(imu[w], s.imu, err_msg=label)
        np.testing.assert_array_equal(cl[w], s.cams, err_msg=label)
        D = s.P.shape[0]
        np.testing.assert_array_equal(ctx.cov_diag_batch([b], 0, D)[0], np.diag(s.P), err_msg=label)
    print("%s readback: diagonals [0, %d) and records of filters %s equal get_state" % (label, n, order))
    return states


# ------------------------------------------------------------------ driver --

class Lifecycle:
    """Drives ``ctx`` (a Context, or an OracleContext) through single steps,
    each compared with the oracle, and keeps the figures:
    ``worst[op]`` the largest deviation per operation, ``updates`` one record
    per update step ([(n_cams, UpdateRef, Obs)] per filter)."""

    def __init__(self, ctx, cap, dtype, B, F, seed, name=""):
        self.ctx, self.cap, self.dtype, self.B, self.F, self.seed = ctx, cap, np.dtype(dtype), B, F, seed
        self.name = name or "cap %d %s" % (cap, self.dtype.name)
        self.worst, self.updates, self.step = {}, [], 0
        self.landmarks = []
        for b in range(B):
            s, L = start_state(cap, seed + b, F)
            ctx.set_state(b, s.imu, s.cams, s.P)
            self.landmarks.append(L)

    def state(self, b):
        return State(*self.ctx.get_state(b))

    def _note(self, op, e):
        self.worst[op] = max(self.worst.get(op, 0.0), float(e))

    def _label(self, b):
        return "[%s step %d filter %d]" % (self.name, self.step, b)

    def prune(self, rm):
        """rm = {filter: slots to remove}: one prune_batch launch."""
        self.step += 1
        filters = sorted(rm)
        before = {b: self.state(b) for b in range(self.B)}
        off = np.concatenate([[0], np.cumsum([len(rm[b]) for b in filters])]).astype(int)
        self.ctx.prune_batch(filters, off, np.concatenate([np.asarray(rm[b], int) for b in filters]))
        for b in range(self.B):
            if b in rm:
                self._note("prune", check_prune(before[b], rm[b], self.state(b), self._label(b)))
            else:
                _assert_state_equal(self.state(b), before[b], self._label(b))

    def propagate(self, counts):
        """counts = {filter: samples}: one propagate_batch launch (a count of 0
        is an empty range in the launch)."""
        self.step += 1
        filters = sorted(counts)
        before = {b: self.state(b) for b in range(self.B)}
        smp = {b: make_samples(before[b], counts[b], (self.seed, self.step, b)) for b in filters}
        off = np.concatenate([[0], np.cumsum([counts[b] for b in filters])]).astype(int)
        dt, gyro, acc = (np.concatenate([smp[b][k] for b in filters]) for k in range(3))
        if self.dtype == np.float32:   # the samples as the context holds them
            dt, gyro, acc = (a.astype(np.float32).astype(float) for a in (dt, gyro, acc))
        self.ctx.propagate_batch(filters, off, dt, gyro, acc)
        for b in range(self.B):
            if b in counts:
                sl = slice(off[filters.index(b)], off[filters.index(b) + 1])
                e = check_propagate(before[b], dt[sl], gyro[sl], acc[sl], self.state(b), self.dtype, self._label(b))
                self._note("propagate", e)
            else:
                _assert_state_equal(self.state(b), before[b], self._label(b))

    def augment(self, filters):
        self.step += 1
        before = {b: self.state(b) for b in range(self.B)}
        self.ctx.augment_batch(list(filters))
        for b in range(self.B):
            if b in filters:
                self._note("augment", check_augment(before[b], self.state(b), self.dtype, self._label(b)))
            else:
                _assert_state_equal(self.state(b), before[b], self._label(b))

    def update(self):
        """One batched update of all filters on freshly generated features."""
        self.step += 1
        before = [self.state(b) for b in range(self.B)]
        obs, refs = [], []
        for b in range(self.B):
            st = oracle_of(before[b])
            o = make_observations(st, self.landmarks[b], (self.seed, self.step, b))
            if self.dtype == np.float32:   # the observations as the context holds them
                o = o._replace(z=o.z.astype(np.float32).astype(float))
            obs.append(o)
            refs.append(update_reference(st, o, self.step + b))
        feat_off = np.concatenate([[0], np.cumsum([len(o.off) - 1 for o in obs])]).astype(int)
        obs_off = [0]
        for o in obs:
            obs_off.extend(list(obs_off[-1] + o.off[1:]))
        self.ctx.batch_load(feat_off, obs_off, np.concatenate([o.cam for o in obs]),
                            np.concatenate([o.z for o in obs]), None, np.concatenate([r.chi2 for r in refs]))
        self.ctx.batch_update(row_cap=0, triangulate=True)
        acc, gam, pw, valid, rows = self.ctx.batch_results()
        rec = []
        for b in range(self.B):
            sl = slice(feat_off[b], feat_off[b + 1])
            got = dict(valid=valid[sl], accept=acc[sl], gamma=gam[sl], p_w=pw[sl], rows=int(rows[b]))
            out = check_update(before[b], obs[b], refs[b], got, self.state(b), self.dtype, self._label(b))
            self._note("update", out["rel_P"])
            self._note("update gamma", out["gamma"])
            self._note("corrections", max(out.get("rel_dcam", 0.0), out.get("rel_dimu", 0.0)))
            rec.append((len(before[b].cams), refs[b], obs[b]))
        self.updates.append(rec)

    def readback(self):
        self.step += 1
        check_readback(self.ctx, self.B, "[%s step %d]" % (self.name, self.step))

    def grow(self, b, n, samples=4):
        """Propagate + augment filter b until it holds n cams (a clone needs
        process noise between itself and the one before, or P_cc is singular)."""
        while len(self.ctx.get_state(b, want_P=False)[1]) < n:
            self.propagate({b: samples})
            self.augment([b])


def window_script(lc):
    """Steps 1 - 8 of the window life cycle on three filters of capacity cap."""
    cap = lc.cap
    lc.update()                                              # 1 full window: fills P and every workspace
    lc.prune({0: list(range(1, cap - 1)),                    # 2 filter 0 down to slots {0, last}
              1: list(range(0, cap, 2)),                     #   filter 1 keeps the odd slots
              2: [0]})                                       #   filter 2 drops slot 0 only
    lc.propagate({0: 5, 1: 0, 2: 1})                         # 3 an empty range in the launch
    lc.augment([0, 2])                                       # 4 filter 1 not listed
    lc.update()                                              # 5 live windows 3, cap // 2, cap in one launch
    lc.readback()                                            # 6
    for n in GROWTH[cap]:                                    # 7 C_b on both sides of a tile / panel edge
        lc.grow(0, n)
        lc.update()
    lc.prune({1: list(range(1, cap // 2))})                  # 8 filter 1 down to one cam: no features
    lc.update()
    return lc


def cap128_slots(seed):
    """The 40 scattered slots filter 0 of the cap-128 script keeps."""
    return np.sort(np.random.default_rng([int(seed), 128, 40]).choice(128, size=40, replace=False))


def cap128_script(lc):
    """Full update, prune to 40 scattered slots, propagate 3 samples, augment,
    update: D = 789 -> 261 -> 267 in ld = 789."""
    keep = set(int(s) for s in cap128_slots(lc.seed))
    lc.update()
    lc.prune({0: [s for s in range(128) if s not in keep]})
    lc.propagate({0: 3})
    lc.augment([0])
    lc.update()
    return lc


# ----------------------------------------------------------- oracle device --

class OracleContext:
    """The oracle behind the Context methods the driver uses (state kept in
    get_state form, rounded to ``dtype`` after every operation as an fp32
    context stores it).  ``wrong`` names one subtle defect to build in -- the
    kind of error a kernel that mishandles a partial window or stale memory
    would make -- for the tests that show each check_* fails on it."""

    def __init__(self, cfg=None, n_filters=1, n_cam_capacity=32, dtype=np.float64, wrong=None):
        self.B, self.Nmax, self.dtype, self.wrong = n_filters, n_cam_capacity, np.dtype(dtype), wrong
        imu = np.zeros(IMU_LEN)
        self.s = [State(imu.copy(), np.zeros((0, CAM_LEN)), np.zeros((21, 21))) for _ in range(n_filters)]
        self.batch = None

    def _r(self, a):
        return np.asarray(a, float).astype(self.dtype).astype(float)

    def _put(self, f, state):
        self.s[f] = State(self._r(state.imu), self._r(state.cams).reshape(-1, CAM_LEN), self._r(state.P))

    def close(self):
        pass

    def set_state(self, f, imu, cams, P):
        n = 0 if cams is None else len(cams)
        if n > self.Nmax:
            raise RuntimeError("n_cams %d exceeds capacity %d" % (n, self.Nmax))
        self._put(f, State(imu, np.zeros((0, CAM_LEN)) if cams is None else cams, P))

    def get_state(self, f, want_P=True):
        s = self.s[f]
        return s.imu.copy(), s.cams.copy(), s.P.copy() if want_P else None

    def prune_batch(self, filters, slot_off, slots):
        for w, f in enumerate(filters):
            rm = [int(c) for c in slots[slot_off[w]:slot_off[w + 1]]]
            if any(c < 0 or c >= len(self.s[f].cams) for c in rm):
                raise RuntimeError("filter %d: prune slot out of range" % f)
        for w, f in enumerate(filters):
            st = oracle_of(self.s[f])
            before = self.s[f]
            O.remove_cam_cov(st, sorted(set(int(c) for c in slots[slot_off[w]:slot_off[w + 1]])))
            out = record_of(st)
            if self.wrong == "prune_rows_only" and len(out.cams) < len(before.cams):
                D = out.P.shape[0]                       # rows compacted, columns left where they were
                _, _, keep = prune_reference(before.P, before.cams, slots[slot_off[w]:slot_off[w + 1]])
                idx = np.concatenate([np.arange(21)] + [21 + 6 * c + np.arange(6) for c in keep]).astype(int)
                out = State(out.imu, out.cams, before.P[idx][:, :D].copy())
            self._put(f, out)

    def prune(self, f, slots):
        if len(slots):
            self.prune_batch([f], [0, len(slots)], list(slots))

    def propagate_batch(self, filters, sample_off, dt, gyro, acc):
        for w, f in enumerate(filters):
            sl = slice(int(sample_off[w]), int(sample_off[w + 1]))
            if sl.stop == sl.start:
                if self.wrong == "empty_range_touches":
                    s = self.s[f]
                    self._put(f, State(s.imu, s.cams, s.P * (1 + 1e-15)))
                continue
            before = self.s[f]
            st = propagate_oracle(oracle_of(before), np.asarray(dt)[sl], np.asarray(gyro)[sl], np.asarray(acc)[sl])
            out = record_of(st)
            if self.wrong == "propagate_last_columns" and len(before.cams):
                out.P[:21, -6:], out.P[-6:, :21] = before.P[:21, -6:], before.P[-6:, :21]   # the last cam's cross block
            self._put(f, out)

    def augment_batch(self, filters):
        for f in filters:
            if len(self.s[f].cams) >= self.Nmax:
                raise RuntimeError("filter %d: cam-state capacity %d exhausted" % (f, self.Nmax))
        for f in filters:
            st = oracle_of(self.s[f])
            n = len(st.cams)
            O.state_augmentation(st, float(n), n)
            out = record_of(st)
            if self.wrong == "augment_stale_corner":
                out.P[-6:, -6:] *= 1 + 1e-4               # the new diagonal block not (quite) the fresh one
            self._put(f, out)

    def augment(self, f):
        self.augment_batch([f])

    def batch_load(self, feat_off, obs_off, obs_cam, obs_z, p_w=None, chi2=None):
        self.batch = (np.asarray(feat_off, int), np.asarray(obs_off, int), np.asarray(obs_cam, int),
                      self._r(obs_z).reshape(-1, 4), np.asarray(chi2, float))
        self.res = None

    def batch_update(self, row_cap=0, triangulate=True):
        feat_off, obs_off, obs_cam, obs_z, chi2 = self.batch
        nf = int(feat_off[-1])
        acc, gam, pw, valid = np.zeros(nf, bool), np.zeros(nf), np.zeros((nf, 3)), np.zeros(nf, bool)
        rows = np.zeros(self.B, np.int32)
        s2 = SIGMA2 if self.dtype == np.float64 else float(np.float32(SIGMA2))
        for b in range(self.B):
            a, e = int(feat_off[b]), int(feat_off[b + 1])
            if e == a:
                continue
            o0 = int(obs_off[a])
            obs = Obs(obs_off[a:e + 1] - o0, obs_cam[o0:int(obs_off[e])], obs_z[o0:int(obs_off[e])])
            before = self.s[b]
            st = oracle_of(before, sigma2=s2)
            tp, ok, g = gate_features(st, obs)
            take = ok & (g < chi2[a:e])
            if self.wrong == "accept_flip":
                take[np.flatnonzero(ok)[0]] ^= True
            acc[a:e], gam[a:e], pw[a:e], valid[a:e] = take, g, tp, ok
            rows[b] = int((4 * np.diff(obs.off)[take] - 3).sum())
            out = record_of(apply_update(st, obs, tp, take))
            if self.wrong == "update_last_tile" and len(before.cams) < self.Nmax:
                out.P[-2:, -2:] = before.P[-2:, -2:]      # a partial window's last rows not updated
            if self.wrong == "update_P_1e-7":
                out.P[21:27, 21:27] *= 1 + 1e-7 * np.linalg.norm(out.P) / np.linalg.norm(out.P[21:27, 21:27])
            self._put(b, out)
        self.res = (acc, gam, pw, valid, rows)

    def batch_results(self):
        return self.res

    def cov_diag_batch(self, filters, i0, n):
        for f in filters:
            if i0 < 0 or i0 + n > self.s[f].P.shape[0]:
                raise RuntimeError("diagonal range out of bounds")
        return np.stack([np.diag(self.s[f].P)[i0:i0 + n] for f in filters])

    def readback(self, filters, want_cams=True, cov=None):
        imu = np.stack([self.s[f].imu for f in filters])
        cv = self.cov_diag_batch(filters, cov[0], cov[1]) if cov else None
        if self.wrong == "readback_order" and cv is not None:
            cv = cv[::-1]
        return imu, [self.s[f].cams.copy() for f in filters], cv
