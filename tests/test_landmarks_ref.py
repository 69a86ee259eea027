"""CPU checks of include/msckf_odometry.h: the numpy restatement
tests/landmarks_ref.py against hand-written rings, the package's host ring
against it, the covariance formula against an independent statement, and the
host logic of both landmark modes and of odometry=True on the stand-in context
(no device): MSCKF and MultiMSCKF(3)."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd
import msckf_amd.scheduler as sched_mod
from msckf_amd import _lib, synth
from msckf_amd.landmarks import HostRing, Landmarks
from msckf_amd.msckf import MSCKF, VioOdometry, VioResult
from msckf_amd.replay import FeatureStream, replay
import landmarks_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the ring --
def append_n(ring, first_id, n, stamp):
    for k in range(n):
        ring.append(first_id + k, [first_id + k, 0.5, -1.0], 3 + k % 4, 0.25 * (first_id + k), stamp)


def test_ring_wrap_at_cap_8():
    """Appends of 3, 4 and 6 rows into 8 slots, slots and seq written by hand."""
    r = lr.Ring(8)
    append_n(r, 100, 3, 0)
    assert r.seq == 3 and r.ids[:3].tolist() == [100, 101, 102]
    append_n(r, 200, 4, 1)
    assert r.seq == 7 and r.ids[:7].tolist() == [100, 101, 102, 200, 201, 202, 203]
    append_n(r, 300, 6, 2)
    assert r.seq == 13
    # appends 7..12 went to slots 7, 0, 1, 2, 3, 4
    assert r.ids.tolist() == [301, 302, 303, 304, 305, 202, 203, 300]
    assert r.stamp.tolist() == [2, 2, 2, 2, 2, 1, 1, 2]
    assert r.n_obs.tolist() == [3 + k % 4 for k in (1, 2, 3, 4, 5)] + [3 + 2, 3 + 3, 3]
    np.testing.assert_array_equal(r.gamma, 0.25 * r.ids)
    np.testing.assert_array_equal(r.p_w[:, 0], r.ids)
    ids, p_w, n_obs, gam, stamp, first, seq = r.get()
    assert (first, seq) == (5, 13) and ids.tolist() == [202, 203, 300, 301, 302, 303, 304, 305]
    assert stamp.tolist() == [1, 1, 2, 2, 2, 2, 2, 2]


def test_incremental_get():
    r = lr.Ring(8)
    append_n(r, 0, 13, 7)                       # the ring holds sequence numbers 5..12, id = sequence number
    below = r.get(2)                            # below the ring's tail: lapped, starts at 5
    assert below[5] == 5 and below[6] == 13 and below[0].tolist() == list(range(5, 13))
    inside = r.get(9)
    assert inside[5] == 9 and inside[0].tolist() == [9, 10, 11, 12]
    at_seq = r.get(13)
    assert at_seq[5] == 13 and at_seq[6] == 13 and len(at_seq[0]) == 0
    beyond = r.get(20)
    assert beyond[5] == 13 and len(beyond[0]) == 0
    few = r.get(6, max_rows=3)                  # fewer than available: the oldest three
    assert few[5] == 6 and few[0].tolist() == [6, 7, 8]
    assert r.get(0, max_rows=0)[0].tolist() == [] and r.get(-4)[5] == 5
    e = lr.Ring(8)
    assert e.get()[5:] == (0, 0) and len(e.get()[0]) == 0
    append_n(e, 0, 3, 0)                        # not yet wrapped
    assert e.get(1)[0].tolist() == [1, 2] and e.get(1)[5] == 1


def test_archive_takes_the_accepted_rows_in_batch_order():
    r = lr.Ring(4)
    lost_ids = np.array([10, 11, 12, 13, 14], np.int64)
    mask = np.array([[0b111, 0], [0b1011, 0], [0, 0b11 << 3], [1 << 63, 1], [0b11111, 0]], np.uint64)
    rows, acc = [4, 1, 3, 0], [1, 0, 1, 1]
    gam, p = np.array([0.5, 9.0, 1.5, 2.5]), np.arange(12.0).reshape(4, 3)
    r.archive(lost_ids, mask, rows, acc, gam, p, 6)
    ids, p_w, n_obs, g, stamp, first, seq = r.get()
    assert (first, seq) == (0, 3) and ids.tolist() == [14, 13, 10] and n_obs.tolist() == [5, 2, 3]
    assert g.tolist() == [0.5, 1.5, 2.5] and stamp.tolist() == [6, 6, 6]
    np.testing.assert_array_equal(p_w, p[[0, 2, 3]])


def test_host_ring_equals_the_reference():
    """The package's numpy ring (landmarks='host') against the restatement."""
    rng = np.random.default_rng(3)
    h, r = HostRing(8), lr.Ring(8)
    for n, stamp in ((3, 0), (4, 1), (0, 2), (6, 3), (8, 4)):
        ids = rng.integers(0, 1 << 40, n)
        p, nobs, gam = rng.standard_normal((n, 3)), rng.integers(3, 20, n), rng.random(n)
        h.append(ids, p, nobs, gam, stamp)
        for k in range(n):
            r.append(ids[k], p[k], nobs[k], gam[k], stamp)
        for first, mx in ((0, None), (5, None), (h.seq, None), (2, 3), (h.seq + 4, None)):
            lr.assert_rows_equal(h.get(first, mx), r.get(first, mx), "n=%d first=%d" % (n, first))


# ----------------------------------------------------- the covariance formula --
def test_pose_covariance_formula():
    """G S G^T against its meaning: the covariance of dy = G dx, with dx the error
    (theta, p) of covariance S -- from S's own factor, no matrix product shared
    with the formula -- and entry by entry from the definition."""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((33, 33))
    P = A @ A.T + np.eye(33)
    T = msckf_amd.FilterConfig().T_imu_body.copy()
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    from msckf_amd.geometry import to_rotation
    R = to_rotation(q) @ T[:3, :3]
    assert np.abs(R - np.eye(3)).max() > 0.1
    pose, vel = lr.odom_covariances(P, R)
    idx = [0, 1, 2, 12, 13, 14]
    S = P[np.ix_(idx, idx)]
    L = np.linalg.cholesky(S)                   # dx = L e with e white: dy = G L e, cov = (G L)(G L)^T
    cols = []
    for j in range(6):
        dx = L[:, j]
        cols.append(np.concatenate([R @ dx[:3], R @ dx[3:]]))
    Y = np.array(cols).T
    np.testing.assert_allclose(pose, Y @ Y.T, rtol=0, atol=64 * np.finfo(float).eps * np.abs(P).max())
    ref = np.zeros((6, 6))
    for a in range(6):
        for b in range(6):
            for i in range(3):
                for j in range(3):
                    ref[a, b] += R[a % 3, i] * S[3 * (a // 3) + i, 3 * (b // 3) + j] * R[b % 3, j]
    np.testing.assert_allclose(pose, ref, rtol=0, atol=64 * np.finfo(float).eps * np.abs(P).max())
    Lv = np.linalg.cholesky(P[6:9, 6:9])
    np.testing.assert_allclose(vel, (R @ Lv) @ (R @ Lv).T, rtol=0, atol=64 * np.finfo(float).eps * np.abs(P).max())
    assert np.allclose(pose, pose.T) and np.linalg.eigvalsh(pose).min() > 0
    np.testing.assert_allclose(np.trace(pose), np.trace(S), rtol=1e-12)   # a rotation keeps the trace


# ------------------------------------------------- host logic without a GPU --
N_FRAMES = 40
_STREAMS = {}


def stream(seed):
    if seed not in _STREAMS:
        _STREAMS[seed] = FeatureStream.from_synthetic(synth.make_sequence(n_frames=N_FRAMES, seed=seed))
    return _STREAMS[seed]


def run_single(monkeypatch, **kw):
    monkeypatch.setattr(_lib, "Context", lr.LandmarkContext)
    flt = MSCKF(**kw)
    results = []
    replay(flt, stream(1), on_result=results.append)
    return flt, results


def run_multi(monkeypatch, **kw):
    monkeypatch.setattr(_lib, "Context", lr.LandmarkContext)
    ms = sched_mod.MultiMSCKF(3, **kw)
    out = []
    trajs = ms.run_streams([stream(1), stream(2), stream(3)], on_frame=lambda k, o: out.append(dict(o)))
    return ms, out, trajs


def logs(flt):
    return flt.gate_log, flt.gamma_log, flt.shape_log, flt.cam_ids


def same_results(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert type(x) is type(y) and x.timestamp == y.timestamp
        np.testing.assert_array_equal(x.pose.t, y.pose.t)
        np.testing.assert_array_equal(x.pose.R, y.pose.R)
        np.testing.assert_array_equal(x.velocity, y.velocity)
        for u, v in zip(x[4:], y[4:]):
            np.testing.assert_array_equal(u, v)


def test_single_filter_device_archive_equals_host_archive(monkeypatch):
    host, rh = run_single(monkeypatch, device_map=True, landmarks="host", odometry=True)
    dev, rd = run_single(monkeypatch, device_map=True, landmarks="device", odometry=True)
    plain, rp = run_single(monkeypatch, device_map=True)
    hostmap, rm = run_single(monkeypatch, landmarks="host")
    a, b = host.landmarks(), dev.landmarks()
    assert isinstance(a, Landmarks) and a.next_seq > 10 and a.first_seq == 0
    lr.assert_rows_equal(a, b)
    lr.assert_rows_equal(a, hostmap.landmarks())             # either map
    assert len(set(a.stamp.tolist())) > 3 and (np.diff(a.stamp) >= 0).all() and (a.n_obs >= 3).all()
    assert len(set(a.ids.tolist())) == len(a.ids)            # every id once
    # the accepted entries of the lost updates, in log order
    lr.assert_rows_equal(host.landmarks(first=5), dev.landmarks(first=5))
    assert dev.landmarks(first=5).first_seq == 5
    lr.assert_rows_equal(host.landmarks(live=True), dev.landmarks(live=True))
    lr.assert_rows_equal(hostmap.landmarks(live=True), dev.landmarks(live=True))
    live = dev.landmarks(live=True)
    n_live = len(live.ids) - len(b.ids)
    assert n_live > 0 and (live.stamp[-n_live:] == -1).all() and np.isnan(live.gamma[-n_live:]).all()
    same_results(rh, rd)
    assert all(isinstance(r, VioOdometry) for r in rd) and all(type(r) is VioResult for r in rp)
    for x, y in zip(rd, rp):                                 # the four fields are today's
        assert x[0] == y[0]
        np.testing.assert_array_equal(x.pose.t, y.pose.t)
        np.testing.assert_array_equal(x.velocity, y.velocity)
    assert logs(host) == logs(dev) == logs(plain) == logs(hostmap)
    # one archive call per lost-form update, none on the host mode; one read per frame either way
    n_lost = sum(1 for r in dev.ctx.sent if r[0] == "upd" and r[-1] == MSCKF.ROW_CAP)
    assert [c[0] for c in dev.ctx.calls].count("landmarks_archive") == n_lost > 3
    assert [c[0] for c in host.ctx.calls].count("landmarks_archive") == 0
    assert [c[0] for c in dev.ctx.calls].count("readback_odom") == len(rd) > 30
    pc, vc = lr.odom_covariances(dev.ctx._P(0), dev._T_imu_body._vio_R__)
    np.testing.assert_array_equal(rd[-1].pose_covariance, pc)
    np.testing.assert_array_equal(rd[-1].velocity_covariance, vc)
    assert rd[-1].pose_covariance.shape == (6, 6) and rd[-1].velocity_covariance.shape == (3, 3)
    dev.clear_landmarks()
    host.clear_landmarks()
    assert dev.landmarks().next_seq == 0 == host.landmarks().next_seq and len(dev.landmarks().ids) == 0


def test_three_lanes_device_archive_equals_host_archive(monkeypatch):
    host, oh, _ = run_multi(monkeypatch, device_map=True, landmarks="host", odometry=True)
    dev, od, _ = run_multi(monkeypatch, device_map=True, landmarks="device", odometry=True)
    plain, op, _ = run_multi(monkeypatch, device_map=True)
    hostmap, om, _ = run_multi(monkeypatch, landmarks="host")
    assert dict(host.launches) == dict(dev.launches) == dict(plain.launches)
    seqs = []
    for i in range(3):
        a = host.landmarks(i)
        lr.assert_rows_equal(a, dev.landmarks(i), "lane %d" % i)
        lr.assert_rows_equal(a, hostmap.landmarks(i), "lane %d" % i)
        lr.assert_rows_equal(host.landmarks(i, live=True), dev.landmarks(i, live=True))
        lr.assert_rows_equal(hostmap.landmarks(i, 3, True), dev.landmarks(i, 3, True))
        assert logs(host.lanes[i]) == logs(dev.lanes[i]) == logs(plain.lanes[i]) == logs(hostmap.lanes[i])
        seqs.append(a.next_seq)
    assert min(seqs) > 10 and len(set(seqs)) > 1
    for fh, fd, fp in zip(oh, od, op):
        assert sorted(fh) == sorted(fd) == sorted(fp)
        pub = [i for i in sorted(fd) if fd[i] is not None]   # None before the gravity initialisation
        assert pub == [i for i in sorted(fh) if fh[i] is not None] == [i for i in sorted(fp) if fp[i] is not None]
        same_results([fh[i] for i in pub], [fd[i] for i in pub])
        for i in pub:
            assert isinstance(fd[i], VioOdometry) and type(fp[i]) is VioResult
            np.testing.assert_array_equal(fd[i].pose.t, fp[i].pose.t)
    calls = [c for c in dev.ctx.calls if c[0] == "landmarks_archive"]
    assert any(len(c[1]) == 3 for c in calls)                # one call for the group
    assert len(calls) == dev.ctx.lost_loads < dev.launches["map_update"]   # one per lost-form update, none for prune
    reads = [c for c in dev.ctx.calls if c[0] == "readback_odom"]
    n_pub = sum(1 for o in od if o[0] is not None)
    assert len(reads) == n_pub > 30 and all(len(c[1]) == 3 for c in reads)    # still one grouped read per frame
    dev.clear_landmarks(1)
    assert dev.landmarks(1).next_seq == 0 and dev.landmarks(0).next_seq == seqs[0]


def test_defaults_return_what_they_returned(monkeypatch):
    """Without either option: VioResult, no landmark or odometry call, the plain read."""
    flt, res = run_single(monkeypatch, device_map=True)
    assert flt.ctx.calls == [] and flt.ctx.landmark_cap is None and flt.landmark_mode is None and not flt.odometry
    assert len(res) > 30 and all(type(r) is VioResult and len(r) == 4 for r in res)
    with pytest.raises(ValueError, match="keeps no landmarks"):
        flt.landmarks()
    with pytest.raises(ValueError, match="keeps no landmarks"):
        flt.clear_landmarks()


def test_constructor_rules(monkeypatch):
    monkeypatch.setattr(_lib, "Context", lr.LandmarkContext)
    with pytest.raises(ValueError, match="device_map"):
        MSCKF(landmarks="device")
    with pytest.raises(ValueError, match="device_map"):
        sched_mod.MultiMSCKF(2, landmarks="device")
    with pytest.raises(ValueError, match="expected one of"):
        MSCKF(landmarks="gpu")
    with pytest.raises(ValueError, match="expected one of"):
        sched_mod.MultiMSCKF(2, device_map=True, landmarks=True)
    with pytest.raises(_lib.MsckfError):                     # the ring is no smaller than the map
        MSCKF(device_map=True, map_capacity=512, landmarks="device", landmark_capacity=256)
    flt = MSCKF(device_map=True, map_capacity=64, landmarks="device", landmark_capacity=128)
    assert flt.ctx.landmark_cap == 128 and flt.landmark_mode == "device" and flt._ring is None
    ms = sched_mod.MultiMSCKF(2, device_map=True, map_capacity=64, landmarks="device", landmark_capacity=64)
    assert ms.ctx.landmark_cap == 64 and all(ln.landmark_mode == "device" for ln in ms.lanes)
    h = sched_mod.MultiMSCKF(2, landmarks="host", landmark_capacity=32, odometry=True)
    assert h.ctx.landmark_cap is None and all(ln._ring.cap == 32 and ln.odometry for ln in h.lanes)
    assert msckf_amd.VioOdometry is VioOdometry and msckf_amd.Landmarks is Landmarks
    assert VioOdometry._fields[:4] == VioResult._fields


def test_stereo_vio_takes_the_arguments():
    import inspect
    from msckf_amd.vio import MultiStereoVIO, StereoVIO
    for cls in (MSCKF, sched_mod.MultiMSCKF, MultiStereoVIO, StereoVIO):
        ps = inspect.signature(cls.__init__).parameters
        assert ps["landmarks"].default is None and ps["landmark_capacity"].default == 4096
        assert ps["odometry"].default is False, cls
    for cls in (sched_mod.MultiMSCKF, MultiStereoVIO, StereoVIO, MSCKF):
        assert callable(cls.landmarks) and callable(cls.clear_landmarks)


# ------------------------------------------------------ header and binding --
def test_header_binding_and_library():
    src = open(os.path.join(ROOT, "include", "msckf_odometry.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decls = dict(re.findall(r"\bint\s+(msckf_[a-z_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    assert sorted(decls) == sorted(_lib.ODOMETRY_EXPORTED) and len(decls) == 5
    for name, params in decls.items():
        assert len(_lib.ODOMETRY_SIGS[name][1]) == params.count(",") + 1, name
    assert not set(_lib.ODOMETRY_EXPORTED) & set(_lib.EXPORTED)    # msckf_hip.h and its list stay as they are
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in decls:
        assert hasattr(lib, s), s
