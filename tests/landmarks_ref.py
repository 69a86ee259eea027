"""include/msckf_odometry.h restated in numpy: the landmark ring, the archive
call, the incremental read and the pose / velocity covariance, row by row and
entry by entry (no vectorised shortcut shared with the package's own ring).

``LandmarkContext`` is tests/feature_map_ref.py's stand-in with these calls and
with what ``scheduler.MultiMSCKF`` batches, so that the host logic of both
landmark modes runs without a device.
"""
import numpy as np

from msckf_amd import _lib
import feature_map_ref as fr


class Ring:
    """One filter's ring: row k holds the append with seq % cap == k."""

    def __init__(self, cap):
        self.cap = cap
        self.ids = np.zeros(cap, np.int64)
        self.p_w = np.zeros((cap, 3))
        self.n_obs = np.zeros(cap, np.int32)
        self.gamma = np.zeros(cap)
        self.stamp = np.zeros(cap, np.int32)
        self.seq = 0

    def append(self, fid, p_w, n_obs, gamma, stamp):
        k = self.seq % self.cap
        self.ids[k], self.p_w[k], self.n_obs[k], self.gamma[k], self.stamp[k] = fid, p_w, n_obs, gamma, stamp
        self.seq += 1

    def archive(self, lost_ids, lost_mask, rows, accepted, gamma, p_w, stamp):
        """msckf_landmarks_archive of one filter: ``lost_ids`` / ``lost_mask``
        (uint64 [n][2]) the lost table as msckf_map_get returned it before the
        call, ``rows`` the load's, ``accepted`` / ``gamma`` / ``p_w`` the
        filter's part of msckf_batch_results, batch order."""
        for i, r in enumerate(rows):
            if accepted[i]:
                bits = bin(int(lost_mask[r][0])).count("1") + bin(int(lost_mask[r][1])).count("1")
                self.append(lost_ids[r], p_w[i], bits, gamma[i], stamp)

    def get(self, first_seq=0, max_rows=None):
        """msckf_landmarks_get: (ids, p_w, n_obs, gamma, stamp, first, seq)."""
        lo = min(max(first_seq, self.seq - self.cap, 0), self.seq)
        n = self.seq - lo
        if max_rows is not None:
            n = min(n, max_rows)
        k = [(lo + j) % self.cap for j in range(n)]
        return (self.ids[k].copy(), self.p_w[k].copy(), self.n_obs[k].copy(), self.gamma[k].copy(),
                self.stamp[k].copy(), lo, self.seq)


def assert_rows_equal(got, want, msg=""):
    """Two ``get`` results (or Landmarks tuples), bit for bit (NaN equals NaN)."""
    assert len(got) == len(want) == 7
    for k, (a, b) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b), err_msg="%s field %d" % (msg, k))
    for k in (0, 2, 4):
        assert np.asarray(got[k]).dtype == np.asarray(want[k]).dtype, (msg, k)


def odom_covariances(P, R_body):
    """(pose_cov 6 x 6, vel_cov 3 x 3) of msckf_readback_odom from a filter's P."""
    P, R = np.asarray(P, float), np.asarray(R_body, float)
    idx = [0, 1, 2, 12, 13, 14]
    G = np.zeros((6, 6))
    G[:3, :3] = G[3:, 3:] = R
    return G @ P[np.ix_(idx, idx)] @ G.T, R @ P[6:9, 6:9] @ R.T


# ------------------------------------------------------------------ stand-in --
class _Share:
    """One filter's share of a batch's deferred results."""

    def __init__(self, res):
        self.res = res

    def get(self):
        return self.res


class LandmarkContext(fr.RecordingContext):
    """RecordingContext with the landmark rings, msckf_readback_odom and the
    batched calls of scheduler.MultiMSCKF (every filter answered by the
    stand-in's own fixed functions, row cap per filter)."""
    P_SEED = 0

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.landmark_cap = None
        self.calls = []           # the landmark / odometry calls in order
        self.lost_loads = 0       # lost-form map loads

    # ---- a covariance to read: fixed per filter and cam count ----
    def _P(self, f):
        n = 21 + 6 * len(self.cam_serial[f])
        A = np.random.default_rng(self.P_SEED + 100 * f + n).standard_normal((n, n))
        return A @ A.T / n + np.eye(n)

    def get_state(self, f, want_P=True):
        imu, cams, _ = super().get_state(f, want_P=False)
        return imu, cams, (self._P(f) if want_P else None)

    def readback_odom(self, filters, R_body, want_cams=True, cov=None):
        self.calls.append(("readback_odom", tuple(int(f) for f in filters)))
        imu, cams, cv = self.readback(filters, want_cams=want_cams, cov=cov if cov and cov[1] else None)
        pcs, vcs = zip(*[odom_covariances(self._P(f), R_body) for f in filters])
        return imu, cams, cv, np.array(pcs), np.array(vcs)

    # ---- the rings ----
    def landmarks_create(self, cap):
        if self.map_cap is None or self.landmark_cap is not None or not self.map_cap <= cap <= _lib.LANDMARKS_MAX_CAP:
            raise _lib.MsckfError("msckf: landmark capacity (rc=-1)")
        self.landmark_cap = cap
        self.rings = [Ring(cap) for _ in range(self.B)]
        self._lm_loaded = None

    def landmarks_clear(self, filters):
        for f in filters:
            self.rings[f].seq = 0

    def landmarks_archive(self, filters, feat_off, rows, stamps):
        self.calls.append(("landmarks_archive", tuple(int(f) for f in filters)))
        key = (tuple(int(f) for f in filters), tuple(int(x) for x in feat_off), tuple(int(r) for r in rows))
        if self._lm_loaded is None or self._lm_loaded[0] != key or not self._lm_loaded[1]:
            raise _lib.MsckfError("msckf: the archive does not follow its load and update (rc=-1)")
        self._lm_loaded = None
        for w, f in enumerate(filters):
            a, b = self._ranges[f]
            acc, gam, p, _, _ = self._results[f]
            t = self.lost[f]
            self.rings[f].archive(t["ids"], fr.mask_words(t["obs"]), rows[feat_off[w]:feat_off[w + 1]], acc, gam, p,
                                  stamps[w])

    def landmarks_get(self, f, first_seq=0, max_rows=None):
        return self.rings[f].get(first_seq, self.landmark_cap if max_rows is None else max_rows)

    # ---- batches over several filters ----
    def map_load(self, mode, filters, feat_off, rows, counts, p_w=None):
        self._loads, self._ranges, a = {}, {}, 0
        for w in np.argsort(np.asarray(filters), kind="stable"):
            f, lo, hi = int(filters[w]), int(feat_off[w]), int(feat_off[w + 1])
            src = self.lost[f] if mode == _lib.MAP_LOAD_LOST else self.tab[f]
            self._loads[f] = fr.load(src, mode, rows[lo:hi], counts[lo:hi], self.rm[f],
                                     None if p_w is None else np.asarray(p_w)[lo:hi])
            self._ranges[f] = (a, a + hi - lo)
            a += hi - lo
        self._lm_loaded = None
        if mode == _lib.MAP_LOAD_LOST:
            self.lost_loads += 1
            self._lm_loaded = [(tuple(int(f) for f in filters), tuple(int(x) for x in feat_off),
                                tuple(int(r) for r in rows)), False]
        return dict(self._ranges)

    def batch_load(self, feat_off, obs_off, obs_cam, obs_z, p_w=None, chi2=None):
        self._loads, self._ranges, self._lm_loaded = {}, {}, None
        obs_off, obs_z = np.asarray(obs_off, np.int64), np.asarray(obs_z, float).reshape(-1, 4)
        for f in range(self.B):
            a, b = int(feat_off[f]), int(feat_off[f + 1])
            if b > a:
                o0, o1 = obs_off[a], obs_off[b]
                self._loads[f] = ((obs_off[a:b + 1] - o0).astype(np.int32), np.asarray(obs_cam, np.int32)[o0:o1],
                                  obs_z[o0:o1], None if p_w is None else np.asarray(p_w, float)[a:b],
                                  None if chi2 is None else np.asarray(chi2, float)[a:b])
                self._ranges[f] = (a, b)

    def batch_triangulate(self):
        self._results = {}
        for f, (off, cams, zs, _, _) in sorted(self._loads.items()):
            self.sent.append(("tri", f, off.copy(), cams.copy(), zs.copy()))
            p, ok = self._tri_answer(off, zs)
            self._results[f] = (None, None, p, ok, None)

    def batch_update(self, row_cap=0, triangulate=True):
        self._results = {}
        for f, (off, cams, zs, pw, chi2) in sorted(self._loads.items()):
            self.sent.append(("upd", f, off.copy(), cams.copy(), zs.copy(), ~np.isfinite(pw).all(axis=1), chi2.copy(),
                              int(row_cap)))
            self._results[f] = self._upd_answer(off, zs, pw, chi2, row_cap)
        if self._lm_loaded is not None:
            self._lm_loaded[1] = True

    def batch_results(self):
        nf = max((b for _, b in self._ranges.values()), default=0)
        p, ok = np.zeros((nf, 3)), np.zeros(nf, bool)
        for f, (a, b) in self._ranges.items():
            p[a:b], ok[a:b] = self._results[f][2], self._results[f][3]
        return None, None, p, ok, None

    def pending(self, ranges):
        return [_Share(self._results[s]) for s, _, _ in ranges]

    def update_async(self, f, off, cams, zs, pw, chi2, row_cap=0):
        self._lm_loaded = None
        return super().update_async(f, off, cams, zs, pw, chi2, row_cap)

    # ---- the rest of what scheduler.MultiMSCKF calls ----
    def propagate_batch(self, filters, sample_off, dt, gyro, acc):
        pass

    def augment_batch(self, filters):
        for f in filters:
            self.augment(f)

    def prune_batch(self, filters, slot_off, slots):
        for w, f in enumerate(filters):
            self.prune(f, slots[slot_off[w]:slot_off[w + 1]])

    def cov_diag_batch(self, filters, i0, n):
        return np.zeros((len(filters), n))
