"""The vision standstill cue of include/msckf_standstill.h restated in numpy: the
motion statistic, the cue's status, the two decision rules around the
zero-velocity update of tests/zupt_ref.py, and the oracle filter with them.

``prm`` is a ``msckf_amd.ZuptConfig``, ``cue`` a ``msckf_amd.VisionCue`` (or
anything with their fields).
"""
import numpy as np

from oracle import msckf_oracle as O
import zupt_ref as Z

MOVING, STILL, UNKNOWN = 0, 1, 2


# ------------------------------------------------------------ the statistic --
def motion_d2(prev, curr):
    """d2 float32 [n]: dx dx + dy dy in float32, each product and the sum rounded once."""
    prev = np.asarray(prev, np.float32).reshape(-1, 2)
    curr = np.asarray(curr, np.float32).reshape(-1, 2)
    dx = curr[:, 0] - prev[:, 0]
    dy = curr[:, 1] - prev[:, 1]
    xx = dx * dx
    yy = dy * dy
    out = xx + yy
    assert out.dtype == np.float32
    return out


def motion_k(n, q):
    """k = floor(q (n - 1)) in double."""
    return int(np.floor(float(q) * float(n - 1)))


def motion_stat(prev, curr, q):
    """(n, the k-th smallest d2 as float32) -- NaN for n = 0."""
    d2 = motion_d2(prev, curr)
    n = len(d2)
    if n == 0:
        return 0, np.float32(np.nan)
    return n, np.sort(d2)[motion_k(n, q)]


# ------------------------------------------------- the status and the rules --
def cue_status(n, d2, cue):
    """n < 0: no record."""
    if n < 0 or n < cue.min_tracks:
        return UNKNOWN
    return STILL if float(np.float32(d2)) <= float(cue.max_px) * float(cue.max_px) else MOVING


def decide(pd, gamma, speed, status, prm, cue):
    """applied, from S positive definite, gamma, |v| and the cue's status."""
    imu_ok = bool(pd and gamma < prm.gate() and speed <= prm.max_speed)
    fall = cue.unknown == "imu"
    if cue.mode == "veto":
        return imu_ok and (status == STILL or (status == UNKNOWN and fall))
    assert cue.mode == "either"
    return bool(pd and status == STILL) or (imu_ok and (status != UNKNOWN or fall))


def zupt_update_cued(st, w_mean, a_mean, prm, cue, n, d2):
    """The cued update on ``st`` in place -> (applied, gamma, status).  Not
    applied: ``st`` is untouched.  The applied update is zupt_ref's."""
    pd, gamma = Z.zupt_gamma(st, w_mean, a_mean, prm)
    status = cue_status(n, d2, cue)
    if not decide(pd, gamma, np.linalg.norm(st.imu.v), status, prm, cue):
        return False, gamma, status
    H, r, nz = Z.zupt_rows(st, w_mean, a_mean, prm)
    P = st.P
    S = H @ P @ H.T + np.diag(nz)
    K = np.linalg.solve(S, H @ P).T
    O.apply_correction(st, K @ r)
    Pn = (np.identity(len(K)) - K @ H) @ st.P
    st.P = (Pn + Pn.T) / 2.
    return True, gamma, status


# ------------------------------------------------------- the oracle filter --
def geometric_cue(prev_feats, feats, focal, q):
    """(n, d2) from two consecutive messages' normalised cam0 coordinates matched
    by id, times the focal length; (-1, NaN) without a previous message."""
    if prev_feats is None:
        return -1, np.float32(np.nan)
    before = {f[0]: (f[1], f[2]) for f in prev_feats}
    pairs = [(before[f[0]], (f[1], f[2])) for f in feats if f[0] in before]
    prev = focal * np.array([p for p, _ in pairs], float).reshape(-1, 2)
    curr = focal * np.array([c for _, c in pairs], float).reshape(-1, 2)
    return motion_stat(prev, curr, q)


class OracleStandstill(Z.OracleZupt):
    """OracleZupt with the cue in the decision.  ``cue`` None: OracleZupt's own
    update (the IMU-only rule), its log extended by the geometric cue it would
    have seen.  ``zupt_log``: (frame, applied, gamma, status, n, d2)."""

    def __init__(self, cfg, chi2, zupt, cue=None, focal=458.654, quantile=0.5):
        super().__init__(cfg, chi2, zupt)
        self.cue, self.focal, self.quantile = cue, focal, quantile
        self._prev_feats = None

    def feature_callback(self, t, features):
        """OracleZupt.feature_callback with the cued update in the update's place.
        The cue is the stream's: a message that arrives before gravity is set is
        remembered too (the front-end tracks those frames), so the filter's first
        frame has a cue whenever the stream had a message before it."""
        if not self.is_gravity_set:
            self._prev_feats = features
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.st.imu.timestamp = t
        ws, accs = Z.propagated_samples(self.st, self.imu_buffer, t)
        self.imu_buffer, self.next_id = O.batch_imu_processing(self.st, self.imu_buffer, t, self.next_id)
        n, d2 = geometric_cue(self._prev_feats, features, self.focal, self.quantile)
        self._prev_feats = features
        if self.zupt is not None and ws:
            w, a = np.mean(np.array(ws), axis=0), np.mean(np.array(accs), axis=0)
            if self.cue is None:
                app, gam = Z.zupt_update(self.st, w, a, self.zupt)
                status = -1
            else:
                app, gam, status = zupt_update_cued(self.st, w, a, self.zupt, self.cue, n, d2)
            self.zupt_log.append((self.n_published, app, gam, status, n, d2))
        O.state_augmentation(self.st, t, self.st.imu.id)
        self._add_observations(features)
        frame = {"t": t}
        frame["lost"] = self._remove_lost_features()
        frame["prune"] = self._prune_cam_state_buffer()
        self.log.append(frame)
        try:
            return self.publish(t)
        finally:
            self.n_published += 1
            self._online_reset()
