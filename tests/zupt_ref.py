"""The zero-velocity update of include/msckf_zupt.h restated in numpy on the
oracle's state (oracle/msckf_oracle.py), and the oracle filter with it.

``prm`` is a ``msckf_amd.ZuptConfig`` (or anything with its fields and its
``mask()`` / ``gate()``).
"""
import numpy as np

from oracle import msckf_oracle as O

VEL, GYRO, ACC = 1, 2, 4


def zupt_residual(st, w_mean, a_mean, mask):
    """r of the kept groups, in the order VEL, GYRO, ACC."""
    imu = st.imu
    Rg = O.to_rotation(imu.q) @ st.gravity
    r = []
    if mask & VEL:
        r.append(-imu.v)
    if mask & GYRO:
        r.append(np.asarray(w_mean, float) - imu.bg)
    if mask & ACC:
        r.append(np.asarray(a_mean, float) - imu.ba + Rg)
    return np.concatenate(r)


def zupt_rows(st, w_mean, a_mean, prm):
    """(H (m x D), r (m), noise variances (m)) of the measurement."""
    mask = prm.mask()
    D = st.P.shape[0]
    Rg = O.to_rotation(st.imu.q) @ st.gravity
    H, nz = [], []
    if mask & VEL:
        h = np.zeros((3, D))
        h[:, 6:9] = np.eye(3)
        H.append(h)
        nz += [prm.vel_noise] * 3
    if mask & GYRO:
        h = np.zeros((3, D))
        h[:, 3:6] = np.eye(3)
        H.append(h)
        nz += [prm.gyro_noise] * 3
    if mask & ACC:
        h = np.zeros((3, D))
        h[:, 0:3] = -O.skew(Rg)
        h[:, 9:12] = np.eye(3)
        H.append(h)
        nz += [prm.acc_noise] * 3
    return np.vstack(H), zupt_residual(st, w_mean, a_mean, mask), np.array(nz, float)


def zupt_gamma(st, w_mean, a_mean, prm):
    """(S positive definite, gamma) -- gamma NaN if it is not."""
    H, r, nz = zupt_rows(st, w_mean, a_mean, prm)
    S = H @ st.P @ H.T + np.diag(nz)
    if not np.isfinite(S).all():
        return False, np.nan
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return False, np.nan
    y = np.linalg.solve(L, r)
    return True, float(y @ y)


def zupt_update(st, w_mean, a_mean, prm):
    """The gated update on ``st`` in place -> (applied, gamma).  Not applied:
    ``st`` is untouched."""
    pd, gamma = zupt_gamma(st, w_mean, a_mean, prm)
    if not (pd and gamma < prm.gate() and np.linalg.norm(st.imu.v) <= prm.max_speed):
        return False, gamma
    H, r, nz = zupt_rows(st, w_mean, a_mean, prm)
    P = st.P
    S = H @ P @ H.T + np.diag(nz)
    K = np.linalg.solve(S, H @ P).T
    dx = K @ r
    O.apply_correction(st, dx)
    Pn = (np.identity(len(K)) - K @ H) @ st.P
    st.P = (Pn + Pn.T) / 2.
    return True, gamma


def propagated_samples(st, buffer, time_bound):
    """The (gyro, acc) samples batch_imu_processing (msckf.py:262-287) will
    hand to process_model, without touching anything."""
    ws, accs = [], []
    t_state = st.imu.timestamp
    for (t, w, a) in buffer:
        if t < t_state:
            continue
        if t > time_bound:
            break
        ws.append(w)
        accs.append(a)
        t_state = t
    return ws, accs


class OracleZupt(O.OracleMSCKF):
    """OracleMSCKF with the zero-velocity update between batch_imu_processing
    and state_augmentation, once per frame that propagated a sample, with the
    means of exactly those samples.  ``zupt_log``: (frame, applied, gamma)."""

    def __init__(self, cfg, chi2, zupt):
        super().__init__(cfg, chi2)
        self.zupt = zupt
        self.zupt_log = []

    def feature_callback(self, t, features):
        """OracleMSCKF.feature_callback (msckf.py:180-233) with the update inserted."""
        if not self.is_gravity_set:
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.st.imu.timestamp = t
        ws, accs = propagated_samples(self.st, self.imu_buffer, t)
        self.imu_buffer, self.next_id = O.batch_imu_processing(self.st, self.imu_buffer, t, self.next_id)
        if self.zupt is not None and ws:
            app, gam = zupt_update(self.st, np.mean(np.array(ws), axis=0), np.mean(np.array(accs), axis=0), self.zupt)
            self.zupt_log.append((self.n_published, app, gam))
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


def run_oracle(orc, seq):
    """Feeds ``seq`` (synth.Sequence) to an oracle filter; returns per published
    frame (t, p (3), v (3), q (4))."""
    recs = []
    for kind, m in seq.events():
        if kind == 0:
            orc.imu_callback(m.vio_timestamp__, m.angular_velocity, m.linear_acceleration)
            continue
        res = orc.feature_callback(m.timestamp, [(f.id, f.u0, f.v0, f.u1, f.v1) for f in m.vio_features])
        if res is not None:
            i = orc.st.imu
            recs.append(np.concatenate([[m.timestamp], i.p, i.v, i.q]))
    return np.array(recs)
