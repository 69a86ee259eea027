"""The aiding fixes of include/msckf_aid.h restated in numpy on the oracle's
state (oracle/msckf_oracle.py), the oracle filter with them, and the fix recipe
of the stream tests.

``prm`` is a ``msckf_amd.AidingConfig`` (or anything with its ``lever``,
``R_body``, ``dir_w`` and ``gates()``); a fix is ``(z (12), var (12), dt,
rows)``, rows the 12-bit mask (bit 3 group + axis; groups POS, VEL, BVEL, DIR).
"""
import numpy as np

from oracle import msckf_oracle as O

POS, VEL, BVEL, DIR = 0x007, 0x038, 0x1c0, 0xe00


def kept(rows):
    return [g for g in range(12) if (rows >> g) & 1]


def aid_predict(st, prm, dt):
    """h(x), all twelve rows."""
    imu = st.imu
    R = O.to_rotation(imu.q)
    l, Rb, d = np.asarray(prm.lever, float), np.asarray(prm.R_body, float), np.asarray(prm.dir_w, float)
    return np.concatenate([imu.p + R.T @ l - dt * imu.v, imu.v, Rb @ R @ imu.v, R @ d])


def aid_rows(st, prm, fix):
    """(H (m x D), r (m), noise variances (m)) of the kept rows."""
    z, var, dt, rows = fix
    imu = st.imu
    D = st.P.shape[0]
    R = O.to_rotation(imu.q)
    l, Rb, d = np.asarray(prm.lever, float), np.asarray(prm.R_body, float), np.asarray(prm.dir_w, float)
    H = np.zeros((12, D))
    H[0:3, 0:3] = -R.T @ O.skew(l)
    H[0:3, 6:9] = -dt * np.eye(3)
    H[0:3, 12:15] = np.eye(3)
    H[3:6, 6:9] = np.eye(3)
    H[6:9, 0:3] = Rb @ O.skew(R @ imu.v)
    H[6:9, 6:9] = Rb @ R
    H[9:12, 0:3] = O.skew(R @ d)
    k = kept(rows)
    r = np.asarray(z, float)[k] - aid_predict(st, prm, dt)[k]
    return H[k], r, np.asarray(var, float)[k]


def aid_gamma(st, prm, fix):
    """(S positive definite, gamma) -- gamma NaN if it is not."""
    H, r, nz = aid_rows(st, prm, fix)
    S = H @ st.P @ H.T + np.diag(nz)
    if not np.isfinite(S).all():
        return False, np.nan
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return False, np.nan
    y = np.linalg.solve(L, r)
    return True, float(y @ y)


def gate_of(prm, rows):
    return prm.gates()[len(kept(rows)) - 1]


def aid_update(st, prm, fix):
    """The gated update on ``st`` in place -> (applied, gamma).  Not applied:
    ``st`` is untouched."""
    pd, gamma = aid_gamma(st, prm, fix)
    if not (pd and gamma < gate_of(prm, fix[3])):
        return False, gamma
    H, r, nz = aid_rows(st, prm, fix)
    P = st.P
    S = H @ P @ H.T + np.diag(nz)
    K = np.linalg.solve(S, H @ P).T
    O.apply_correction(st, K @ r)
    Pn = (np.identity(len(K)) - K @ H) @ st.P
    st.P = (Pn + Pn.T) / 2.
    return True, gamma


def merge(msgs, t_frame, max_age):
    """The frame's fix from the buffered messages ``(t, z, var, rows)``: those
    with t_frame - max_age <= t <= t_frame, every group from the newest message
    that has a row of it; dt is the age of the message that gave the POS rows,
    or of the newest one.  None without a message in the window."""
    win = sorted((m for m in msgs if t_frame - max_age <= m[0] <= t_frame), key=lambda m: -m[0])
    if not win:
        return None
    z, var, rows, dt = np.zeros(12), np.ones(12), 0, t_frame - win[0][0]
    for (t, zf, vf, rf) in win:
        for g in range(4):
            grp = 7 << (3 * g)
            if (rf & grp) and not (rows & grp):
                z[3 * g:3 * g + 3], var[3 * g:3 * g + 3] = zf[3 * g:3 * g + 3], vf[3 * g:3 * g + 3]
                rows |= rf & grp
                if g == 0:
                    dt = t_frame - t
    return z, var, dt, rows


class OracleAid(O.OracleMSCKF):
    """OracleMSCKF with the aiding fix between batch_imu_processing and
    state_augmentation.  ``aiding_callback(t, z, var, rows)`` buffers a message
    already in the filter's world frame; ``aid_log``: (frame, rows, applied,
    gamma)."""

    def __init__(self, cfg, chi2, aiding):
        super().__init__(cfg, chi2)
        self.aiding = aiding
        self.aid_buffer = []
        self.aid_log = []

    def aiding_callback(self, t, z, var, rows):
        self.aid_buffer.append((t, np.asarray(z, float), np.asarray(var, float), rows))

    def feature_callback(self, t, features):
        """OracleMSCKF.feature_callback (msckf.py:180-233) with the update inserted."""
        if not self.is_gravity_set:
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.st.imu.timestamp = t
        self.imu_buffer, self.next_id = O.batch_imu_processing(self.st, self.imu_buffer, t, self.next_id)
        if self.aiding is not None and self.aid_buffer:
            fix = merge(self.aid_buffer, t, self.aiding.max_age)
            self.aid_buffer = [m for m in self.aid_buffer if m[0] > t]
            if fix is not None:
                app, gam = aid_update(self.st, self.aiding, fix)
                self.aid_log.append((self.n_published, fix[3], app, gam))
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


# ------------------------------------------------------------ the streams --

ACC_BIAS = np.array([0.08, -0.06, 0.05])   # added to every IMU sample of the outage streams
LEVER = (0.10, -0.05, 0.20)
SIG = np.array([0.02] * 9 + [0.01] * 3)
MAX_AGE = 0.04
DIR_W = np.array([1.0, 0.0, 0.0])


def outage_sequence(seq, first_blind):
    """``seq`` (synth.Sequence) with the bias on every accelerometer sample and
    every feature message from frame index ``first_blind`` on emptied."""
    from msckf_amd import synth
    imu = [synth.ImuMsg(m.vio_timestamp__, m.angular_velocity, m.linear_acceleration + ACC_BIAS) for m in seq.imu]
    frames = [f if k < first_blind else synth.FeatureMsg(f.timestamp, []) for k, f in enumerate(seq.frames)]
    return synth.Sequence(imu, frames, seq.gt_t, seq.gt_p, seq.gt_R)


def truth_rows(t, t0, A, lever=LEVER, h=1e-4):
    """The noise-free z (12) at time t in the filter's world frame: ``A`` rotates
    the synthetic world into it (both origins coincide); ``t0`` is the end of
    the stream's rest (synth._traj).  R_body = I, d_w = DIR_W."""
    from msckf_amd import synth
    p, R_iw = synth._traj(t, t0)
    v = (synth._traj(t + h, t0)[0] - synth._traj(t - h, t0)[0]) / (2 * h)
    R_f = (A @ R_iw).T          # filter world -> IMU
    pf, vf = A @ p, A @ v
    return np.concatenate([pf + R_f.T @ np.asarray(lever), vf, R_f @ vf, R_f @ DIR_W])


def fix_messages(frame_t, t0, A, rows, seed=100, lead=0.012, every=4, offset=None):
    """The recipe: a message 12 ms before every 4th published frame, truth plus
    sig * standard_normal(12) from default_rng(seed) per message -> [(t, z, var,
    rows)].  ``offset`` (12) is added to every z."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(0, len(frame_t), every):
        t = frame_t[k] - lead
        z = truth_rows(t, t0, A) + SIG * rng.standard_normal(12)
        if offset is not None:
            z = z + offset
        out.append((t, z, SIG ** 2, rows))
    return out


def run_outage(orc, seq, first_blind, msgs=()):
    """Feeds the outage stream of ``seq`` to an oracle filter, the aiding
    messages ``msgs`` up front; returns per published frame (t, p (3), v (3),
    q (4))."""
    for m in msgs:
        orc.aiding_callback(*m)
    recs = []
    for kind, m in outage_sequence(seq, first_blind).events():
        if kind == 0:
            orc.imu_callback(m.vio_timestamp__, m.angular_velocity, m.linear_acceleration)
            continue
        res = orc.feature_callback(m.timestamp, [(f.id, f.u0, f.v0, f.u1, f.v1) for f in m.vio_features])
        if res is not None:
            i = orc.st.imu
            recs.append(np.concatenate([[m.timestamp], i.p, i.v, i.q]))
    return np.array(recs)


def alignment(rec0, seq):
    """A of the recipe from the first published frame's record: the filter's
    IMU -> world rotation times the truth's world -> IMU."""
    k = int(np.argmin(np.abs(seq.gt_t - rec0[0])))
    return O.to_rotation(rec0[7:11]).T @ seq.gt_R[k].T


def position_errors(rec, seq, A):
    """|p - A p_true| per published frame."""
    k0 = int(np.argmin(np.abs(seq.gt_t - rec[0, 0])))
    return np.linalg.norm(rec[:, 1:4] - seq.gt_p[k0:k0 + len(rec)] @ A.T, axis=1)
