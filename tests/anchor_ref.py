"""The anchor fixes of include/msckf_anchor.h restated in numpy on the oracle's
state (oracle/msckf_oracle.py), the oracle filter with them, and the anchor
recipe of the stream tests.

``prm`` is a ``msckf_amd.AnchorConfig`` (or anything with its ``obs_var``,
``gate()``, ``min_depth`` and ``min_anchors``; an ``obs_var`` of None is the
state's own sigma2); the anchors of a call are ``(p (K, 3), cov (K, 3, 3),
z (K, 4))`` in the filter's world frame.
"""
import numpy as np

from oracle import msckf_oracle as O

USED, GATED, DEPTH, NOT_PD = 0, 1, 2, 3
COLS = [0, 1, 2] + list(range(12, 21))   # the twelve columns of P that H touches
MAX = 64


def obs_var_of(prm, st):
    return st.sigma2 if prm.obs_var is None else float(prm.obs_var)


def geometry(st):
    """(R, R0, t0, R1, t1): world -> IMU, world -> cam0 and its centre, cam1's."""
    imu = st.imu
    R = O.to_rotation(imu.q)
    R0 = imu.R_imu_cam0 @ R
    t0 = imu.p + R.T @ imu.t_cam0_imu
    R1 = st.R_cam0_cam1 @ R0
    t1 = t0 - R1.T @ st.t_cam0_cam1
    return R, R0, t0, R1, t1


def anchor_predict(st, p_w):
    """(zhat (4), a, b): the predicted normalised coordinates and the point in cam0 and cam1."""
    _, R0, t0, R1, t1 = geometry(st)
    a, b = R0 @ (p_w - t0), R1 @ (p_w - t1)
    return np.array([a[0] / a[2], a[1] / a[2], b[0] / b[2], b[1] / b[2]]), a, b


def anchor_rows(st, p_w, cov, z, obs_var):
    """(H_l (4 x D), r (4), N_l (4 x 4), Hf (4 x 3)) of one anchor."""
    imu = st.imu
    R, R0, t0, R1, t1 = geometry(st)
    zhat, a, b = anchor_predict(st, p_w)
    dz0, dz1 = np.zeros((4, 3)), np.zeros((4, 3))
    dz0[0] = [1 / a[2], 0, -a[0] / a[2] ** 2]
    dz0[1] = [0, 1 / a[2], -a[1] / a[2] ** 2]
    dz1[2] = [1 / b[2], 0, -b[0] / b[2] ** 2]
    dz1[3] = [0, 1 / b[2], -b[1] / b[2] ** 2]
    Hx = np.zeros((4, 6))
    Hx[:, 0:3] = dz0 @ O.skew(a) + dz1 @ st.R_cam0_cam1 @ O.skew(a)
    Hx[:, 3:6] = -(dz0 @ R0 + dz1 @ R1)
    J = np.zeros((6, 21))
    J[0:3, 0:3] = imu.R_imu_cam0
    J[0:3, 15:18] = np.eye(3)
    J[3:6, 0:3] = -R.T @ O.skew(imu.t_cam0_imu)
    J[3:6, 12:15] = np.eye(3)
    J[3:6, 18:21] = R.T
    H = np.zeros((4, st.P.shape[0]))
    H[:, :21] = Hx @ J
    Hf = -Hx[:, 3:6]
    return H, np.asarray(z, float) - zhat, obs_var * np.eye(4) + Hf @ np.asarray(cov, float) @ Hf.T, Hf


def _chol(M):
    """The lower Cholesky factor, or None at a pivot <= 0 or a NaN."""
    if not np.isfinite(M).all():
        return None
    try:
        return np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None


def anchor_gate(st, prm, anchors):
    """Per anchor: (status uint8 (K), gamma (K), whitened rows [(Ht (4 x D), rt (4))] of the used ones)."""
    p, cov, z = anchors
    K = len(p)
    status, gamma, rows = np.zeros(K, np.uint8), np.full(K, np.nan), []
    var = obs_var_of(prm, st)
    for l in range(K):
        _, a, b = anchor_predict(st, p[l])
        if not (a[2] > prm.min_depth and b[2] > prm.min_depth):
            status[l] = DEPTH
            continue
        H, r, N, _ = anchor_rows(st, p[l], cov[l], z[l], var)
        C = _chol(N)
        L = _chol(H @ st.P @ H.T + N) if C is not None else None
        if L is None:
            status[l] = NOT_PD
            continue
        y = np.linalg.solve(L, r)
        gamma[l] = y @ y
        if not gamma[l] < prm.gate():
            status[l] = GATED
            continue
        rows.append((np.linalg.solve(C, H), np.linalg.solve(C, r)))
    return status, gamma, rows


def compress(Ht, rt):
    """The stack's thin QR in the columns COLS when it has more than twelve rows: (H' (m x D), r' (m))."""
    if len(Ht) <= 12:
        return Ht, rt
    Q, R = np.linalg.qr(Ht[:, COLS])
    Hp = np.zeros((12, Ht.shape[1]))
    Hp[:, COLS] = R
    return Hp, Q.T @ rt


def anchor_update(st, prm, anchors, compressed=False):
    """The gated update on ``st`` in place -> (applied, used, rows, status (K),
    gamma (K)).  Not applied: ``st`` is untouched.  The update itself is the
    UNCOMPRESSED one, all 4 K' whitened rows, unless ``compressed``: rows is the
    specification's m = min(4 K', 12) either way."""
    status, gamma, rows = anchor_gate(st, prm, anchors)
    used = len(rows)
    m = min(4 * used, 12)
    if used == 0 or used < prm.min_anchors:
        return False, used, m, status, gamma
    Ht, rt = np.vstack([h for h, _ in rows]), np.concatenate([r for _, r in rows])
    if compressed:
        Ht, rt = compress(Ht, rt)
    P = st.P
    S = Ht @ P @ Ht.T + np.eye(len(Ht))
    if _chol(S) is None:
        return False, used, m, status, gamma
    K = np.linalg.solve(S, Ht @ P).T
    O.apply_correction(st, K @ rt)
    Pn = (np.identity(len(K)) - K @ Ht) @ st.P
    st.P = (Pn + Pn.T) / 2.
    return True, used, m, status, gamma


class OracleAnchor(O.OracleMSCKF):
    """OracleMSCKF with the anchor update between batch_imu_processing and
    state_augmentation.  ``anchor_callback(t, p, cov, z)`` buffers a message
    already in the filter's world frame; the frame within ``time_tol`` of it
    applies it, older messages are dropped.  ``anchor_log``: (frame, n, used,
    applied); ``anchor_records``: (status, gamma) per logged frame."""

    def __init__(self, cfg, chi2, anchors):
        super().__init__(cfg, chi2)
        self.anchors = anchors
        self.anchor_buffer = []
        self.anchor_log = []
        self.anchor_records = []
        self.anchor_dropped = 0

    def anchor_callback(self, t, p, cov, z):
        self.anchor_buffer.append((t, (np.asarray(p, float), np.asarray(cov, float), np.asarray(z, float))))
        self.anchor_buffer.sort(key=lambda m: m[0])

    def _take(self, t):
        tol, msg = self.anchors.time_tol, None
        while self.anchor_buffer and self.anchor_buffer[0][0] <= t + tol:
            m = self.anchor_buffer.pop(0)
            if m[0] >= t - tol and msg is None:
                msg = m[1]
            else:
                self.anchor_dropped += 1
        return msg

    def feature_callback(self, t, features):
        """OracleMSCKF.feature_callback (msckf.py:180-233) with the update inserted."""
        if not self.is_gravity_set:
            if self.anchors is not None and self._take(t) is not None:   # before gravity initialisation: dropped
                self.anchor_dropped += 1
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.st.imu.timestamp = t
        self.imu_buffer, self.next_id = O.batch_imu_processing(self.st, self.imu_buffer, t, self.next_id)
        if self.anchors is not None:
            msg = self._take(t)
            if msg is not None:
                app, used, _, status, gamma = anchor_update(self.st, self.anchors, msg)
                self.anchor_log.append((self.n_published, len(status), used, app))
                self.anchor_records.append((status, gamma))
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

BOX = (np.array([4.0, -2.5, -1.5]), np.array([7.0, 2.5, 1.5]))   # in the synthetic world
SURVEY_SIGMA = 0.005
PIX_SIGMA = 0.5 / 458.654


def visible(L, t, t0, cfg):
    """make_sequence's visibility test of the synthetic-world points ``L`` (n, 3)
    at time t: (mask (n), true normalised coordinates (n, 4))."""
    from msckf_amd import synth
    R_ic, t_ic = cfg.T_imu_cam0[:3, :3], cfg.T_imu_cam0[:3, 3]
    Rcc, tcc = cfg.T_cn_cnm1[:3, :3], cfg.T_cn_cnm1[:3, 3]
    p_i, R_iw = synth._traj(t, t0)
    R0 = R_ic @ R_iw.T
    t_c0 = p_i + R_iw @ (-R_ic.T @ t_ic)
    R1 = Rcc @ R0
    t_c1 = t_c0 - R1.T @ tcc
    pc0, pc1 = (L - t_c0) @ R0.T, (L - t_c1) @ R1.T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = np.stack([pc0[:, 0] / pc0[:, 2], pc0[:, 1] / pc0[:, 2], pc1[:, 0] / pc1[:, 2], pc1[:, 1] / pc1[:, 2]], 1)
    vis = (pc0[:, 2] > 0.5) & (pc1[:, 2] > 0.5) & (np.abs(uv[:, 0]) < 0.75) & (np.abs(uv[:, 1]) < 0.5) \
        & (np.abs(uv[:, 2]) < 0.75) & (np.abs(uv[:, 3]) < 0.5)
    return vis, uv


def anchor_messages(frame_t, t0, Al, cfg, n=8, seed=200, every=4):
    """The recipe: ``n`` anchors uniform in BOX from default_rng(seed), rotated
    into the filter's world by ``Al`` (both origins coincide) plus SURVEY_SIGMA
    * standard_normal((n, 3)) and declared with SURVEY_SIGMA^2 I; a message AT
    every ``every``-th published frame with the anchors that pass
    make_sequence's visibility test, their true projections plus PIX_SIGMA *
    standard_normal(4) each -> ([(t, p, cov, z)], declared positions (n, 3),
    true positions in the synthetic world (n, 3))."""
    rng = np.random.default_rng(seed)
    L = BOX[0] + (BOX[1] - BOX[0]) * rng.random((n, 3))
    declared = L @ Al.T + SURVEY_SIGMA * rng.standard_normal((n, 3))
    out = []
    for k in range(0, len(frame_t), every):
        vis, uv = visible(L, frame_t[k], t0, cfg)
        idx = np.flatnonzero(vis)
        z = uv[idx] + PIX_SIGMA * rng.standard_normal((len(idx), 4))
        cov = np.broadcast_to(SURVEY_SIGMA ** 2 * np.eye(3), (len(idx), 3, 3)).copy()
        out.append((frame_t[k], declared[idx].copy(), cov, z))
    return out, declared, L


def run_outage(orc, seq, first_blind, msgs=()):
    """aid_ref.run_outage with the anchor messages ``msgs`` up front."""
    import aid_ref
    for m in msgs:
        orc.anchor_callback(*m)
    return aid_ref.run_outage(orc, seq, first_blind)
