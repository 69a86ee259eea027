"""The delayed aiding fixes of include/msckf_aid_delayed.h restated in numpy on
the oracle's state (oracle/msckf_oracle.py), the routing of late messages, the
oracle filter with both and the late-fix recipe of the stream tests.

``prm`` is a ``msckf_amd.AidingConfig`` (or anything with its ``lever``,
``dir_w`` and ``gates()``); a fix is ``(z (6), var (6), slot, lam, rows)``, rows
the 6-bit mask (bit 3 group + axis; groups POS, DIR).
"""
import numpy as np

from oracle import msckf_oracle as O
import aid_ref

POS, DIR = 0x07, 0x38
NONE, APPLIED, GATED, NOT_PD, BAD_SLOT = -1, 0, 1, 2, 3
SMALL = 1e-4      # below this angle the series forms are used
TIME_TOL = 1e-9   # a stamp this close to a clone's is the clone's


def kept(rows):
    return [g for g in range(6) if (rows >> g) & 1]


# ------------------------------------------------------------------ SO(3) --

def _abc(th):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3."""
    if th < SMALL:
        t2 = th * th
        return 1.0 - t2 / 6.0, 0.5 - t2 / 24.0, 1.0 / 6.0 - t2 / 120.0
    return np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3


def so3_exp(phi):
    K = O.skew(phi)
    a, b, _ = _abc(np.linalg.norm(phi))
    return np.eye(3) + a * K + b * K @ K


def so3_log(M):
    """phi with so3_exp(phi) = M, |phi| < pi, from M's skew part v = sin(th) axis
    and its trace."""
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    s = np.linalg.norm(v)
    if s < SMALL:
        return v * (1.0 + s * s / 6.0)
    return v * (np.arctan2(s, 0.5 * (np.trace(M) - 1.0)) / s)


def so3_jl(phi):
    K = O.skew(phi)
    _, b, c = _abc(np.linalg.norm(phi))
    return np.eye(3) + b * K + c * K @ K


def so3_jl_inv(phi):
    K = O.skew(phi)
    th = np.linalg.norm(phi)
    if th < SMALL:
        d = 1.0 / 12.0 + th * th / 720.0
    else:
        d = 1.0 / th ** 2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) - 0.5 * K + d * K @ K


# ------------------------------------------------------------ measurement --

def in_window(st, slot, lam):
    n = len(st.cams)
    return 0 <= slot < n and (lam == 0.0 or slot + 1 < n)


def interpolate(st, slot, lam):
    """(R_c, p_c, A0, A1): the interpolated world -> cam0 rotation and cam0
    position, and dtheta_c = A0 dtheta_s + A1 dtheta_{s+1}.  lam == 0 reads clone
    ``slot`` alone."""
    cams = list(st.cams.values())
    R0, p0 = O.to_rotation(cams[slot].q), cams[slot].p
    if lam == 0.0:
        return R0, p0.copy(), np.eye(3), np.zeros((3, 3))
    R1, p1 = O.to_rotation(cams[slot + 1].q), cams[slot + 1].p
    phi = so3_log(R1 @ R0.T)
    E, Jl, Ji = so3_exp(lam * phi), so3_jl(lam * phi), so3_jl_inv(phi)
    return E @ R0, (1.0 - lam) * p0 + lam * p1, E - lam * Jl @ Ji.T, lam * Jl @ Ji


def predict(st, prm, slot, lam):
    """h(x), all six rows."""
    imu = st.imu
    Rc, pc, _, _ = interpolate(st, slot, lam)
    mc = imu.R_imu_cam0 @ (np.asarray(prm.lever, float) - imu.t_cam0_imu)
    return np.concatenate([pc + Rc.T @ mc, imu.R_imu_cam0.T @ (Rc @ np.asarray(prm.dir_w, float))])


def rows_of(st, prm, fix):
    """(H (m x D), r (m), noise variances (m)) of the kept rows."""
    z, var, slot, lam, rows = fix
    imu = st.imu
    D = st.P.shape[0]
    Rc, pc, A0, A1 = interpolate(st, slot, lam)
    Ric = imu.R_imu_cam0
    mc = Ric @ (np.asarray(prm.lever, float) - imu.t_cam0_imu)
    u = Rc @ np.asarray(prm.dir_w, float)
    Gp, Gd = -Rc.T @ O.skew(mc), Ric.T @ O.skew(u)
    H = np.zeros((6, D))
    c0 = 21 + 6 * slot
    H[0:3, 15:18], H[0:3, 18:21] = -Gp, -Rc.T @ Ric
    H[3:6, 15:18] = -Gd
    H[0:3, c0:c0 + 3], H[0:3, c0 + 3:c0 + 6] = Gp @ A0, (1.0 - lam) * np.eye(3)
    H[3:6, c0:c0 + 3] = Gd @ A0
    if lam != 0.0:
        H[0:3, c0 + 6:c0 + 9], H[0:3, c0 + 9:c0 + 12] = Gp @ A1, lam * np.eye(3)
        H[3:6, c0 + 6:c0 + 9] = Gd @ A1
    k = kept(rows)
    r = np.asarray(z, float)[k] - predict(st, prm, slot, lam)[k]
    return H[k], r, np.asarray(var, float)[k]


def gamma_of(st, prm, fix):
    """(S positive definite, gamma) -- gamma NaN if it is not."""
    H, r, nz = rows_of(st, prm, fix)
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


def update(st, prm, fix):
    """The gated update on ``st`` in place -> (applied, gamma, status).  Not
    applied: ``st`` is untouched."""
    if not in_window(st, fix[2], fix[3]):
        return False, np.nan, BAD_SLOT
    pd, gamma = gamma_of(st, prm, fix)
    if not pd:
        return False, gamma, NOT_PD
    if not gamma < gate_of(prm, fix[4]):
        return False, gamma, GATED
    H, r, nz = rows_of(st, prm, fix)
    P = st.P
    S = H @ P @ H.T + np.diag(nz)
    K = np.linalg.solve(S, H @ P).T
    O.apply_correction(st, K @ r)
    Pn = (np.identity(len(K)) - K @ H) @ st.P
    st.P = (Pn + Pn.T) / 2.
    return True, gamma, APPLIED


# ---------------------------------------------------------------- routing --

def route(t, rows12, t_frame, cam_times, cfg):
    """Where the message (t, 12-bit rows) goes at the frame t_frame <= its stamp's
    frame: ("current",), ("delayed", slot, lam, rows6, dropped rows12), ("wait",)
    or ("drop", reason).  ``cam_times`` are the live clones' times, oldest first;
    ``cfg`` has max_age, delayed, max_delay, max_gap."""
    age = t_frame - t
    if age <= cfg.max_age:
        return ("current",)
    if not cfg.delayed:
        return ("drop", "stale")
    rows6 = (rows12 & 0x007) | ((rows12 >> 9) & 0x7) << 3
    if not rows6:
        return ("drop", "no delayed rows")
    if age > cfg.max_delay:
        return ("drop", "older than max_delay")
    if not len(cam_times) or t < cam_times[0] - TIME_TOL:
        return ("drop", "older than the window")
    if t > cam_times[-1] + TIME_TOL:
        return ("wait",)
    other = rows12 & 0x1f8
    for s, ts in enumerate(cam_times):
        if abs(t - ts) <= TIME_TOL:
            return ("delayed", s, 0.0, rows6, other)
    s = int(np.searchsorted(np.asarray(cam_times), t)) - 1
    gap = cam_times[s + 1] - cam_times[s]
    if gap > cfg.max_gap + TIME_TOL:
        return ("drop", "clones too far apart")
    return ("delayed", s, float((t - cam_times[s]) / gap), rows6, other)


def six(z12, var12):
    """The POS and DIR entries of a 12-row message."""
    z12, var12 = np.asarray(z12, float), np.asarray(var12, float)
    return np.concatenate([z12[0:3], z12[9:12]]), np.concatenate([var12[0:3], var12[9:12]])


class OracleAidDelayed(aid_ref.OracleAid):
    """OracleAid with the routing above: the delayed fixes oldest first, then
    the frame's merged fix, between batch_imu_processing and state_augmentation.
    ``aid_delayed_log``: (frame, rows, applied, gamma, slot, lam, status);
    ``aid_dropped``: (frame, t, reason)."""

    def __init__(self, cfg, chi2, aiding):
        super().__init__(cfg, chi2, aiding)
        self.aid_delayed_log = []
        self.aid_dropped = []

    def feature_callback(self, t, features):
        if not self.is_gravity_set:
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.st.imu.timestamp = t
        self.imu_buffer, self.next_id = O.batch_imu_processing(self.st, self.imu_buffer, t, self.next_id)
        if self.aiding is not None and self.aid_buffer:
            cam_times = [c.timestamp for c in self.st.cams.values()]
            keep, cur, late = [], [], []
            for m in self.aid_buffer:
                if m[0] > t:
                    keep.append(m)
                    continue
                rt = route(m[0], m[3], t, cam_times, self.aiding)
                if rt[0] == "current":
                    cur.append(m)
                elif rt[0] == "delayed":
                    late.append((m, rt))
                elif rt[0] == "wait":
                    keep.append(m)
                else:
                    self.aid_dropped.append((self.n_published, m[0], rt[1]))
            self.aid_buffer = keep
            for m, (_, slot, lam, rows6, _) in sorted(late, key=lambda e: e[0][0]):
                z, var = six(m[1], m[2])
                app, gam, status = update(self.st, self.aiding, (z, var, slot, lam, rows6))
                self.aid_delayed_log.append((self.n_published, rows6, app, gam, slot, lam, status))
            fix = aid_ref.merge(cur, t, self.aiding.max_age)
            if fix is not None:
                app, gam = aid_ref.aid_update(self.st, self.aiding, fix)
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


def late_messages(frame_t, t0, A, rows12, latency, seed=100, lead=0.012, every=4):
    """aid_ref.fix_messages' recipe (the same stamps, truth and noise) with the
    delivery time: [(arrival, (t, z, var, rows))], arrival = t + latency."""
    return [(m[0] + latency, m) for m in aid_ref.fix_messages(frame_t, t0, A, rows12, seed=seed, lead=lead, every=every)]


def run_outage_late(orc, seq, first_blind, late):
    """aid_ref.run_outage, each message handed over once the stream's time has
    reached its arrival."""
    late = sorted(late, key=lambda e: e[0])
    k, recs = 0, []
    for kind, m in aid_ref.outage_sequence(seq, first_blind).events():
        tm = m.vio_timestamp__ if kind == 0 else m.timestamp
        while k < len(late) and late[k][0] <= tm:
            orc.aiding_callback(*late[k][1])
            k += 1
        if kind == 0:
            orc.imu_callback(m.vio_timestamp__, m.angular_velocity, m.linear_acceleration)
            continue
        res = orc.feature_callback(m.timestamp, [(f.id, f.u0, f.v0, f.u1, f.v1) for f in m.vio_features])
        if res is not None:
            i = orc.st.imu
            recs.append(np.concatenate([[m.timestamp], i.p, i.v, i.q]))
    return np.array(recs)
