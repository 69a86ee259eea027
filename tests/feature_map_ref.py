"""include/msckf_map.h restated in numpy, arrays only, one function per call.

A table is a dict of arrays: ids int64 [n], obs bool [n][Nmax] (the mask),
z float64 [n][Nmax][4], p_w float64 [n][3], init bool [n].  Every function
returns a new table and leaves its input alone, as the two tables of a slot do.
``COUNTERS`` counts the branches taken (tests assert that each was).

``RecordingContext`` is a stand-in for ``_lib.Context`` without a device: it
keeps cam counts and a table per slot through the functions below, records the
feature batch of every triangulate / update request and the slots of every
prune, and answers triangulations and gates by a fixed function of the
feature -- of the bits of its first observation sent down, which identify the
feature and are the same whichever path packed them.
"""
import collections
import zlib

import numpy as np

from msckf_amd import _lib
from msckf_amd.config import chi2_threshold

COUNTERS = collections.Counter()
BRANCHES = ("new", "tracked", "invalid", "candidate", "single_involved", "involved_initialised",
            "involved_uninitialised", "failed_triangulation_drop")


class MapError(Exception):
    def __init__(self, rc, msg):
        super().__init__("%s (rc=%d)" % (msg, rc))
        self.rc = rc


def empty(Nmax):
    return dict(ids=np.zeros(0, np.int64), obs=np.zeros((0, Nmax), bool), z=np.zeros((0, Nmax, 4)),
                p_w=np.zeros((0, 3)), init=np.zeros(0, bool))


def copy(t):
    return {k: v.copy() for k, v in t.items()}


def take(t, rows):
    return {k: v[rows].copy() for k, v in t.items()}


def mask_words(obs):
    """bool [n][Nmax] -> uint64 [n][2]"""
    n, N = obs.shape
    w = np.zeros((n, 2), np.uint64)
    for s in range(N):
        w[:, s >> 6] |= obs[:, s].astype(np.uint64) << np.uint64(s & 63)
    return w


def mask_bools(words, Nmax):
    words = np.asarray(words, np.uint64).reshape(-1, 2)
    return np.stack([((words[:, s >> 6] >> np.uint64(s & 63)) & np.uint64(1)).astype(bool) for s in range(Nmax)],
                    axis=1).reshape(len(words), Nmax)


def masked_z(t):
    """z with the entries without an observation zeroed (what msckf_map_get returns)."""
    return np.where(t["obs"][:, :, None], t["z"], 0.0)


def add_lost(t, ids, z, s, cap):
    """msckf_map_add_lost of one filter: (next table, tracked, n_before,
    candidate ids, candidate info [.][4])."""
    ids = np.asarray(ids, np.int64)
    z = np.asarray(z, float).reshape(-1, 4)
    if len(np.unique(ids)) != len(ids):
        raise MapError(-1, "an id is repeated within the message")
    n, N = len(t["ids"]), t["obs"].shape[1]
    # 1. match
    order = np.argsort(t["ids"], kind="stable")
    sid = t["ids"][order]
    k = np.minimum(np.searchsorted(sid, ids), max(n - 1, 0))
    match = (sid[k] == ids) if n else np.zeros(len(ids), bool)
    row = np.where(match, order[k] if n else 0, -1)
    new = ~match
    tracked, n_new = int(match.sum()), int(new.sum())
    # 2. append in message order
    if n + n_new > cap:
        raise MapError(-3, "%d rows exceed the map capacity %d" % (n + n_new, cap))
    row[new] = n + np.arange(n_new)
    T = dict(ids=np.concatenate([t["ids"], ids[new]]), obs=np.concatenate([t["obs"], np.zeros((n_new, N), bool)]),
             z=np.concatenate([t["z"], np.zeros((n_new, N, 4))]), p_w=np.concatenate([t["p_w"], np.zeros((n_new, 3))]),
             init=np.concatenate([t["init"], np.zeros(n_new, bool)]))
    # 3. the observation at the newest slot
    T["obs"][row, s] = True
    T["z"][row, s] = z
    # 4. classify the rows without it
    lost = ~T["obs"][:, s]
    M = T["obs"].sum(axis=1)
    cand = lost & (M >= 3)
    COUNTERS["new"] += n_new
    COUNTERS["tracked"] += tracked
    COUNTERS["invalid"] += int((lost & (M < 3)).sum())
    COUNTERS["candidate"] += int(cand.sum())
    # 5-6. remove both kinds; the descriptor in map order
    rows = np.flatnonzero(cand)
    info = np.stack([M[rows], np.zeros(len(rows), int), T["init"][rows].astype(int), rows], axis=1).astype(np.int32)
    return take(T, np.flatnonzero(~lost)), tracked, n, T["ids"][rows].copy(), info.reshape(-1, 4)


def removed_mask(slots, Nmax):
    rm = np.zeros(Nmax, bool)
    rm[np.asarray(slots, int)] = True
    return rm


def prune_select(t, rm):
    """msckf_map_prune_select of one filter: (next table, involved ids, info)."""
    T = copy(t)
    k = (T["obs"] & rm).sum(axis=1)
    M = T["obs"].sum(axis=1)
    single = k == 1
    T["obs"][single] &= ~rm
    rows = np.flatnonzero(k >= 2)
    COUNTERS["single_involved"] += int(single.sum())
    COUNTERS["involved_initialised"] += int(T["init"][rows].sum())
    COUNTERS["involved_uninitialised"] += int((~T["init"][rows]).sum())
    info = np.stack([M[rows], k[rows], T["init"][rows].astype(int), rows], axis=1).astype(np.int32)
    return T, T["ids"][rows].copy(), info.reshape(-1, 4)


def load(t, mode, rows, counts, rm=None, p_w=None):
    """The fill of msckf_map_load for one filter, as the arrays msckf_batch_load
    takes: (obs_off, obs_cam, obs_z, p_w | None, chi2 | None).  ``t``: the lost
    table (mode 0) or the current one."""
    rows, counts = np.asarray(rows, int), np.asarray(counts, int)
    for c in counts:
        dof = c - 1 if mode == _lib.MAP_LOAD_LOST else c
        if mode != _lib.MAP_LOAD_PRUNE_TRI and not 1 <= dof <= 99:
            raise MapError(-1, "no chi-square threshold for %d degrees of freedom" % dof)
    off, cams, zs, pws, chis = [0], [], [], [], []
    for i, (r, c) in enumerate(zip(rows, counts)):
        o = t["obs"][r] & rm if mode == _lib.MAP_LOAD_PRUNE_UPDATE else t["obs"][r]
        sl = np.flatnonzero(o)          # ascending cam slot
        assert len(sl) == c, "counts must be the descriptor's"
        cams.extend(sl)
        zs.extend(t["z"][r, sl])
        off.append(len(cams))
        if mode == _lib.MAP_LOAD_LOST:
            pws.append(t["p_w"][r] if t["init"][r] else np.full(3, np.nan))
            chis.append(chi2_threshold(int(c) - 1))
        elif mode == _lib.MAP_LOAD_PRUNE_UPDATE:
            given = p_w is not None and np.isfinite(p_w[i]).all()
            pws.append(np.asarray(p_w[i], float) if given else t["p_w"][r])
            chis.append(chi2_threshold(int(c)))
    tri = mode == _lib.MAP_LOAD_PRUNE_TRI
    return (np.array(off, np.int32), np.array(cams, np.int32), np.array(zs, float).reshape(-1, 4),
            None if tri else np.array(pws, float).reshape(-1, 3), None if tri else np.array(chis, float))


def prune_commit(t, rm, rows, valid, p_w):
    """msckf_map_prune_commit of one filter: the next table."""
    T = copy(t)
    rows = np.asarray(rows, int)
    valid = np.asarray(valid, bool).reshape(len(rows))
    T["p_w"][rows] = np.asarray(p_w, float).reshape(len(rows), 3)
    T["init"][rows] = valid
    COUNTERS["failed_triangulation_drop"] += int((~valid).sum())
    N = T["obs"].shape[1]
    keep = np.flatnonzero(~rm)           # slot s goes to s minus the removed slots below it
    obs, z = np.zeros_like(T["obs"]), np.zeros_like(T["z"])
    obs[:, :len(keep)] = T["obs"][:, keep]
    z[:, :len(keep)] = T["z"][:, keep]
    T["obs"], T["z"] = obs, z
    assert obs.shape[1] == N
    return T


# ------------------------------------------------------------------ stand-in --
def _feature_hash(obs_z_row):
    return zlib.crc32(np.ascontiguousarray(obs_z_row, np.float64).tobytes())


class _Pending:
    def __init__(self, res):
        self.res = res

    def get(self):
        return self.res


class RecordingContext:
    """Stand-in for _lib.Context (one filter slot is enough for MSCKF)."""

    def __init__(self, cfg=None, n_filters=1, n_cam_capacity=32, dtype=np.float64, device=0):
        self.B, self.Nmax, self.dtype = n_filters, n_cam_capacity, np.dtype(dtype)
        self.imu = [np.zeros(_lib.IMU_LEN) for _ in range(n_filters)]
        self.cam_serial = [[] for _ in range(n_filters)]   # a serial number per cam state, slot order
        self.next_serial = [0] * n_filters
        self.sent = []            # ("tri", off, cams, zs) / ("upd", off, cams, zs, nan rows, chi2, cap) / ("prune", slots)
        self.map_cap = None
        self.loaded = None

    def close(self):
        pass

    # ---- state ----
    def set_state(self, f, imu, cams, P):
        self.imu[f] = np.asarray(imu, float).copy()
        if P is not None and len(P) == 21:   # the initial covariance: first set, or an online reset
            self.cam_serial[f] = []

    def get_state(self, f, want_P=True):
        n = len(self.cam_serial[f])
        return self.imu[f].copy(), self._cams(f), (np.eye(21 + 6 * n) if want_P else None)

    def _cams(self, f):
        out = np.zeros((len(self.cam_serial[f]), _lib.CAM_LEN))
        for i, c in enumerate(self.cam_serial[f]):
            # steps of 0.1 or 0.5 m: both branches of find_redundant_cam_states occur
            x = sum(0.1 if zlib.crc32(b"%d" % k) % 3 else 0.5 for k in range(c + 1))
            out[i, 0:4] = out[i, 7:11] = [0, 0, 0, 1]
            out[i, 4] = x
        return out

    def readback(self, filters, want_cams=True, cov=None):
        imu = np.array([self.imu[f] for f in filters])
        cv = np.zeros((len(filters), cov[1])) if cov else None
        return imu, [self._cams(f) for f in filters], cv

    def cov_diag(self, f, i0, n):
        return np.zeros(n)

    def propagate(self, f, dt, gyro, acc):
        pass

    def augment(self, f):
        self.cam_serial[f].append(self.next_serial[f])
        self.next_serial[f] += 1

    def prune(self, f, slots):
        self.sent.append(("prune", np.asarray(slots, np.int32).copy()))
        for s in sorted((int(x) for x in slots), reverse=True):
            del self.cam_serial[f][s]

    # ---- the answers: a fixed function of the feature ----
    @staticmethod
    def _tri_answer(off, zs):
        nf = len(off) - 1
        p, ok = np.zeros((nf, 3)), np.zeros(nf, bool)
        for i in range(nf):
            h = _feature_hash(zs[off[i]])
            ok[i] = h % 5 != 0
            p[i] = [h % 7, h % 11, 1.0 + h % 3]
        return p, ok

    def _upd_answer(self, off, zs, pw, chi2, row_cap):
        nf = len(off) - 1
        p_t, ok_t = self._tri_answer(off, zs)
        nan = ~np.isfinite(pw).all(axis=1)
        valid = np.where(nan, ok_t, True)
        p = np.where(nan[:, None], p_t, pw)
        gam = np.array([(_feature_hash(zs[off[i]]) % 100) / 8.0 for i in range(nf)])
        acc, rows = np.zeros(nf, bool), 0
        for i in range(nf):
            if not valid[i]:
                continue
            if gam[i] < chi2[i]:
                acc[i] = True
                rows += 4 * (off[i + 1] - off[i]) - 3
            if row_cap and rows > row_cap:
                break
        return acc, gam, p, valid, rows

    def triangulate(self, f, off, cams, zs):
        off, cams, zs = np.asarray(off, np.int32), np.asarray(cams, np.int32), np.asarray(zs, float).reshape(-1, 4)
        self.sent.append(("tri", off.copy(), cams.copy(), zs.copy()))
        return self._tri_answer(off, zs)

    def update_async(self, f, off, cams, zs, pw, chi2, row_cap=0):
        off, cams, zs = np.asarray(off, np.int32), np.asarray(cams, np.int32), np.asarray(zs, float).reshape(-1, 4)
        pw, chi2 = np.asarray(pw, float).reshape(-1, 3), np.asarray(chi2, float)
        self.sent.append(("upd", off.copy(), cams.copy(), zs.copy(), ~np.isfinite(pw).all(axis=1), chi2.copy(),
                          int(row_cap)))
        return _Pending(self._upd_answer(off, zs, pw, chi2, row_cap))

    def settle(self):
        pass

    # ---- the map calls: the numpy reference ----
    def map_create(self, cap):
        self.map_cap = cap
        self.tab = [empty(self.Nmax) for _ in range(self.B)]
        self.lost = [None] * self.B
        self.rm = [None] * self.B

    def map_clear(self, filters):
        for f in filters:
            self.tab[f] = empty(self.Nmax)

    def map_get(self, f):
        t = self.tab[f]
        return t["ids"].copy(), mask_words(t["obs"]), masked_z(t), t["p_w"].copy(), t["init"].copy()

    def map_add_lost(self, filters, msg_off, ids, z):
        out = []
        for w, f in enumerate(filters):
            a, b = msg_off[w], msg_off[w + 1]
            nxt, tracked, nb, cid, info = add_lost(self.tab[f], ids[a:b], z[a:b], len(self.cam_serial[f]) - 1,
                                                   self.map_cap)
            self.lost[f], self.tab[f] = self.tab[f], nxt
            out.append((tracked, nb, cid, info))
        return out

    def map_prune_select(self, filters, slot_off, slots):
        out = []
        for w, f in enumerate(filters):
            self.rm[f] = removed_mask(slots[slot_off[w]:slot_off[w + 1]], self.Nmax)
            self.tab[f], iid, info = prune_select(self.tab[f], self.rm[f])
            out.append((iid, info))
        return out

    def map_load(self, mode, filters, feat_off, rows, counts, p_w=None):
        assert len(filters) == 1
        f = filters[0]
        src = self.lost[f] if mode == _lib.MAP_LOAD_LOST else self.tab[f]
        self.loaded = load(src, mode, rows, counts, self.rm[f], p_w)
        return {f: (0, len(rows))}

    def batch_triangulate(self):
        off, cams, zs, _, _ = self.loaded
        self.sent.append(("tri", off.copy(), cams.copy(), zs.copy()))
        self._res = self._tri_answer(off, zs)

    def batch_results(self):
        p, ok = self._res
        return None, None, p, ok, None

    def batch_update(self, row_cap=0, triangulate=True):
        off, cams, zs, pw, chi2 = self.loaded
        self.sent.append(("upd", off.copy(), cams.copy(), zs.copy(), ~np.isfinite(pw).all(axis=1), chi2.copy(),
                          int(row_cap)))
        self._pend = _Pending(self._upd_answer(off, zs, pw, chi2, row_cap))

    def pending(self, ranges):
        return [self._pend for _ in ranges]

    def map_prune_commit(self, filters, ent_off, rows, valid, p_w):
        for w, f in enumerate(filters):
            a, b = ent_off[w], ent_off[w + 1]
            self.tab[f] = prune_commit(self.tab[f], self.rm[f], rows[a:b], valid[a:b], np.asarray(p_w)[a:b])
