"""CPU stand-ins for both ends of msckf_amd.vio (include/msckf_handoff.h
restated around the stand-ins of msckf_tracks.h and msckf_map.h):

``VioOracleFrontend``: tests/frontend_tracks_ref.py's TracksOracleFrontend with
the lanes' messages -- ``tracks_msg_put`` / ``tracks_msg_get`` and
``tracks_step(to_message=True)``, which keeps ids / uv as the named lanes'
messages and returns None in their place; ``tracks_put`` and every step clear
the valid flag of the lanes they name.  A step in message form is logged as
``tracks_step_msg``.

``VioRecordingContext``: tests/feature_map_ref.py's RecordingContext with
``map_add_lost_tracks`` -- the lane's message fetched from the stand-in
front-end, then the numpy ``add_lost`` -- plus the batched calls
scheduler.MultiMSCKF serves its requests with and the keyframe choice of
tests/keyframe_ref.py.  ``map_calls`` logs the add_lost calls by name.

The oracle's LK makes a 30-frame run take most of a minute, and the tests
compare three runs of the same stream.  ``step`` is a pure function of the
images in the slots, the tables and the lanes' arguments, so the stand-in
remembers its results by those inputs' bytes (``STEP_MEMO``)."""
import hashlib

import numpy as np

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
import feature_map_ref as fr
import frontend_tracks_ref as tr
import keyframe_ref as kr

STEP_MEMO = {}


def _digest(parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, (tuple, list)):
            h.update(_digest(p))
        elif p is None:
            h.update(b"None")
        else:
            a = np.ascontiguousarray(p)
            h.update(str((a.dtype, a.shape)).encode() + a.tobytes())
    return h.digest()


class VioOracleFrontend(tr.TracksOracleFrontend):
    def tracks_create(self, n_lanes, cap, grid_row, grid_col, grid_min, grid_max):
        super().tracks_create(n_lanes, cap, grid_row, grid_col, grid_min, grid_max)
        self.messages = {i: None for i in range(n_lanes)}     # None: no valid message

    def tracks_put(self, lane, ids, lifetimes, cam0, cam1, next_id):
        super().tracks_put(lane, ids, lifetimes, cam0, cam1, next_id)
        self.messages[lane] = None

    def tracks_msg_put(self, lane, ids, uv):
        self.calls.append("tracks_msg_put")
        ids = np.asarray(ids, np.int64).reshape(-1).copy()
        uv = np.asarray(uv, np.float64).reshape(-1, 4).copy()
        if lane not in self.messages or len(ids) > self.tracks_cap or len(np.unique(ids)) != len(ids):
            self._fail("bad lane, n or a repeated id")
        self.messages[lane] = (ids, uv)

    def tracks_msg_get(self, lane):
        self.calls.append("tracks_msg_get")
        m = self.messages[lane]
        if m is None:
            return False, np.zeros(0, np.int64), np.zeros((0, 4))
        return True, m[0].copy(), m[1].copy()

    def _step_key(self, lanes, threshold, max_kp, inlier_error, n_hyp, lk):
        parts = [np.array([self.W, self.H, threshold, max_kp, n_hyp, *self.grid]), np.array([inlier_error]),
                 np.array(sorted(lk.items()), dtype="U32")]
        for a in lanes:
            t = self.tables[a.lane]
            parts += [np.array([a.lane, t.next_id]), t.ids, t.life, t.cam0, t.cam1,
                      [self.slots[s] for s in (a.slot_prev, a.slot_c0, a.slot_c1)],
                      a.Hpred, a.cam0[0], np.array([a.cam0[1], a.cam1[1]]), a.cam0[2], a.cam1[0], a.cam1[2], a.R_guess,
                      a.E, np.array([a.stereo_threshold]), a.ransac]
        return _digest(parts)

    def tracks_step(self, lanes, threshold, max_kp=1 << 16, inlier_error=0.0, n_hyp=0, to_message=False, **lk):
        key = self._step_key(lanes, threshold, max_kp, inlier_error, n_hyp, lk)
        if key in STEP_MEMO:
            self.calls.append("tracks_step")
            res, nxt = STEP_MEMO[key]
            self.tables.update(nxt)
        else:
            before = dict(self.tables)
            res = super().tracks_step(lanes, threshold, max_kp, inlier_error, n_hyp, **lk)
            STEP_MEMO[key] = (res, {a.lane: self.tables[a.lane] for a in lanes})
            assert all(self.tables[l] is before[l] for l in before if l not in [a.lane for a in lanes])
        for a in lanes:
            self.messages[a.lane] = None
        if not to_message:
            return [fe_mod.TracksResult(r.n, r.ids.copy(), r.uv.copy(), r.counters.copy(), r.n_total, r.next_id)
                    for r in res]
        self.calls[-1] = "tracks_step_msg"
        for a, r in zip(lanes, res):
            self.messages[a.lane] = (r.ids.copy(), r.uv.copy())
        return [fe_mod.TracksResult(r.n, None, None, r.counters.copy(), r.n_total, r.next_id) for r in res]


class VioRecordingContext(fr.RecordingContext):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.map_calls = []

    # ---- the hand-off ----
    def map_add_lost(self, filters, msg_off, ids, z):
        self.map_calls.append("map_add_lost")
        return super().map_add_lost(filters, msg_off, ids, z)

    def map_add_lost_tracks(self, filters, fe, lanes):
        self.map_calls.append("map_add_lost_tracks")
        if len(set(lanes)) != len(lanes) or len(lanes) != len(filters):
            raise _lib.MsckfError("msckf: bad lane list (rc=-1)")
        msgs = []
        for lane in lanes:
            m = getattr(fe, "messages", {}).get(lane)
            if m is None:
                raise _lib.MsckfError("msckf: lane %d has no valid message (rc=-1)" % lane)
            msgs.append(m)
        off = np.cumsum([0] + [len(m[0]) for m in msgs])
        return fr.RecordingContext.map_add_lost(self, filters, off, np.concatenate([m[0] for m in msgs]),
                                                np.concatenate([m[1] for m in msgs]).reshape(-1, 4))

    # ---- what scheduler.MultiMSCKF batches ----
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

    def keyframe_select(self, filters, rates):
        out = []
        for f, rate in zip(filters, rates):
            ch = kr.choice(self._cams(f), rate)
            (iid, info), = self.map_prune_select([f], [0, 2], ch.slots)
            out.append((ch.slots, iid, info))
        return out
