"""The landmark archive of a filter (include/msckf_odometry.h): the features that
left the map through an accepted lost-feature update, with their triangulated
positions, in a ring of ``cap`` rows.

``landmarks="device"`` keeps the ring in device memory, filled by
``msckf_landmarks_archive`` inside the update's call chain; ``HostRing`` below is
the same ring in numpy, filled from the deferred update results the host
receives anyway (``landmarks="host"``) -- the statement the device mode equals.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

# ids int64 [n], p_w float64 [n][3], n_obs int32 [n], gamma float64 [n], stamp int32 [n]: the archived rows with
# sequence numbers first_seq, first_seq + 1, ... (oldest first), then -- if asked -- the live rows (stamp -1,
# gamma NaN); next_seq: the number of rows ever archived.
Landmarks = namedtuple("Landmarks", ["ids", "p_w", "n_obs", "gamma", "stamp", "first_seq", "next_seq"])

MODES = (None, "host", "device")


def check_mode(landmarks, device_map):
    if landmarks not in MODES:
        raise ValueError("landmarks = %r, expected one of %r" % (landmarks, MODES))
    if landmarks == "device" and not device_map:
        raise ValueError("landmarks='device' needs device_map=True: the archive is filled from the device map's "
                         "lost table")


class HostRing:
    """The ring of msckf_odometry.h in numpy."""

    def __init__(self, cap):
        self.cap = int(cap)
        self.ids = np.zeros(self.cap, np.int64)
        self.p_w = np.zeros((self.cap, 3))
        self.n_obs = np.zeros(self.cap, np.int32)
        self.gamma = np.zeros(self.cap)
        self.stamp = np.zeros(self.cap, np.int32)
        self.seq = 0

    def clear(self):
        self.seq = 0

    def append(self, ids, p_w, n_obs, gamma, stamp):
        """Rows in the order given; ``stamp``: one value for all of them."""
        ids = np.asarray(ids, np.int64)
        k = (self.seq + np.arange(len(ids))) % self.cap
        self.ids[k] = ids
        self.p_w[k] = np.asarray(p_w, float).reshape(-1, 3)
        self.n_obs[k] = n_obs
        self.gamma[k] = gamma
        self.stamp[k] = stamp
        self.seq += len(ids)

    def get(self, first_seq=0, max_rows=None):
        """msckf_landmarks_get: (ids, p_w, n_obs, gamma, stamp, first, seq)."""
        lo = min(max(int(first_seq), self.seq - self.cap, 0), self.seq)
        n = self.seq - lo if max_rows is None else min(int(max_rows), self.seq - lo)
        k = (lo + np.arange(n)) % self.cap
        return self.ids[k], self.p_w[k], self.n_obs[k], self.gamma[k], self.stamp[k], lo, self.seq


def with_live(rows, ids, p_w, n_obs):
    """``rows`` (a ``get`` result) as Landmarks, the live rows appended."""
    a_ids, a_p, a_n, a_g, a_s, first, seq = rows
    n = len(ids)
    return Landmarks(np.concatenate([a_ids, np.asarray(ids, np.int64).reshape(n)]),
                     np.concatenate([a_p, np.asarray(p_w, float).reshape(n, 3)]),
                     np.concatenate([a_n, np.asarray(n_obs, np.int32).reshape(n)]),
                     np.concatenate([a_g, np.full(n, np.nan)]),
                     np.concatenate([a_s, np.full(n, -1, np.int32)]), int(first), int(seq))
