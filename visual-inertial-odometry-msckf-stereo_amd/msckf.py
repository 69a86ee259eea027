"""Drop-in host class for the reference filter (MSCKF/msckf.py:104-908).

``MSCKF(config)`` keeps the reference's public API -- ``imu_callback(imu_msg)``
and ``feature_callback(feature_msg) -> vio_result | None`` with the same
message tuples -- so it sits behind the existing stereo front-end unchanged.

What stays in Python (host bookkeeping, as SURVEY.md section 8(b) prescribes):
the IMU message buffer walk, the feature map and its observation dicts, cam-id
<-> slot bookkeeping, the chi2 table lookup, the ordered 1500-row cap inputs,
keyframe selection, the online-reset decision and ``publish``.
What runs on the GPU (through the C-ABI, libmsckf_hip.so): IMU covariance
propagation, state augmentation, triangulation, measurement Jacobians +
nullspace projection, gating, stacking, compression of the stacked rows
(information assembly), the Kalman update and covariance compaction.  There is
no CPU fallback.  With ``device_map=True`` the feature map is device state as
well (include/msckf_map.h): adding observations, the lost-feature and prune
selections and the packing of an update's observations are device calls, the
host keeps the decisions' descriptors (ids, track lengths) for its logs, and a
frame's message may be a ``TrackMessage`` that names where the front-end left
it on the device (include/msckf_handoff.h); with
``device_keyframes=True`` the keyframe selection is part of the prune select's
device call too (include/msckf_keyframes.h).  ``landmarks`` / ``odometry`` add
the outputs of include/msckf_odometry.h: the archive of the features that left
the map through an accepted update, and the published pose's covariance.
``zupt`` adds the zero-velocity update of include/msckf_zupt.h: once per frame,
between propagation and augmentation, gated on the device.  ``aiding`` adds the
aiding fixes of include/msckf_aid.h: external position, velocity, body-frame
velocity and heading messages (``aiding_callback``), applied at the same point.
``anchors`` adds the anchor fixes of include/msckf_anchor.h: stereo observations
of points with known world positions (``anchor_callback``), applied behind them.

Every device interaction of a frame is expressed as a request yielded by a
step generator (``_frame_steps``); ``feature_callback`` serves the requests
one by one on this filter's slot, while ``scheduler.MultiMSCKF`` advances many
filters' generators in lock step and serves each kind of request for all of
them with one batched launch.  Both paths run the same host logic.

Differences from the reference that are deliberate:
* the reference's IMU-buffer race between the IMU and vio threads
  (msckf.py:173 vs 287) is removed -- every call holds the context lock;
* class-level globals (gravity, next ids, cam0->cam1 extrinsics; quirk Q7) are
  per-instance, so several filters can live in one process.
"""
from __future__ import annotations

import threading
from collections import OrderedDict, namedtuple

import numpy as np

from . import _lib
from .config import ANCHOR_MAX, CHI2_05, AidingConfig, AnchorConfig, FilterConfig, ZuptConfig, chi2_threshold
from .geometry import Isometry3d, from_two_vectors, to_quaternion, to_rotation
from .landmarks import HostRing, Landmarks, check_mode, with_live

VioResult = namedtuple("vio_result", ["timestamp", "pose", "velocity", "cam0_pose"])
# What feature_callback returns with odometry=True: the vio_result's fields and the 6 x 6 covariance of the pose
# (orientation error angle, then position) and the 3 x 3 of the velocity, both rotated by T_imu_body's rotation
# (include/msckf_odometry.h states the frame).
VioOdometry = namedtuple("vio_odometry", ["timestamp", "pose", "velocity", "cam0_pose", "pose_covariance",
                                          "velocity_covariance"])
# A feature message as arrays: ids int64 [n], uv float64 [n][4] (u0 v0 u1 v1).
# Accepted wherever the reference's feature_msg tuple is.
# ``motion``: None, or the front-end's motion record (n, d2) of the frame (include/msckf_standstill.h)
FeatureArrays = namedtuple("FeatureArrays", ["timestamp", "ids", "uv", "motion"], defaults=(None,))
# A feature message that stayed on the device (include/msckf_handoff.h): the n-row message of lane
# ``lane`` of the front-end context ``frontend`` (a frontend.Frontend).  Accepted with device_map=True only.
TrackMessage = namedtuple("TrackMessage", ["timestamp", "frontend", "lane", "n"])


def _cue_source(feature_msg):
    """Where the frame's vision cue comes from (msckf_standstill.h): (front-end
    context, lane, None) for a message on the device -- its lane's motion record
    is read there, and a lane's first frame has none -- or (None, n, d2) for the
    host: an array message's ``motion``, else (-1, NaN), "no record"."""
    if isinstance(feature_msg, TrackMessage):
        return (feature_msg.frontend, int(feature_msg.lane), None)
    motion = getattr(feature_msg, "motion", None)
    if motion is None:
        return (None, -1, float("nan"))
    return (None, int(motion[0]), np.float32(motion[1]))


def message_arrays(feature_msg):
    """(ids int64 [n], uv float64 [n][4]) of either message type."""
    if isinstance(feature_msg, FeatureArrays):
        return (np.ascontiguousarray(feature_msg.ids, np.int64),
                np.ascontiguousarray(feature_msg.uv, np.float64).reshape(-1, 4))
    fs = feature_msg.vio_features
    ids = np.fromiter((f.id for f in fs), np.int64, len(fs))
    uv = np.array([(f.u0, f.v0, f.u1, f.v1) for f in fs], np.float64).reshape(-1, 4)
    return ids, uv


class Feature:
    """Host record of a map feature (reference Feature fields, feature.py:15-31)."""
    __slots__ = ("id", "observations", "position", "is_initialized")

    def __init__(self, fid):
        self.id = fid
        self.observations: "OrderedDict[int, np.ndarray]" = OrderedDict()
        self.position = np.zeros(3)
        self.is_initialized = False


_CHI2 = np.array(CHI2_05[:99])


def _chi2_of(dofs):
    """chi2_threshold of an array of dofs (KeyError outside 1..99, as the dict)."""
    dofs = np.asarray(dofs, np.int64)
    bad = (dofs < 1) | (dofs > 99)
    if bad.any():
        raise KeyError(int(dofs[bad][0]))
    return _CHI2[dofs - 1]


def check_motion(observations, cams, threshold):
    """Feature.check_motion (feature.py:124-165): is the translation between the
    first and the last observing cam, orthogonal to the first observation's
    ray, above ``threshold``?  ``cams``: cam id -> dict(q, p).  A negative
    threshold (the EuRoC config, config.py:10) accepts every feature."""
    if threshold < 0:
        return True
    ids = list(observations.keys())
    c0, c1 = cams[ids[0]], cams[ids[-1]]
    d = np.array([*observations[ids[0]][:2], 1.0])
    d = to_rotation(np.asarray(c0["q"], float)).T @ (d / np.linalg.norm(d))
    tr = np.asarray(c1["p"], float) - np.asarray(c0["p"], float)
    orth = tr - (tr @ d) * d
    return bool(np.linalg.norm(orth) > threshold)


class MSCKF:
    ROW_CAP = 1500   # msckf.py:678

    def __init__(self, config=None, dtype=np.float64, device=0, cam_capacity=None, ctx=None, slot=0,
                 device_map=False, map_capacity=1024, device_keyframes=False, landmarks=None,
                 landmark_capacity=4096, odometry=False, zupt=None, aiding=None, anchors=None):
        """``device_map``: keep the feature map in the context's tables
        (msckf_map.h) instead of ``map_server``'s dicts; ``map_capacity``: rows
        per filter.  A shared ``ctx`` must already have its tables.
        ``device_keyframes`` (with ``device_map``): a prune frame's cam states
        are chosen on the device, in the prune select's call
        (msckf_keyframes.h), instead of from a read of the cam poses.
        ``landmarks``: archive the features that leave the map through an
        accepted lost-feature update (``landmarks()``), ``landmark_capacity``
        rows: "device" (with ``device_map``) fills the ring on the device
        inside the update's calls (msckf_odometry.h), "host" keeps it in numpy
        from the deferred results.  A shared ``ctx`` must already have its
        rings.  ``odometry``: the callbacks return ``VioOdometry`` -- the
        frame's read brings the pose and velocity covariance along.
        ``zupt`` (a ``ZuptConfig``; None: off): the zero-velocity update
        (msckf_zupt.h) of every frame that propagated IMU samples, with their
        means, between propagation and augmentation; the device gates it, the
        decisions are read with the frame's state into ``zupt_log``.
        ``aiding`` (an ``AidingConfig``; None: off): the fixes given to
        ``aiding_callback`` are applied by the frame that follows them within
        ``max_age`` (msckf_aid.h), after propagation (and the zero-velocity
        update) and before augmentation; the device gates them, the decisions
        are read with the frame's state into ``aid_log``.  With
        ``AidingConfig(delayed=True)`` a fix older than ``max_age`` is not dropped
        but applied at its own timestamp, on the pose interpolated between the two
        window clones that bracket it (msckf_aid_delayed.h; position and
        direction rows only), oldest first and before the frame's own fix; the
        records go to ``aid_delayed_log``, what no path takes to
        ``aid_dropped_log``.
        ``anchors`` (an ``AnchorConfig``; None: off): the messages given to
        ``anchor_callback`` are applied by the frame whose timestamp lies within
        ``time_tol`` of theirs (msckf_anchor.h), after propagation (and the
        zero-velocity update and the aiding fix) and before augmentation; the
        device gates every anchor, the records are read with the frame's state
        into ``anchor_log``."""
        if config is None:
            config = FilterConfig()
        elif not isinstance(config, FilterConfig):
            config = FilterConfig.from_reference(config)
        self.config = config
        self.device_map = bool(device_map)
        self.device_keyframes = bool(device_keyframes)
        check_mode(landmarks, self.device_map)
        self.landmark_mode = landmarks
        self.odometry = bool(odometry)
        if zupt is not None and not isinstance(zupt, ZuptConfig):
            raise TypeError("zupt must be a ZuptConfig or None, not %r" % (zupt,))
        self.zupt = zupt
        self._zupt_prm = zupt.params() if zupt is not None else None   # checks the row names and chi2's table
        # the vision cue (msckf_standstill.h): the frame's message names or carries the front-end's motion record
        self._cue_prm = zupt.vision.params() if zupt is not None and zupt.vision is not None else None
        # (frame, applied, gamma), one per zero-velocity update enqueued; with zupt.vision
        # (frame, applied, gamma, cue, n, d2) -- the cue's status and record as the device saw them
        self.zupt_log = []
        self._zupt_count = 0
        if aiding is not None and not isinstance(aiding, AidingConfig):
            raise TypeError("aiding must be an AidingConfig or None, not %r" % (aiding,))
        self.aiding = aiding
        self._aid_prm = aiding.params() if aiding is not None else None   # checks R_body, dir_w, world_from_ext
        self._aid_buffer = []              # AidingFix messages not yet past a frame
        self.aid_log = []                  # (frame, rows, applied, gamma), one per fix enqueued
        self._aid_count = 0
        # the delayed path (msckf_aid_delayed.h), AidingConfig(delayed=True)
        self.aid_delayed_log = []          # (frame, rows, applied, gamma, slot, lambda, status), one per fix enqueued
        self.aid_dropped_log = []          # (frame, timestamp, reason): fixes no path took, and VEL / BVEL rows left out
        self._aid_delayed_count = 0
        if anchors is not None and not isinstance(anchors, AnchorConfig):
            raise TypeError("anchors must be an AnchorConfig or None, not %r" % (anchors,))
        self.anchors = anchors
        self._anchor_prm = anchors.params(config.observation_noise) if anchors is not None else None   # checks it
        self._anchor_buffer = []           # (timestamp, msckf_anchor_t records) not yet past a frame, in time order
        self.anchor_log = []               # (frame, n, used, applied), one per message enqueued
        self.anchor_dropped = 0            # messages no frame matched
        self._anchor_count = 0
        if self.device_keyframes and not self.device_map:
            raise ValueError("device_keyframes=True needs device_map=True: the choice is part of the map's prune "
                             "select")
        if self.device_map and config.optimization.translation_threshold >= 0:
            raise ValueError("device_map=True needs optimization.translation_threshold < 0 (it is %r): check_motion "
                             "reads the cam poses on the host" % (config.optimization.translation_threshold,))
        cap = cam_capacity or (config.max_cam_state_size + 2)
        self._own_ctx = ctx is None
        self.ctx = ctx if ctx is not None else _lib.Context(config, n_filters=1, n_cam_capacity=cap, dtype=dtype,
                                                            device=device)
        self.slot = slot
        self._lock = threading.RLock()
        self.imu_msg_buffer = []
        if self.device_map:   # map_server is then a snapshot read from the device (a property of a subclass)
            self.__class__ = _device_map_class(type(self))
            if self._own_ctx:
                self.ctx.map_create(map_capacity)
                if landmarks == "device":
                    self.ctx.landmarks_create(landmark_capacity)
        else:
            self.map_server: "OrderedDict[int, Feature]" = OrderedDict()
        self.cam_ids: list = []            # cam-state ids in slot order (oldest first)
        self.cam_times: list = []          # their frame times, in step with cam_ids
        self.imu_timestamp = None
        self.imu_id = None
        self._next_id = 0
        self.tracking_rate = None
        self.is_gravity_set = False
        self.is_first_img = True
        self.gate_log = []                 # (frame, dof, rows, accepted) like tools/gen_golden.py
        self.gamma_log = []                # (feature id, gamma), one per gate_log entry
        self.shape_log = []
        self.reset_log = []                # frames after which online_reset fired
        self._deferred = []                # (Pending, callback): update results not read back yet
        self._n_published = 0
        self._ring = HostRing(landmark_capacity) if landmarks == "host" else None
        T_cam0_imu = np.linalg.inv(config.T_imu_cam0)
        self._T_imu_body = Isometry3d(config.T_imu_body[:3, :3], config.T_imu_body[:3, 3])
        imu = _lib.pack_imu(q=[0, 0, 0, 1], p=np.zeros(3), v=config.velocity, bg=np.zeros(3), ba=np.zeros(3),
                            q_null=[0, 0, 0, 1], p_null=np.zeros(3), v_null=np.zeros(3),
                            R_imu_cam0=T_cam0_imu[:3, :3].T, t_cam0_imu=T_cam0_imu[:3, 3],
                            gravity=config.gravity, alias=False)
        self.ctx.set_state(self.slot, imu, None, self._initial_cov())

    # ------------------------------------------------------------ helpers --
    def _initial_cov(self):
        """msckf.py:820-830"""
        c = self.config
        P = np.zeros((21, 21))
        P[3:6, 3:6] = c.gyro_bias_cov * np.eye(3)
        P[6:9, 6:9] = c.velocity_cov * np.eye(3)
        P[9:12, 9:12] = c.acc_bias_cov * np.eye(3)
        P[15:18, 15:18] = c.extrinsic_rotation_cov * np.eye(3)
        P[18:21, 18:21] = c.extrinsic_translation_cov * np.eye(3)
        return P

    def imu_state(self):
        imu, _, _ = self.ctx.get_state(self.slot, want_P=False)
        return _lib.unpack_imu(imu)

    def cam_states(self):
        """OrderedDict cam id -> dict(q, p, q_null) in slot order."""
        _, cams, _ = self.ctx.get_state(self.slot, want_P=False)
        return self._cam_dict(cams)

    def _cam_dict(self, cams):
        return OrderedDict((cid, dict(q=cams[i, 0:4], p=cams[i, 4:7], q_null=cams[i, 7:11]))
                           for i, cid in enumerate(self.cam_ids))

    def state_cov(self):
        return self.ctx.get_state(self.slot, want_P=True)[2]

    def _map_snapshot(self):
        """Read-only copy of the device table in map_server's form."""
        ids, mask, z, p_w, init = self.ctx.map_get(self.slot)
        out = OrderedDict()
        for i, fid in enumerate(ids):
            feat = Feature(int(fid))
            for s, cid in enumerate(self.cam_ids):
                if (int(mask[i, s >> 6]) >> (s & 63)) & 1:
                    feat.observations[cid] = tuple(float(v) for v in z[i, s])
            feat.position = p_w[i].copy()
            feat.is_initialized = bool(init[i])
            out[feat.id] = feat
        return out

    # ------------------------------------------------- device request server --
    def _serve(self, req):
        """Executes one request of the step generators on this filter's slot."""
        kind, f, ctx = req[0], self.slot, self.ctx
        if kind == "propagate":
            return ctx.propagate(f, req[1], req[2], req[3])
        if kind == "augment":
            return ctx.augment(f)
        if kind == "zupt" and len(req) > 3:   # (kind, means, the frame's cue source): msckf_standstill.h
            fe, a, b = req[3]
            if fe is not None:
                return ctx.zupt_batch_cued([f], req[1], req[2], self._zupt_prm, self._cue_prm, fe=fe, lanes=[a])
            return ctx.zupt_batch_cued([f], req[1], req[2], self._zupt_prm, self._cue_prm, cue_n=[a], cue_d2=[b])
        if kind == "zupt":   # (kind, mean angular rate, mean specific force)
            return ctx.zupt_batch([f], req[1], req[2], self._zupt_prm)
        if kind == "zupt_results" and self._cue_prm is not None:   # the six records in one read
            app, gam, cnt, cue, cn, cd = ctx.zupt_cue_results([f])
            return bool(app[0]), float(gam[0]), int(cnt[0]), int(cue[0]), int(cn[0]), float(cd[0])
        if kind == "zupt_results":
            app, gam, cnt = ctx.zupt_results([f])
            return bool(app[0]), float(gam[0]), int(cnt[0])
        if kind == "aid":   # (kind, the frame's merged fix)
            return ctx.aid_batch([f], [req[1]], self._aid_prm)
        if kind == "aid_results":
            app, gam, rows, cnt = ctx.aid_results([f])
            return bool(app[0]), float(gam[0]), int(rows[0]), int(cnt[0])
        if kind == "aid_delayed":   # (kind, one late fix on its clone pair)
            return ctx.aid_delayed_batch([f], [req[1]], self._aid_prm)
        if kind == "aid_delayed_results":
            app, gam, rows, sta, cnt = ctx.aid_delayed_results([f])
            return bool(app[0]), float(gam[0]), int(rows[0]), int(sta[0]), int(cnt[0])
        if kind == "anchor":   # (kind, the frame's msckf_anchor_t records)
            return ctx.anchor_batch([f], [req[1]], self._anchor_prm)
        if kind == "anchor_results":
            app, used, rows, cnt = ctx.anchor_results([f])
            return bool(app[0]), int(used[0]), int(rows[0]), int(cnt[0])
        if kind == "triangulate":
            return ctx.triangulate(f, req[1], req[2], req[3])
        if kind == "update":
            return ctx.update_async(f, *req[1:])
        if kind == "states" and len(req) > 3:   # ("states", i0, n, R_body): the read of msckf_readback_odom
            imu, cams, cv, pc, vc = ctx.readback_odom([f], req[3], cov=req[1:3])
            return imu[0], cams[0], None if cv is None else cv[0], pc[0], vc[0]
        if kind == "states":   # ("states"[, i0, n]): one read, with P's diagonal [i0, i0 + n) if asked
            imu, cams, cv = ctx.readback([f], cov=req[1:3] if len(req) > 1 else None)
            return (imu[0], cams[0]) if cv is None else (imu[0], cams[0], cv[0])
        if kind == "prune":
            return ctx.prune(f, req[1])
        if kind == "cov_diag":
            return ctx.cov_diag(f, req[1], req[2])
        if kind == "set_state":
            return ctx.set_state(f, req[1], req[2], req[3])
        if kind == "map_add_lost":
            return ctx.map_add_lost([f], [0, len(req[1])], req[1], req[2])[0]
        if kind == "map_add_lost_tracks":   # (kind, front-end context, lane)
            return ctx.map_add_lost_tracks([f], req[1], [req[2]])[0]
        if kind == "map_prune_select":
            return ctx.map_prune_select([f], [0, len(req[1])], req[1])[0]
        if kind == "map_keyframe_select":   # (kind, tracking rate)
            return ctx.keyframe_select([f], [req[1]])[0]
        if kind == "map_triangulate":
            ctx.map_load(_lib.MAP_LOAD_PRUNE_TRI, [f], [0, len(req[1])], req[1], req[2])
            ctx.batch_triangulate()
            _, _, p, v, _ = ctx.batch_results()
            return p, v
        if kind == "map_update":   # (kind, form, rows, counts, p_w, triangulate, row cap)
            ctx.map_load(req[1], [f], [0, len(req[2])], req[2], req[3], req[4])
            ctx.batch_update(row_cap=req[6], triangulate=req[5])
            if self.landmark_mode == "device" and req[1] == _lib.MAP_LOAD_LOST:   # directly behind the update
                ctx.landmarks_archive([f], [0, len(req[2])], req[2], [self._n_published])
            return ctx.pending([(f, 0, len(req[2]))])[0]
        if kind == "map_prune_commit":
            return ctx.map_prune_commit([f], [0, len(req[1])], req[1], req[2], req[3])
        if kind == "map_clear":
            return ctx.map_clear([f])
        raise ValueError("unknown request %r" % (kind,))

    def _settle(self):
        """Applies the deferred update results (gate / shape logs, new
        positions) in request order.  Called at the frame's synchronisation
        points -- after a ``states`` read or a ``map_keyframe_select``, when the
        device has drained anyway."""
        d, self._deferred = self._deferred, []
        for pend, fn in d:
            fn(*pend.get())

    def _drive(self, gen):
        try:
            req = next(gen)
            while True:
                req = gen.send(self._serve(req))
        except StopIteration as e:
            return e.value

    # ----------------------------------------------------------- callbacks --
    def imu_callback(self, imu_msg):
        """msckf.py:166-178"""
        with self._lock:
            self.imu_msg_buffer.append(imu_msg)
            if not self.is_gravity_set and len(self.imu_msg_buffer) >= 200:
                self._drive(self._initialize_gravity_and_bias())
                self.is_gravity_set = True

    def aiding_callback(self, fix):
        """Buffers an ``AidingFix``; the next frame at or after its timestamp
        applies it if it is no older than ``max_age`` by then."""
        if self.aiding is None:
            raise ValueError("aiding_callback needs MSCKF(aiding=AidingConfig())")
        with self._lock:
            buf = self._aid_buffer   # kept in time order; messages usually arrive so
            k = len(buf)
            while k > 0 and buf[k - 1].timestamp > fix.timestamp:
                k -= 1
            buf.insert(k, fix)

    def _take_fix(self, t_frame):
        """The frame's merged fix as a msckf_aid_fix_t (None without one); the
        fixes up to the frame time leave the buffer."""
        buf = self._aid_buffer
        if not buf or buf[0].timestamp > t_frame:
            return None
        n = 1
        while n < len(buf) and buf[n].timestamp <= t_frame:
            n += 1
        held = [f for f in buf[:n] if f.received is not None and f.received > t_frame]   # not handed over yet
        seen = [f for f in buf[:n] if not (f.received is not None and f.received > t_frame)]
        self._aid_buffer = held + buf[n:]
        merged = self.aiding.merge(seen, t_frame)
        return _lib.aid_fix(*merged) if merged is not None else None

    def _take_fixes(self, t_frame):
        """``_take_fix`` with ``AidingConfig.route`` in front (delayed=True):
        (the late fixes as [(msckf_aid_delayed_fix_t, slot, lambda)], oldest
        first, the frame's merged fix or None).  A stale fix newer than the
        newest clone stays in the buffer for the next frame; what no path takes
        goes to ``aid_dropped_log``."""
        cfg, buf = self.aiding, self._aid_buffer
        keep, cur, late = [], [], []
        for fix in buf:
            if fix.timestamp > t_frame or (fix.received is not None and fix.received > t_frame):
                keep.append(fix)
                continue
            z, var, mask = cfg.rows_of(fix)
            rt = cfg.route(fix.timestamp, mask, t_frame, self.cam_times)
            if rt[0] == "current":
                cur.append(fix)
            elif rt[0] == "wait":
                keep.append(fix)
            elif rt[0] == "drop":
                self.aid_dropped_log.append((self._n_published, fix.timestamp, rt[1]))
            else:
                _, slot, lam, rows, other = rt
                if other:
                    self.aid_dropped_log.append((self._n_published, fix.timestamp,
                                                 "velocity rows 0x%03x of a delayed fix" % other))
                late.append((_lib.aid_delayed_fix(np.r_[z[0:3], z[9:12]], np.r_[var[0:3], var[9:12]], slot, lam, rows),
                             slot, lam))
        self._aid_buffer = keep
        merged = cfg.merge(cur, t_frame) if cur else None
        return late, (_lib.aid_fix(*merged) if merged is not None else None)

    def _log_delayed(self, slot, lam, rec):
        app, gam, rows, status, self._aid_delayed_count = rec
        self.aid_delayed_log.append((self._n_published, rows, app, gam, slot, lam, status))

    def anchor_callback(self, fix):
        """Buffers an ``AnchorFix``; the frame whose timestamp lies within
        ``time_tol`` of the message's applies it.  A message no frame matches
        (an older one, or one from before gravity initialisation) is dropped
        and counted in ``anchor_dropped``."""
        if self.anchors is None:
            raise ValueError("anchor_callback needs MSCKF(anchors=AnchorConfig())")
        p, cov, z = self.anchors.in_world(fix)
        if len(p) > ANCHOR_MAX:
            raise ValueError("an AnchorFix holds at most %d anchors, not %d" % (ANCHOR_MAX, len(p)))
        rec = _lib.pack_anchors(p, cov, z)
        with self._lock:
            buf = self._anchor_buffer   # kept in time order; messages usually arrive so
            k = len(buf)
            while k > 0 and buf[k - 1][0] > fix.timestamp:
                k -= 1
            buf.insert(k, (float(fix.timestamp), rec))

    def _take_anchors(self, t_frame):
        """The frame's anchor records (None without a message); the messages
        up to the frame time leave the buffer."""
        buf, tol, msg = self._anchor_buffer, self.anchors.time_tol, None
        while buf and buf[0][0] <= t_frame + tol:
            t, rec = buf.pop(0)
            if t >= t_frame - tol and msg is None:
                msg = rec
            else:
                self.anchor_dropped += 1
        return msg

    def anchor_status(self):
        """(status uint8 [K], gamma [K]) of the anchors of the last message
        applied (_lib.ANCHOR_USED / GATED / DEPTH / NOT_PD); synchronises."""
        if self.anchors is None:
            raise ValueError("anchor_status needs MSCKF(anchors=AnchorConfig())")
        return self.ctx.anchor_status(self.slot)

    def _initialize_gravity_and_bias(self):
        """msckf.py:235-258"""
        sw = np.zeros(3)
        sa = np.zeros(3)
        for m in self.imu_msg_buffer:
            sw += m.angular_velocity
            sa += m.linear_acceleration
        bg = sw / len(self.imu_msg_buffer)
        g_imu = sa / len(self.imu_msg_buffer)
        g = np.array([0.0, 0.0, -np.linalg.norm(g_imu)])
        imu, _ = yield ("states",)
        imu = imu.copy()
        imu[_lib.I_BG:_lib.I_BG + 3] = bg
        imu[_lib.I_G:_lib.I_G + 3] = g
        imu[_lib.I_Q:_lib.I_Q + 4] = from_two_vectors(-g, g_imu)
        yield ("set_state", imu, None, self._initial_cov() if not self.cam_ids else None)

    def feature_callback(self, feature_msg):
        """msckf.py:180-233"""
        with self._lock:
            return self._drive(self._frame_steps(feature_msg))

    def _frame_steps(self, feature_msg):
        """The body of feature_callback as a request generator; returns the
        vio_result (or None before gravity initialisation)."""
        if isinstance(feature_msg, TrackMessage) and not self.device_map:
            raise TypeError("a TrackMessage names a message on the device, which only the device feature map reads: "
                            "it needs MSCKF(device_map=True)")
        if not self.is_gravity_set:
            if self.anchors is not None and self._take_anchors(feature_msg.timestamp) is not None:
                self.anchor_dropped += 1   # before gravity initialisation
            return None
        if self.is_first_img:
            self.is_first_img = False
            self.imu_timestamp = feature_msg.timestamp
        ws, accs = yield from self._batch_imu_processing(feature_msg.timestamp)
        zupt = self.zupt is not None and len(ws) > 0
        if zupt:   # the standstill update with the means of exactly the samples propagated (msckf_zupt.h)
            means = (np.mean(np.array(ws).reshape(-1, 3), axis=0), np.mean(np.array(accs).reshape(-1, 3), axis=0))
            if self._cue_prm is not None:
                yield ("zupt",) + means + (_cue_source(feature_msg),)
            else:
                yield ("zupt",) + means
        late = []
        if self.aiding is not None and self.aiding.delayed:   # late fixes on their clones first, oldest first
            late, fix = self._take_fixes(feature_msg.timestamp)
            for k, (f, slot, lam) in enumerate(late):   # one request each (msckf_aid_delayed.h)
                yield ("aid_delayed", f)
                if k + 1 < len(late):   # the next fix overwrites the slot's record: read it now (synchronises; rare)
                    self._log_delayed(slot, lam, (yield ("aid_delayed_results",)))
        else:
            fix = self._take_fix(feature_msg.timestamp) if self.aiding is not None else None
        if fix is not None:   # the frame's aiding fix (msckf_aid.h)
            yield ("aid", fix)
        anc = self._take_anchors(feature_msg.timestamp) if self.anchors is not None else None
        if anc is not None:   # the frame's anchor message (msckf_anchor.h)
            yield ("anchor", anc)
        yield from self._state_augmentation(feature_msg.timestamp)
        if self.device_map:
            yield from self._map_add_and_remove_lost(feature_msg)
            yield from self._map_prune_cam_state_buffer()
        else:
            self._add_feature_observations(feature_msg)
            yield from self._remove_lost_features()
            yield from self._prune_cam_state_buffer()
        # publish and online_reset's position variances in one read
        thr = self.config.position_std_threshold
        if self.odometry:   # the same read, the pose / velocity covariance with it
            st = yield ("states", 12, 3 if thr > 0 else 0, self._T_imu_body._vio_R__)
        else:
            st = yield (("states", 12, 3) if thr > 0 else ("states",))
        self._settle()
        if zupt:   # the device has drained: the update's record
            rec = yield ("zupt_results",)
            self._zupt_count = rec[2]
            self.zupt_log.append((self._n_published, rec[0], rec[1]) + tuple(rec[3:]))
        if late:   # the last late fix's record (the earlier ones were read behind their calls)
            self._log_delayed(late[-1][1], late[-1][2], (yield ("aid_delayed_results",)))
        if fix is not None:
            app, gam, rows, self._aid_count = yield ("aid_results",)
            self.aid_log.append((self._n_published, rows, app, gam))
        if anc is not None:
            app, used, _, self._anchor_count = yield ("anchor_results",)
            self.anchor_log.append((self._n_published, len(anc), used, app))
        res = self._publish_from(feature_msg.timestamp, _lib.unpack_imu(st[0]))
        if self.odometry:
            res = VioOdometry(*res, st[3], st[4])
        self._n_published += 1
        yield from self._online_reset(st[2] if thr > 0 else None)
        return res

    # ---------------------------------------------------------- propagation --
    def _batch_imu_processing(self, time_bound):
        """msckf.py:262-287: host walks the buffer, the device applies the samples.
        Returns the angular rates and specific forces handed to the device."""
        used = 0
        dts, ws, accs = [], [], []
        t_state = self.imu_timestamp
        for m in self.imu_msg_buffer:
            t = m.vio_timestamp__
            if t < t_state:
                used += 1
                continue
            if t > time_bound:
                break
            dts.append(t - t_state)
            ws.append(m.angular_velocity)
            accs.append(m.linear_acceleration)
            used += 1
            t_state = t
        if dts:
            yield ("propagate", np.array(dts), np.array(ws).reshape(-1, 3), np.array(accs).reshape(-1, 3))
        self.imu_timestamp = t_state
        self.imu_id = self._next_id
        self._next_id += 1
        self.imu_msg_buffer = self.imu_msg_buffer[used:]
        return ws, accs

    def _state_augmentation(self, time):
        """msckf.py:385-407"""
        yield ("augment",)
        self.cam_ids.append(self.imu_id)
        self.cam_times.append(time)

    def _drop_cams(self, ids):
        """The pruned cam states leave ``cam_ids`` and ``cam_times`` together."""
        for c in ids:
            k = self.cam_ids.index(c)
            del self.cam_ids[k], self.cam_times[k]

    def _add_feature_observations(self, feature_msg):
        """msckf.py:409-427"""
        sid = self.imu_id
        ms = self.map_server
        get = ms.get
        cur = len(ms)
        tracked = 0
        if isinstance(feature_msg, FeatureArrays):   # an array message, walked row by row
            for fid, z in zip(feature_msg.ids.tolist(), np.asarray(feature_msg.uv, float).tolist()):
                feat = get(fid)
                if feat is None:
                    feat = Feature(fid)
                    ms[fid] = feat
                else:
                    tracked += 1
                feat.observations[sid] = tuple(z)
            self.tracking_rate = tracked / (cur + 1e-5)
            return
        for f in feature_msg.vio_features:
            z = (float(f.u0), float(f.v0), float(f.u1), float(f.v1))   # packed into arrays once per request (_pack)
            feat = get(f.id)
            if feat is None:
                feat = Feature(f.id)
                ms[f.id] = feat
            else:
                tracked += 1
            feat.observations[sid] = z
        self.tracking_rate = tracked / (cur + 1e-5)

    # -------------------------------------------------------------- updates --
    def _pack(self, feats, cam_lists):
        slot = {cid: i for i, cid in enumerate(self.cam_ids)}
        off = [0]
        cams, zs = [], []
        for feat, cl in zip(feats, cam_lists):
            obs = feat.observations
            cams.extend([slot[cid] for cid in cl])
            zs.extend([obs[cid] for cid in cl])
            off.append(len(cams))
        return (np.array(off, np.int32), np.array(cams, np.int32),
                np.array(zs, float).reshape(-1, 4))

    def _triangulate(self, feats):
        """Feature.initialize_position (feature.py:167-295) for a batch of
        features, one wavefront each on the device."""
        if not feats:
            return
        off, cams, zs = self._pack(feats, [list(f.observations.keys()) for f in feats])
        p, ok = yield ("triangulate", off, cams, zs)
        for f, pi, oki in zip(feats, p, ok):
            f.position = pi
            f.is_initialized = bool(oki)

    def _update(self, feats, cam_lists, dofs, row_cap, to_init=()):
        """Stacked update over ``feats`` in order (device: jacobian, gating,
        stacking with the row cap, QR, Kalman), enqueued without a wait.
        Features in ``to_init`` are triangulated in the same device chain from
        the observations passed (their p_w rows go down as NaN); those whose
        triangulation fails take no part, exactly as if the host had dropped
        them (msckf.py:640-652).  The decision log and the new positions are
        applied at the next synchronisation point (``_settle``)."""
        if not feats:
            return
        off, cams, zs = self._pack(feats, cam_lists)
        chi2 = np.array([chi2_threshold(d) for d in dofs])
        init = set(id(f) for f in to_init)
        pw = np.array([np.full(3, np.nan) if id(f) in init else f.position for f in feats])
        pend = yield ("update", off, cams, zs, pw, chi2, row_cap)
        frame, D = self._n_published, 21 + 6 * len(self.cam_ids)

        def apply(acc, gam, p, valid, rows):
            # reproduce the reference's decision log: features after the row-cap
            # break are never gated (msckf.py:678-679); failed triangulations
            # never reach measurement_update
            for i, f in enumerate(feats):
                if id(f) in init:
                    f.is_initialized = bool(valid[i])
                    f.position = p[i]
            count = 0
            for i, f in enumerate(feats):
                if not valid[i]:
                    continue
                k = 4 * len(cam_lists[i]) - 3
                ok = bool(gam[i] < chi2[i])
                self.gate_log.append((frame, dofs[i], k, int(ok)))
                self.gamma_log.append((f.id, float(gam[i])))
                if ok:
                    count += k
                if row_cap and count > row_cap:
                    break
            # no processed feature (every triangulation failed): the reference
            # returns before measurement_update and logs no shape (msckf.py:652-654)
            if np.any(valid):
                self.shape_log.append((frame, rows, D))
        self._deferred.append((pend, apply))

    def _archive_deferred(self, ids, n_obs):
        """landmarks="host": when the results of the update just deferred -- a
        lost-path one over the features ``ids`` with ``n_obs`` observations each
        -- are applied, its accepted features go into the ring, as
        msckf_landmarks_archive appends them on the device."""
        if self._ring is None:
            return
        pend, fn = self._deferred[-1]
        ids, n_obs, frame = np.asarray(ids, np.int64), np.asarray(n_obs, np.int64), self._n_published

        def apply(acc, gam, p, valid, rows):
            fn(acc, gam, p, valid, rows)
            a = np.flatnonzero(acc)
            self._ring.append(ids[a], p[a], n_obs[a], gam[a], frame)
        self._deferred[-1] = (pend, apply)

    def _remove_lost_features(self):
        """msckf.py:616-689"""
        sid = self.imu_id
        invalid, candidates = [], []
        for feat in self.map_server.values():
            if sid in feat.observations:
                continue
            if len(feat.observations) < 3:
                invalid.append(feat.id)
                continue
            candidates.append(feat)
        # check_motion (always True with the EuRoC config's threshold -1,
        # config.py:10) needs the cam poses; the triangulations are independent
        # of each other, so they are batched into one launch.
        # The triangulations of the new features ride in the update's device
        # chain (their observations are the update's own): no wait here.
        thr = self.config.optimization.translation_threshold
        lost = candidates
        to_init = [f for f in candidates if not f.is_initialized]
        if thr >= 0 and to_init:
            _, cams_arr = yield ("states",)
            self._settle()
            cams = self._cam_dict(cams_arr)
            moved = set(id(f) for f in to_init if check_motion(f.observations, cams, thr))
            to_init = [f for f in to_init if id(f) in moved]
            candidates = [f for f in candidates if f.is_initialized or id(f) in moved]
        for fid in invalid:
            del self.map_server[fid]
        for feat in lost:   # gone from the map whether or not it initialises
            del self.map_server[feat.id]
        if not candidates:
            return
        cam_lists = [list(f.observations.keys()) for f in candidates]
        dofs = [len(cl) - 1 for cl in cam_lists]
        yield from self._update(candidates, cam_lists, dofs, self.ROW_CAP, to_init)
        self._archive_deferred([f.id for f in candidates], [len(cl) for cl in cam_lists])

    def _find_redundant_cam_states(self, cams_arr):
        """msckf.py:691-727 (host; needs the cam poses)."""
        cams = list(self._cam_dict(cams_arr).items())
        key = len(cams) - 4
        ci = key + 1
        first = 0
        kp = cams[key][1]["p"]
        kR = to_rotation(cams[key][1]["q"])
        rm = []
        for _ in range(2):
            pos = cams[ci][1]["p"]
            Rc = to_rotation(cams[ci][1]["q"])
            dist = np.linalg.norm(pos - kp)
            ang = 2 * np.arccos(to_quaternion(Rc @ kR.T)[-1])
            if ang < 0.2618 and dist < 0.4 and self.tracking_rate > 0.5:
                rm.append(cams[ci][0])
                ci += 1
            else:
                rm.append(cams[first][0])
                first += 1
                ci += 1
        return sorted(rm)

    def _prune_cam_state_buffer(self):
        """msckf.py:730-818"""
        if len(self.cam_ids) < self.config.max_cam_state_size:
            return
        _, cams_arr = yield ("states",)
        self._settle()
        rm = self._find_redundant_cam_states(cams_arr)
        thr = self.config.optimization.translation_threshold
        cams = self._cam_dict(cams_arr)
        to_init, involved = [], []   # (feature, its observations of removed cams), map order
        for feat in self.map_server.values():
            obs = feat.observations
            inv = [c for c in rm if c in obs]
            if not inv:
                continue
            if len(inv) == 1:
                del obs[inv[0]]
                continue
            involved.append((feat, inv))
            if not feat.is_initialized:
                to_init.append(feat)
        # features that fail check_motion stay uninitialized: their involved
        # observations are dropped below like those of a failed triangulation
        yield from self._triangulate([f for f in to_init if check_motion(f.observations, cams, thr)])
        feats, cam_lists = [], []
        for feat, inv in involved:
            if feat.is_initialized:
                feats.append(feat)
                cam_lists.append(inv)
            else:
                for c in inv:
                    del feat.observations[c]
        if feats:
            yield from self._update(feats, cam_lists, [len(cl) for cl in cam_lists], 0)
        else:   # the reference still calls measurement_update with an empty H
            self.shape_log.append((self._n_published, 0, 21 + 6 * len(self.cam_ids)))
        for feat, cl in zip(feats, cam_lists):
            for c in cl:
                del feat.observations[c]
        slots = [self.cam_ids.index(c) for c in rm]
        yield ("prune", np.array(slots, np.int32))
        self._drop_cams(rm)

    # ------------------------------------------------- the map on the device --
    def _log_update(self, pend, ids, counts, dofs, row_cap):
        """Defers the decision log of an update loaded from the device map:
        what ``_update.apply`` does, from the descriptors (arrays, no loop per
        feature)."""
        dofs = np.asarray(dofs, np.int64)
        chi2 = _chi2_of(dofs)
        k = 4 * np.asarray(counts, np.int64) - 3
        ids = np.asarray(ids, np.int64)
        frame, D = self._n_published, 21 + 6 * len(self.cam_ids)

        def apply(acc, gam, p, valid, rows):
            v = np.flatnonzero(valid)     # a failed triangulation never reaches measurement_update
            ok = gam[v] < chi2[v]
            if row_cap:                   # features after the row-cap break are never gated
                over = np.flatnonzero(np.cumsum(np.where(ok, k[v], 0)) > row_cap)
                if len(over):
                    v, ok = v[:over[0] + 1], ok[:over[0] + 1]
            self.gate_log.extend(zip([frame] * len(v), dofs[v].tolist(), k[v].tolist(), ok.astype(int).tolist()))
            self.gamma_log.extend(zip(ids[v].tolist(), np.asarray(gam, float)[v].tolist()))
            if np.any(valid):
                self.shape_log.append((frame, rows, D))
        self._deferred.append((pend, apply))

    def _map_add_and_remove_lost(self, feature_msg):
        """msckf.py:409-427 and 616-689 on the device table."""
        if isinstance(feature_msg, TrackMessage):   # the message lies on the device (msckf_handoff.h)
            tracked, cur, cand_ids, info = yield ("map_add_lost_tracks", feature_msg.frontend, feature_msg.lane)
        else:
            ids, uv = message_arrays(feature_msg)
            tracked, cur, cand_ids, info = yield ("map_add_lost", ids, uv)
        self.tracking_rate = tracked / (cur + 1e-5)
        if not len(cand_ids):
            return
        M = info[:, 0]
        _chi2_of(M - 1)   # KeyError for a dof outside the table, as the host path
        pend = yield ("map_update", _lib.MAP_LOAD_LOST, info[:, 3], M, None, not bool(info[:, 2].all()),
                      self.ROW_CAP)
        self._log_update(pend, cand_ids, M, M - 1, self.ROW_CAP)
        self._archive_deferred(cand_ids, M)

    def _map_prune_cam_state_buffer(self):
        """msckf.py:730-818 on the device table."""
        if len(self.cam_ids) < self.config.max_cam_state_size:
            return
        if self.device_keyframes:   # the choice, the select and the deferred results in one call
            slots, inv_ids, info = yield ("map_keyframe_select", self.tracking_rate)
            self._settle()          # the device has drained
            slots = np.asarray(slots, np.int32)
            rm = [self.cam_ids[s] for s in slots]
        else:
            _, cams_arr = yield ("states",)
            self._settle()
            rm = self._find_redundant_cam_states(cams_arr)
            slots = np.array([self.cam_ids.index(c) for c in rm], np.int32)
            inv_ids, info = yield ("map_prune_select", slots)
        init = info[:, 2].astype(bool)
        tri = np.flatnonzero(~init)
        pw = np.full((len(inv_ids), 3), np.nan)
        ok = init.copy()
        if len(tri):
            p, v = yield ("map_triangulate", info[tri, 3], info[tri, 0])
            pw[tri] = p
            ok[tri] = v
        upd = np.flatnonzero(ok)
        if len(upd):
            k = info[upd, 1]
            _chi2_of(k)
            pw_u = pw[upd]
            pw_u[~np.isfinite(pw_u).all(axis=1)] = np.nan
            pend = yield ("map_update", _lib.MAP_LOAD_PRUNE_UPDATE, info[upd, 3], k, pw_u, False, 0)
            self._log_update(pend, inv_ids[upd], k, k, 0)
        else:   # the reference still calls measurement_update with an empty H
            self.shape_log.append((self._n_published, 0, 21 + 6 * len(self.cam_ids)))
        yield ("map_prune_commit", info[tri, 3], ok[tri], pw[tri])
        yield ("prune", slots)
        self._drop_cams(rm)

    # ------------------------------------------------------ output / reset --
    def publish(self, time):
        """msckf.py:888-908"""
        return self._publish_from(time, self.imu_state())

    def _publish_from(self, time, s):
        T_i_w = Isometry3d(to_rotation(s["q"]).T, s["p"])
        Tb = self._T_imu_body
        T_b_w = Tb * T_i_w * Tb.inverse()
        body_velocity = Tb._vio_R__ @ s["v"]
        R_w_c = s["R_imu_cam0"] @ T_i_w._vio_R__.T
        t_c_w = s["p"] + T_i_w._vio_R__ @ s["t_cam0_imu"]
        return VioResult(time, T_b_w, body_velocity, Isometry3d(R_w_c.T, t_c_w))

    # ------------------------------------------------------------ landmarks --
    def landmarks(self, first=0, live=False):
        """The archive from sequence number ``first`` on as ``Landmarks``
        (msckf_odometry.h; oldest first, at most the ring's capacity);
        ``live``: the map's initialised features appended (stamp -1, gamma
        NaN).  A deferred update is applied first."""
        if self.landmark_mode is None:
            raise ValueError("this filter keeps no landmarks (MSCKF(landmarks='host' | 'device'))")
        with self._lock:
            if self._ring is not None:
                self._settle()
                rows = self._ring.get(first)
            else:
                rows = self.ctx.landmarks_get(self.slot, first)
            if not live:
                return Landmarks(*rows)
            if self.device_map:
                ids, mask, _, p_w, init = self.ctx.map_get(self.slot)
                n_obs = np.array([bin(int(m[0])).count("1") + bin(int(m[1])).count("1") for m in mask], np.int32)
                return with_live(rows, ids[init], p_w[init], n_obs[init])
            fs = [f for f in self.map_server.values() if f.is_initialized]
            return with_live(rows, [f.id for f in fs], np.array([f.position for f in fs], float).reshape(-1, 3),
                             [len(f.observations) for f in fs])

    @property
    def zupt_count(self):
        """Zero-velocity updates applied to this filter's slot (the device's
        counter as of the last frame's read)."""
        return self._zupt_count

    @property
    def aid_count(self):
        """Aiding fixes applied to this filter's slot (the device's counter as
        of the last frame's read)."""
        return self._aid_count

    @property
    def aid_delayed_count(self):
        """Delayed aiding fixes applied to this filter's slot (the device's
        counter as of the last record read)."""
        return self._aid_delayed_count

    @property
    def anchor_count(self):
        """Anchor updates applied to this filter's slot (the device's counter
        as of the last frame's read)."""
        return self._anchor_count

    def clear_landmarks(self):
        """Empties the archive (an online reset does not: the world frame continues)."""
        if self.landmark_mode is None:
            raise ValueError("this filter keeps no landmarks (MSCKF(landmarks='host' | 'device'))")
        with self._lock:
            if self._ring is not None:
                self._settle()
                self._ring.clear()
            else:
                self.ctx.landmarks_clear([self.slot])

    def _online_reset(self, d):
        """msckf.py:859-886 (``d``: P's position-block diagonal, read with the
        publish state)"""
        thr = self.config.position_std_threshold
        if thr <= 0:
            return
        if np.max(np.sqrt(d)) < thr:
            return
        self.cam_ids.clear()
        self.cam_times.clear()
        if self.device_map:
            yield ("map_clear",)
        else:
            self.map_server.clear()
        self.reset_log.append(self._n_published - 1)   # the frame just published
        imu, _ = yield ("states",)
        yield ("set_state", imu, None, self._initial_cov())

    def close(self):
        if self._own_ctx:
            self.ctx.close()


_DEVICE_MAP_CLASSES = {}


def _device_map_class(cls):
    """The class a ``cls(device_map=True)`` instance becomes: ``cls`` itself --
    MSCKF or a user's subclass, whose overrides stay -- plus ``map_server`` as a
    read-only snapshot of the device table.  (A subclass rather than a
    ``__getattr__`` on MSCKF, which would slow every attribute read of the
    host-map instances too.)"""
    sub = _DEVICE_MAP_CLASSES.get(cls)
    if sub is None:
        sub = type(cls.__name__ + "DeviceMap", (cls,), {
            "map_server": property(lambda self: self._map_snapshot(),
                                   doc="read-only snapshot of the device table (msckf_map_get)"),
            "__module__": cls.__module__})
        _DEVICE_MAP_CLASSES[cls] = sub
    return sub
