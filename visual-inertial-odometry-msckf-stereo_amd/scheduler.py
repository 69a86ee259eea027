"""Batched multi-sequence scheduler.

Many independent filters -- one per sequence -- share one device context
(one filter slot each, P of all of them resident in HBM side by side).  Each
filter keeps its own host bookkeeping (an ``MSCKF`` lane: feature map, cam ids,
IMU buffer), and its frame is the same request generator the single-filter
``feature_callback`` drives.  The scheduler advances all lanes that have a
frame in lock step and serves every kind of request for all waiting lanes
with ONE batched launch:

  propagate   -> msckf_propagate_batch   (IMU propagation fused across filters)
  zupt        -> msckf_zupt_batch        (zupt=ZuptConfig: the standstill update,
                 gated on the device; zupt_results -> msckf_zupt_results, behind
                 the frame's states read; with ZuptConfig(vision=VisionCue) the
                 request carries the frame's cue source and the call is
                 msckf_zupt_batch_cued, one per source -- a front-end context's
                 motion records read on the device, or host arrays -- and the
                 read is msckf_zupt_cue_results, msckf_standstill.h)
  aid         -> msckf_aid_batch         (aiding=AidingConfig: the lanes that have
                 a fix at this frame, each with its own; aid_results ->
                 msckf_aid_results, behind the frame's states read)
  aid_delayed -> msckf_aid_delayed_batch (AidingConfig(delayed=True): the lanes'
                 j-th late fix of the frame step, one call per j, before aid;
                 aid_delayed_results -> msckf_aid_delayed_results, behind the
                 frame's states read, and behind the call when a lane has
                 another late fix in the same frame)
  anchor      -> msckf_anchor_batch      (anchors=AnchorConfig: the lanes that
                 have an anchor message at this frame, each with its own;
                 anchor_results -> msckf_anchor_results, behind the frame's
                 states read)
  augment     -> msckf_augment_batch
  triangulate -> msckf_batch_load + msckf_batch_triangulate
  update      -> msckf_batch_load + msckf_batch_update (per row cap), results
                 read back at the lanes' next sync point (one read per batch)
  states      -> msckf_readback          (publish + online_reset's diagonal,
                 keyframe selection; the deferred update results ride along)
  prune       -> msckf_prune_batch
  cov_diag    -> msckf_get_cov_diag_batch (online reset)
  map_*       -> the msckf_map_* call of the name (device_map=True;
                 map_add_lost_tracks: the lanes' messages read on the device
                 where the front-end left them, msckf_handoff.h), and
                 map_keyframe_select -> msckf_keyframe_select
                 (device_keyframes=True: the keyframe selection and the prune
                 select in one call, the deferred update results riding along)

Lanes whose frames diverge (one triangulates, another is already at its
update) wait at the earliest pipeline stage first, so requests of the same
kind merge again.  Results are identical to running each filter alone: the
batched kernels compute every filter independently.
"""
from __future__ import annotations

from collections import defaultdict

import numpy as np

from . import _lib
from .config import FilterConfig
from .frontend import MultiImageProcessor  # noqa: F401  (the image-side counterpart, same interface)
from .landmarks import check_mode
from .msckf import MSCKF
from .vio import MultiStereoVIO, StereoVIO  # noqa: F401  (both ends in one class)
from .trajectory import Trajectory

# pipeline order: a lane waiting at an earlier stage is served first
_ORDER = {"set_state": 0, "propagate": 1, "zupt": 1.5, "zupt_results": 5.1, "aid": 1.7, "aid_results": 5.2,
          "anchor": 1.8, "anchor_results": 5.25, "aid_delayed": 1.6, "aid_delayed_results": 1.65,
          "augment": 2, "map_add_lost": 2.5, "map_add_lost_tracks": 2.5, "triangulate": 3,
          "map_triangulate": 3, "update": 4, "map_update": 4, "states": 5, "map_prune_select": 5.3,
          "map_keyframe_select": 5.3,
          "map_prune_commit": 5.6, "prune": 6, "cov_diag": 7, "map_clear": 8}


class MultiMSCKF:
    """``n`` filters (one per sequence) on one device context."""

    def __init__(self, n, config=None, dtype=np.float64, device=0, cam_capacity=None, lane_configs=None,
                 device_map=False, map_capacity=1024, device_keyframes=False, landmarks=None, landmark_capacity=4096,
                 odometry=False, zupt=None, aiding=None, anchors=None):
        """``anchors``: as ``MSCKF``'s, one ``AnchorConfig`` for all lanes;
        ``anchor_callback(i, fix)`` feeds lane i, and one msckf_anchor_batch per
        frame step lists only the lanes that have a message.
        ``aiding``: as ``MSCKF``'s, one ``AidingConfig`` for all lanes (they
        share the parameters); ``aiding_callback(i, fix)`` feeds lane i, and one
        msckf_aid_batch per frame step lists only the lanes that have a fix.
        ``zupt``: as ``MSCKF``'s, one ``ZuptConfig`` for all lanes (as the
        device config is): one msckf_zupt_batch for the lanes of a frame step.
        ``landmarks`` / ``landmark_capacity`` / ``odometry``: as ``MSCKF``'s,
        for every lane ("device": one archive call for the lanes of a lost
        update, msckf_odometry.h; ``landmarks(i)`` reads lane i's).
        ``device_map`` / ``map_capacity``: every lane keeps its feature map
        in the context's tables (msckf_map.h), as ``MSCKF(device_map=True)``;
        ``device_keyframes``: the lanes' prune frames choose their cam states
        on the device (msckf_keyframes.h), one call for all waiting lanes.
        ``lane_configs`` (optional, one per lane): per-sequence host-side
        settings (check_motion's translation threshold, online_reset's
        position std threshold, window size).  The device context is shared,
        so every lane must agree on what the device computes with (noise,
        extrinsics, LM parameters: the C-ABI msckf_config_t)."""
        if device_keyframes and not device_map:
            raise ValueError("device_keyframes=True needs device_map=True")
        check_mode(landmarks, device_map)
        config = config or FilterConfig()
        if not isinstance(config, FilterConfig):
            config = FilterConfig.from_reference(config)
        cfgs = [config] * n if lane_configs is None else [
            c if isinstance(c, FilterConfig) else FilterConfig.from_reference(c) for c in lane_configs]
        if len(cfgs) != n:
            raise ValueError("%d lane configs for %d lanes" % (len(cfgs), n))
        dev0 = bytes(_lib.make_config(cfgs[0]))
        for i, c in enumerate(cfgs):
            if bytes(_lib.make_config(c)) != dev0:
                raise ValueError("lane %d: device-side filter parameters differ from lane 0's" % i)
        cap = cam_capacity or max(c.max_cam_state_size for c in cfgs) + 2
        self.config = cfgs[0]
        self.ctx = _lib.Context(cfgs[0], n_filters=n, n_cam_capacity=cap, dtype=dtype, device=device)
        self.device_map = bool(device_map)
        if self.device_map:
            for i, c in enumerate(cfgs):   # before the tables are made: MSCKF's own rule, per lane
                if c.optimization.translation_threshold >= 0:
                    self.ctx.close()
                    raise ValueError("lane %d: device_map=True needs optimization.translation_threshold < 0" % i)
            self.ctx.map_create(map_capacity)
            if landmarks == "device":
                try:
                    self.ctx.landmarks_create(landmark_capacity)
                except BaseException:
                    self.ctx.close()
                    raise
        self.device_keyframes = bool(device_keyframes)
        self.landmark_mode = landmarks
        self.lanes = [MSCKF(cfgs[i], ctx=self.ctx, slot=i, device_map=self.device_map,
                            device_keyframes=self.device_keyframes, landmarks=landmarks,
                            landmark_capacity=landmark_capacity, odometry=odometry, zupt=zupt, aiding=aiding,
                            anchors=anchors)
                      for i in range(n)]
        self.launches = defaultdict(int)       # batched device calls per request kind

    def __len__(self):
        return len(self.lanes)

    def close(self):
        self.ctx.close()

    def landmarks(self, i, first=0, live=False):
        """Lane i's archive, as ``MSCKF.landmarks``."""
        return self.lanes[i].landmarks(first, live)

    def clear_landmarks(self, i=None):
        """Empties lane i's archive (None: every lane's)."""
        for ln in (self.lanes if i is None else [self.lanes[i]]):
            ln.clear_landmarks()

    # ------------------------------------------------------------ callbacks --
    def imu_callback(self, i, imu_msg):
        self.lanes[i].imu_callback(imu_msg)

    def aiding_callback(self, i, fix):
        self.lanes[i].aiding_callback(fix)

    def anchor_callback(self, i, fix):
        self.lanes[i].anchor_callback(fix)

    def feature_callbacks(self, msgs):
        """``msgs``: {lane index: feature_msg}.  Returns {lane index:
        vio_result | None}, as the lanes' own feature_callback would."""
        gens, pending, out = {}, {}, {}
        for i, m in msgs.items():
            g = self.lanes[i]._frame_steps(m)
            gens[i] = g
            self._advance(i, g, None, pending, out, first=True)
        while pending:
            kind = min((r[0] for r in pending.values()), key=lambda k: _ORDER[k])
            group = [i for i, r in pending.items() if r[0] == kind]
            if kind in ("update", "map_update"):   # the row cap is per call: lost path 1500, prune path none
                cap = min(pending[i][6] for i in group)
                group = [i for i in group if pending[i][6] == cap]
            elif kind in ("cov_diag", "states"):   # one diagonal range (and, with odometry, one R_body) per call
                key = _read_key(pending[group[0]])
                group = [i for i in group if _read_key(pending[i]) == key]
            elif kind == "map_add_lost_tracks":   # one front-end context per call
                group = [i for i in group if pending[i][1] is pending[group[0]][1]]
            elif kind == "zupt" and len(pending[group[0]]) > 3:   # one cue source per call: a front-end context or the host
                group = [i for i in group if pending[i][3][0] is pending[group[0]][3][0]]
            results = self._serve(kind, group, [pending[i] for i in group])
            for i, res in zip(group, results):
                del pending[i]
                self._advance(i, gens[i], res, pending, out)
        return out

    def _advance(self, i, gen, value, pending, out, first=False):
        try:
            req = next(gen) if first else gen.send(value)
            pending[i] = req
        except StopIteration as e:
            out[i] = e.value

    # --------------------------------------------------------- batched calls --
    def _serve(self, kind, group, reqs):
        ctx = self.ctx
        slots = [self.lanes[i].slot for i in group]
        self.launches[kind] += 1
        if kind == "propagate":
            off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reqs])]).astype(np.int32)
            ctx.propagate_batch(slots, off, np.concatenate([r[1] for r in reqs]),
                                np.concatenate([r[2] for r in reqs]), np.concatenate([r[3] for r in reqs]))
            return [None] * len(group)
        if kind == "augment":
            ctx.augment_batch(slots)
            return [None] * len(group)
        if kind == "zupt" and len(reqs[0]) > 3:   # with the vision cue (msckf_standstill.h): one msckf_zupt_batch_cued
            ln0 = self.lanes[group[0]]
            w, a = np.array([r[1] for r in reqs]), np.array([r[2] for r in reqs])
            fe = reqs[0][3][0]
            if fe is not None:   # the lanes' motion records read where the front-end left them
                ctx.zupt_batch_cued(slots, w, a, ln0._zupt_prm, ln0._cue_prm, fe=fe, lanes=[r[3][1] for r in reqs])
            else:
                ctx.zupt_batch_cued(slots, w, a, ln0._zupt_prm, ln0._cue_prm, cue_n=[r[3][1] for r in reqs],
                                    cue_d2=[r[3][2] for r in reqs])
            return [None] * len(group)
        if kind == "zupt":   # the lanes share the parameters (one ZuptConfig)
            ctx.zupt_batch(slots, np.array([r[1] for r in reqs]), np.array([r[2] for r in reqs]),
                           self.lanes[group[0]]._zupt_prm)
            return [None] * len(group)
        if kind == "zupt_results" and self.lanes[group[0]]._cue_prm is not None:   # the six records in one read
            app, gam, cnt, cue, cn, cd = ctx.zupt_cue_results(slots)
            return [(bool(app[w]), float(gam[w]), int(cnt[w]), int(cue[w]), int(cn[w]), float(cd[w]))
                    for w in range(len(group))]
        if kind == "zupt_results":
            app, gam, cnt = ctx.zupt_results(slots)
            return [(bool(app[w]), float(gam[w]), int(cnt[w])) for w in range(len(group))]
        if kind == "aid":   # the lanes share the parameters (one AidingConfig), each has its own fix
            ctx.aid_batch(slots, [r[1] for r in reqs], self.lanes[group[0]]._aid_prm)
            return [None] * len(group)
        if kind == "aid_results":
            app, gam, rows, cnt = ctx.aid_results(slots)
            return [(bool(app[w]), float(gam[w]), int(rows[w]), int(cnt[w])) for w in range(len(group))]
        if kind == "aid_delayed":   # the lanes' j-th late fix of the frame step, each on its own clone pair
            ctx.aid_delayed_batch(slots, [r[1] for r in reqs], self.lanes[group[0]]._aid_prm)
            return [None] * len(group)
        if kind == "aid_delayed_results":
            app, gam, rows, sta, cnt = ctx.aid_delayed_results(slots)
            return [(bool(app[w]), float(gam[w]), int(rows[w]), int(sta[w]), int(cnt[w])) for w in range(len(group))]
        if kind == "anchor":   # the lanes share the parameters (one AnchorConfig), each has its own anchors
            ctx.anchor_batch(slots, [r[1] for r in reqs], self.lanes[group[0]]._anchor_prm)
            return [None] * len(group)
        if kind == "anchor_results":
            app, used, rows, cnt = ctx.anchor_results(slots)
            return [(bool(app[w]), int(used[w]), int(rows[w]), int(cnt[w])) for w in range(len(group))]
        if kind == "triangulate":
            self._load(slots, reqs, with_pw=False)
            ctx.batch_triangulate()
            _, _, p, v, _ = ctx.batch_results()
            return self._split(slots, reqs, lambda a, b, _s: (p[a:b].copy(), v[a:b].copy()))
        if kind == "update":   # deferred: each lane reads its share at its next sync point
            self._load(slots, reqs, with_pw=True)
            tri = any(not np.isfinite(np.asarray(r[4], float)).all() for r in reqs)
            ctx.batch_update(row_cap=reqs[0][6], triangulate=tri)
            return ctx.pending([(s,) + self._ranges[s] for s in slots])
        if kind == "states" and len(reqs[0]) > 3:   # the same read through msckf_readback_odom
            imu, cams, cv, pc, vc = ctx.readback_odom(slots, reqs[0][3], cov=reqs[0][1:3])
            return [(imu[w], cams[w], None if cv is None else cv[w], pc[w], vc[w]) for w in range(len(group))]
        if kind == "states":   # one read for the group (with the deferred batch, if any)
            cov = reqs[0][1:3] if len(reqs[0]) > 1 else None
            imu, cams, cv = ctx.readback(slots, cov=cov)
            if cv is None:
                return [(imu[w], cams[w]) for w in range(len(group))]
            return [(imu[w], cams[w], cv[w]) for w in range(len(group))]
        if kind == "prune":
            off = np.concatenate([[0], np.cumsum([len(r[1]) for r in reqs])]).astype(np.int32)
            ctx.prune_batch(slots, off, np.concatenate([r[1] for r in reqs]))
            return [None] * len(group)
        if kind == "cov_diag":
            d = ctx.cov_diag_batch(slots, reqs[0][1], reqs[0][2])
            return [d[w] for w in range(len(group))]
        if kind == "set_state":
            for s, r in zip(slots, reqs):
                ctx.set_state(s, r[1], r[2], r[3])
            return [None] * len(group)
        cat = lambda xs, dt: np.concatenate([np.asarray(x, dt) for x in xs])  # noqa: E731
        offs = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)  # noqa: E731
        if kind == "map_add_lost":
            return ctx.map_add_lost(slots, offs([r[1] for r in reqs]), cat([r[1] for r in reqs], np.int64),
                                    np.concatenate([np.asarray(r[2], float).reshape(-1, 4) for r in reqs]))
        if kind == "map_add_lost_tracks":
            return ctx.map_add_lost_tracks(slots, reqs[0][1], [r[2] for r in reqs])
        if kind == "map_prune_select":
            return ctx.map_prune_select(slots, offs([r[1] for r in reqs]), cat([r[1] for r in reqs], np.int32))
        if kind == "map_keyframe_select":   # the deferred batch, if any, rides along as with "states"
            return ctx.keyframe_select(slots, [r[1] for r in reqs])
        if kind == "map_triangulate":
            self._ranges = ctx.map_load(_lib.MAP_LOAD_PRUNE_TRI, slots, offs([r[1] for r in reqs]),
                                        cat([r[1] for r in reqs], np.int32), cat([r[2] for r in reqs], np.int32))
            ctx.batch_triangulate()
            _, _, p, v, _ = ctx.batch_results()
            return self._split(slots, reqs, lambda a, b, _s: (p[a:b].copy(), v[a:b].copy()))
        if kind == "map_update":   # one form per call (the row cap decides it); deferred like "update"
            form = reqs[0][1]
            pw = None
            if form == _lib.MAP_LOAD_PRUNE_UPDATE:
                pw = np.concatenate([np.asarray(r[4], float).reshape(-1, 3) for r in reqs])
            self._ranges = ctx.map_load(form, slots, offs([r[2] for r in reqs]), cat([r[2] for r in reqs], np.int32),
                                        cat([r[3] for r in reqs], np.int32), pw)
            ctx.batch_update(row_cap=reqs[0][6], triangulate=any(r[5] for r in reqs))
            if self.landmark_mode == "device" and form == _lib.MAP_LOAD_LOST:   # directly behind the update
                ctx.landmarks_archive(slots, offs([r[2] for r in reqs]), cat([r[2] for r in reqs], np.int32),
                                      [self.lanes[i]._n_published for i in group])
            return ctx.pending([(s,) + self._ranges[s] for s in slots])
        if kind == "map_prune_commit":
            ctx.map_prune_commit(slots, offs([r[1] for r in reqs]), cat([r[1] for r in reqs], np.int32),
                                 cat([r[2] for r in reqs], np.uint8),
                                 np.concatenate([np.asarray(r[3], float).reshape(-1, 3) for r in reqs]))
            return [None] * len(group)
        if kind == "map_clear":
            ctx.map_clear(slots)
            return [None] * len(group)
        raise ValueError("unknown request %r" % (kind,))

    def _load(self, slots, reqs, with_pw):
        """Concatenates the lanes' feature lists into one batch over all
        filter slots (slots without a request get no features)."""
        B = self.ctx.B
        by_slot = dict(zip(slots, reqs))
        feat_off, obs_off, cams, zs, pws, chis = [0], [0], [], [], [], []
        self._ranges = {}
        for s in range(B):
            r = by_slot.get(s)
            if r is not None:
                off, oc, oz = r[1], r[2], r[3]
                nf = len(off) - 1
                self._ranges[s] = (feat_off[-1], feat_off[-1] + nf)
                obs_off.extend(list(obs_off[-1] + np.asarray(off[1:], np.int64)))
                cams.append(np.asarray(oc, np.int32))
                zs.append(np.asarray(oz, float).reshape(-1, 4))
                if with_pw:
                    pws.append(np.asarray(r[4], float).reshape(-1, 3))
                    chis.append(np.asarray(r[5], float))
                feat_off.append(feat_off[-1] + nf)
            else:
                feat_off.append(feat_off[-1])
        cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)  # noqa: E731
        self.ctx.batch_load(np.array(feat_off), np.array(obs_off), cat(cams, (0,)).astype(np.int32),
                            cat(zs, (0, 4)), cat(pws, (0, 3)) if with_pw else None,
                            cat(chis, (0,)) if with_pw else None)

    def _split(self, slots, reqs, take):
        out = []
        for s in slots:
            a, b = self._ranges[s]
            out.append(take(a, b, s))
        return out

    # -------------------------------------------------------------- streams --
    def run_streams(self, streams, on_frame=None, messages=None, arrays=False):
        """Replays ``streams`` (replay.FeatureStream, one per lane) in lock
        step -- frame k of every stream in one batched round, each lane fed
        its own IMU samples up to its frame stamp first (IMU first on ties,
        as replay.FeatureStream.events) -- and returns one Trajectory per lane.
        ``messages``: the streams' ``messages()`` built by the caller
        beforehand (the front-end's output; a timed run leaves them out).
        ``arrays``: feed the frames as array messages (FeatureStream.frame_arrays)."""
        if len(streams) > len(self.lanes):
            raise ValueError("%d streams for %d filter slots" % (len(streams), len(self.lanes)))
        if messages is not None and len(messages) != len(streams):
            raise ValueError("%d message sets for %d streams" % (len(messages), len(streams)))
        imu_pos = [0] * len(streams)
        results = [[] for _ in streams]
        n_rounds = max(s.n_frames for s in streams) if streams else 0
        for k in range(n_rounds):
            msgs = {}
            for i, st in enumerate(streams):
                if k >= st.n_frames:
                    continue
                t = st.frame_t[k]
                j = int(np.searchsorted(st.imu[:, 0], t, side="right"))
                if messages is None:
                    for r in st.imu[imu_pos[i]:j]:
                        self.imu_callback(i, _imu_msg(r))
                    msgs[i] = st.frame_arrays(k) if arrays else st.frame_msg(k)
                else:
                    for m in messages[i][0][imu_pos[i]:j]:
                        self.imu_callback(i, m)
                    msgs[i] = messages[i][1][k]
                imu_pos[i] = j
            out = self.feature_callbacks(msgs)
            for i, res in out.items():
                if res is not None:
                    results[i].append(res)
            if on_frame is not None:
                on_frame(k, out)
        for i, st in enumerate(streams):        # trailing IMU samples
            if messages is None:
                for r in st.imu[imu_pos[i]:]:
                    self.imu_callback(i, _imu_msg(r))
            else:
                for m in messages[i][0][imu_pos[i]:]:
                    self.imu_callback(i, m)
        return [Trajectory.from_results(r) for r in results]


def _read_key(req):
    """What the lanes of one ``states`` / ``cov_diag`` call must share."""
    return tuple(req[1:3]) + ((np.asarray(req[3], float).tobytes(),) if len(req) > 3 else ())


def _imu_msg(r):
    from .synth import ImuMsg
    return ImuMsg(r[0], r[1:4].copy(), r[4:7].copy())
