"""Images to poses in one class: the stereo front-end's lanes and the filters'
lanes of one device, joined.

``MultiStereoVIO(n)`` owns one ``frontend.MultiImageProcessor`` (the lanes'
tracks on the device, include/msckf_tracks.h) and one
``scheduler.MultiMSCKF(device_map=True)`` (the lanes' feature maps on the
device, include/msckf_map.h).  ``imu_callback(i, msg)`` feeds both ends;
``stereo_callbacks({lane: stereo_msg})`` runs the lanes' frames through the
front-end and hands every lane's message to its filter:

  handoff="device"  the message never leaves the device
                    (include/msckf_handoff.h): a tracked frame's
                    ``mfe_tracks_step_msg`` writes it into the lane's message
                    table, the filters' ``msckf_map_add_lost_tracks`` reads it
                    there -- one call for all lanes of the round; the host
                    passes ``msckf.TrackMessage``s, which name the place;
  handoff="host"    the front-end's ids / uv come back to the host and go down
                    again as ``msckf.FeatureArrays``.

Both give every lane the poses the two classes wired by hand give it, bit for
bit.  ``StereoVIO`` is the one-lane form with the reference's call shape
(``imu_callback(msg)``, ``stereo_callback(msg)``).

With ``zupt=ZuptConfig(vision=VisionCue(...))`` the front-end also leaves each
lane's track motion on the device and the filters' zero-velocity update reads
it there (include/msckf_standstill.h; under handoff="host" the two numbers
travel with the array message).  The update is asynchronous and reads the
record in place: the frame's ``feature_callbacks`` ends in synchronising calls
(add_lost, the states read), so it has drained before the next frame's step
rewrites the record.

What still synchronises per frame: the front-end's step returns synchronised
(the host needs each lane's n and next_id, and the message must be complete
before another context's stream reads it), and so does the filters' add_lost
(its descriptors decide the update's shape on the host).
"""
from __future__ import annotations

import numpy as np

from .frontend import FrontendConfig, MultiImageProcessor
from .trajectory import Trajectory

HANDOFFS = ("device", "host")


def _frontend_configs(n, config, lane_configs, vision=None):
    """The lanes' front-end configs with device_pipeline and device_tracks forced on --
    and, with a ``VisionCue``, the motion statistic at its quantile."""
    if lane_configs is None:
        if config is None:
            config = FrontendConfig()
        elif not isinstance(config, FrontendConfig):
            config = FrontendConfig.from_reference(config)
        lane_configs = [config] * n
    cfgs = [c if isinstance(c, FrontendConfig) else FrontendConfig.from_reference(c) for c in lane_configs]
    extra = {"device_pipeline": True, "device_tracks": True}
    if vision is not None:   # the cue of the zero-velocity update (msckf_standstill.h), for both handoffs
        extra.update(track_motion=True, track_motion_quantile=float(vision.quantile))
    return [FrontendConfig(**{**vars(c), **extra}) for c in cfgs]


class MultiStereoVIO:
    """``n`` stereo-inertial streams (lanes) on one device, images to poses."""

    def __init__(self, n, filter_config=None, frontend_config=None, lane_filter_configs=None,
                 lane_frontend_configs=None, dtype=np.float64, device=0, map_capacity=1024, device_keyframes=True,
                 handoff="device", landmarks=None, landmark_capacity=4096, odometry=False, zupt=None,
                 aiding=None, anchors=None):
        """``landmarks`` / ``landmark_capacity`` / ``odometry``: as
        ``MultiMSCKF``'s (msckf_odometry.h); ``zupt``: as ``MultiMSCKF``'s
        (msckf_zupt.h; ``zupt_log(i)`` reads lane i's decisions; with
        ``ZuptConfig(vision=VisionCue(...))`` the front-end's lanes leave their
        track motion on the device and the update is gated on it too,
        msckf_standstill.h, under either handoff); ``aiding``:
        as ``MultiMSCKF``'s (msckf_aid.h; ``aiding_callback(i, fix)``,
        ``aid_log(i)``); ``anchors``: as ``MultiMSCKF``'s (msckf_anchor.h;
        ``anchor_callback(i, fix)``, ``anchor_log(i)``).
        ``filter_config`` / ``lane_filter_configs``: as ``MultiMSCKF``'s
        ``config`` / ``lane_configs``; ``frontend_config`` /
        ``lane_frontend_configs``: as ``MultiImageProcessor``'s (device_pipeline
        and device_tracks are switched on in every lane).  The constructor's
        errors are the two classes' own; no context is left open behind one."""
        from .scheduler import MultiMSCKF   # scheduler exports this module's classes
        if handoff not in HANDOFFS:
            raise ValueError("handoff = %r, expected one of %r" % (handoff, HANDOFFS))
        self.handoff = handoff
        vision = getattr(zupt, "vision", None)
        self.frontend = MultiImageProcessor(n, lane_configs=_frontend_configs(n, frontend_config,
                                                                              lane_frontend_configs, vision),
                                            device=device)
        try:
            self.filters = MultiMSCKF(n, config=filter_config, dtype=dtype, device=device,
                                      lane_configs=lane_filter_configs, device_map=True, map_capacity=map_capacity,
                                      device_keyframes=device_keyframes, landmarks=landmarks,
                                      landmark_capacity=landmark_capacity, odometry=odometry, zupt=zupt,
                                      aiding=aiding, anchors=anchors)
        except BaseException:
            self.frontend.close()
            raise
        self._closed = False

    def __len__(self):
        return len(self.filters)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if not self._closed:
            self._closed = True
            self.frontend.close()
            self.filters.close()

    @property
    def launches(self):
        """Device calls per request kind: {"frontend": ..., "filter": ...}."""
        return {"frontend": dict(self.frontend.launches), "filter": dict(self.filters.launches)}

    def tracks(self, i):
        """Lane i's track table on the device, as ``MultiImageProcessor.tracks``."""
        return self.frontend.tracks(i)

    def landmarks(self, i, first=0, live=False):
        """Lane i's landmark archive, as ``MultiMSCKF.landmarks``."""
        return self.filters.landmarks(i, first, live)

    def clear_landmarks(self, i=None):
        self.filters.clear_landmarks(i)

    def zupt_log(self, i):
        """Lane i's zero-velocity decisions, (frame, applied, gamma) per update
        enqueued -- with a vision cue (frame, applied, gamma, cue, n, d2)."""
        return self.filters.lanes[i].zupt_log

    def aid_log(self, i):
        """Lane i's aiding decisions, (frame, rows, applied, gamma) per fix enqueued."""
        return self.filters.lanes[i].aid_log

    def aid_delayed_log(self, i):
        """Lane i's delayed aiding decisions (``AidingConfig(delayed=True)``),
        (frame, rows, applied, gamma, slot, lambda, status) per late fix enqueued."""
        return self.filters.lanes[i].aid_delayed_log

    def anchor_log(self, i):
        """Lane i's anchor decisions, (frame, n, used, applied) per message enqueued."""
        return self.filters.lanes[i].anchor_log

    # ------------------------------------------------------------ callbacks --
    def imu_callback(self, i, msg):
        self.frontend.imu_callback(i, msg)
        self.filters.imu_callback(i, msg)

    def aiding_callback(self, i, fix):
        self.filters.aiding_callback(i, fix)

    def anchor_callback(self, i, fix):
        self.filters.anchor_callback(i, fix)

    def stereo_callbacks(self, msgs):
        """``msgs``: {lane index: stereo_msg}.  Returns {lane index:
        vio_result | None}, as the lanes' own feature_callback would."""
        if self.handoff == "device":
            feats = self.frontend.stereo_callbacks(msgs, handoff=True)
        else:
            feats = self.frontend.stereo_callbacks(msgs, arrays=True)
        return self.filters.feature_callbacks(feats)

    # -------------------------------------------------------------- streams --
    def run(self, streams, start=None, on_step=None):
        """Replays ``streams`` -- per lane one list of (imu messages, stereo
        message), a frame's IMU messages first -- in lock step, lane i from
        step ``start[i]`` on, and returns one Trajectory per lane.
        ``on_step(step, {lane: vio_result | None})`` runs after each step."""
        if len(streams) > len(self):
            raise ValueError("%d streams for %d lanes" % (len(streams), len(self)))
        start = list(start) if start is not None else [0] * len(streams)
        if len(start) != len(streams):
            raise ValueError("%d start steps for %d streams" % (len(start), len(streams)))
        results = [[] for _ in streams]
        for step in range(max([s + len(fr) for s, fr in zip(start, streams)], default=0)):
            msgs = {}
            for i, (s, fr) in enumerate(zip(start, streams)):
                if 0 <= step - s < len(fr):
                    imu, msg = fr[step - s]
                    for m in imu:
                        self.imu_callback(i, m)
                    msgs[i] = msg
            out = self.stereo_callbacks(msgs) if msgs else {}
            for i, res in out.items():
                if res is not None:
                    results[i].append(res)
            if on_step is not None:
                on_step(step, out)
        return [Trajectory.from_results(r) for r in results]


class StereoVIO:
    """One stream, the reference's call shape: ``imu_callback(msg)`` and
    ``stereo_callback(stereo_msg) -> vio_result | None``."""

    def __init__(self, filter_config=None, frontend_config=None, dtype=np.float64, device=0, map_capacity=1024,
                 device_keyframes=True, handoff="device", landmarks=None, landmark_capacity=4096, odometry=False,
                 zupt=None, aiding=None, anchors=None):
        self.multi = MultiStereoVIO(1, filter_config=filter_config, frontend_config=frontend_config, dtype=dtype,
                                    device=device, map_capacity=map_capacity, device_keyframes=device_keyframes,
                                    handoff=handoff, landmarks=landmarks, landmark_capacity=landmark_capacity,
                                    odometry=odometry, zupt=zupt, aiding=aiding, anchors=anchors)
        self.handoff = self.multi.handoff

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.multi.close()

    @property
    def launches(self):
        return self.multi.launches

    @property
    def filter(self):
        """The stream's ``MSCKF`` lane."""
        return self.multi.filters.lanes[0]

    def tracks(self):
        return self.multi.tracks(0)

    def landmarks(self, first=0, live=False):
        return self.multi.landmarks(0, first, live)

    def clear_landmarks(self):
        self.multi.clear_landmarks(0)

    @property
    def zupt_log(self):
        return self.multi.zupt_log(0)

    @property
    def zupt_count(self):
        return self.filter.zupt_count

    @property
    def aid_log(self):
        return self.multi.aid_log(0)

    @property
    def aid_count(self):
        return self.filter.aid_count

    @property
    def aid_delayed_log(self):
        return self.multi.aid_delayed_log(0)

    @property
    def aid_delayed_count(self):
        return self.filter.aid_delayed_count

    @property
    def anchor_log(self):
        return self.multi.anchor_log(0)

    @property
    def anchor_count(self):
        return self.filter.anchor_count

    def anchor_status(self):
        return self.filter.anchor_status()

    def imu_callback(self, msg):
        self.multi.imu_callback(0, msg)

    def anchor_callback(self, fix):
        self.multi.anchor_callback(0, fix)

    def aiding_callback(self, fix):
        self.multi.aiding_callback(0, fix)

    def stereo_callback(self, stereo_msg):
        return self.multi.stereo_callbacks({0: stereo_msg})[0]

    stareo_callback = stereo_callback   # the reference's spelling (image.py), as in ImageProcessor
