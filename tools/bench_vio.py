"""Images to poses, lanes: the stereo front-end and the filters of one device
joined three ways, on the stream of tools/bench_frontend.py --lanes (752 x 480,
distinct textures and motions per lane, ten IMU samples per frame) and with its
warm-up (timed from step 2 on):

  (a) wired    MultiImageProcessor(device_tracks).stereo_callbacks(arrays=True)
               into MultiMSCKF(device_map, device_keyframes).feature_callbacks,
               joined by hand;
  (b) host     MultiStereoVIO(handoff="host"): the same calls inside the class;
  (c) device   MultiStereoVIO(handoff="device"): the message stays on the
               device (include/msckf_handoff.h).

One JSON line per run: lane-frames/s, the device calls per step by kind (both
ends) and the calls among them that end with a synchronisation.  (b) and (c)
must publish (a)'s poses bit for bit; the tool exits non-zero otherwise.

    python tools/bench_vio.py [--frames 60] [--lanes 1 11] [--repeat R] [--dtype f64|f32]
                              [--zupt [--zupt-cue veto|either]]

--zupt adds the zero-velocity update (msckf_zupt.h) to every composition;
--zupt-cue gates it on the front-end's track motion as well (msckf_standstill.h,
VisionCue's defaults in the given mode).

--repeat R runs (a), (b), (c), (a), (b), (c), ... R times over, alternating, on
the same rendered streams in one process, one JSON line per run (every run of
(b) and (c) is compared with the first (a)): the raw material of
profiles/vio_pipeline/."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import msckf_pkg  # noqa: E402,F401
import msckf_amd.frontend as fe_mod  # noqa: E402
from msckf_amd.scheduler import MultiMSCKF, MultiStereoVIO  # noqa: E402
from bench_frontend import lane_messages, lane_streams  # noqa: E402

# every front-end call returns synchronised; of the filters' request kinds these do
FILTER_SYNCS = ("map_add_lost", "map_add_lost_tracks", "states", "map_keyframe_select", "map_prune_select",
                "map_triangulate", "cov_diag")


class Wired:
    """(a): the two classes joined by hand, behind MultiStereoVIO's interface."""

    def __init__(self, n, frontend_config, dtype, opt):
        extra = {"device_pipeline": True, "device_tracks": True}
        vision = getattr(opt.get("zupt"), "vision", None)
        if vision is not None:   # as MultiStereoVIO switches it on
            extra.update(track_motion=True, track_motion_quantile=float(vision.quantile))
        cfg = fe_mod.FrontendConfig(**{**vars(frontend_config), **extra})
        self.frontend = fe_mod.MultiImageProcessor(n, config=cfg)
        self.filters = MultiMSCKF(n, dtype=dtype, device_map=True, device_keyframes=True, **opt)

    def imu_callback(self, i, m):
        self.frontend.imu_callback(i, m)
        self.filters.imu_callback(i, m)

    def stereo_callbacks(self, msgs):
        return self.filters.feature_callbacks(self.frontend.stereo_callbacks(msgs, arrays=True))

    @property
    def launches(self):
        return {"frontend": dict(self.frontend.launches), "filter": dict(self.filters.launches)}

    def close(self):
        self.frontend.close()
        self.filters.close()


def make(which, n, cfg, dtype, opt):
    """``opt``: the landmarks / odometry arguments (msckf_odometry.h), the same in every composition."""
    if which == "wired":
        return Wired(n, cfg, dtype, opt)
    return MultiStereoVIO(n, frontend_config=cfg, dtype=dtype, handoff=which, **opt)


def pose_bytes(res):
    if res is None:
        return None
    return b"".join(np.ascontiguousarray(x, np.float64).tobytes() for x in
                    (res.timestamp, res.pose._vio_R__, res.pose._vio_t__, res.velocity, res.cam0_pose._vio_R__,
                     res.cam0_pose._vio_t__))


def run(which, streams, cfg, dtype, opt):
    """(lane-frames/s from step 2 on, poses per lane as bytes, calls per step by kind)."""
    S, n = len(streams), len(streams[0])
    vio = make(which, S, cfg, dtype, opt)
    poses = [[] for _ in range(S)]
    try:
        for k in range(n):
            imu, stereo = lane_messages(k, streams)
            if k == 2:
                t0, l0 = time.perf_counter(), vio.launches
            for i in range(S):
                for m in imu:
                    vio.imu_callback(i, m)
            out = vio.stereo_callbacks(dict(enumerate(stereo)))
            for i in range(S):
                poses[i].append(pose_bytes(out[i]))
        el = time.perf_counter() - t0
        l1 = vio.launches
    finally:
        vio.close()
    per = {side: {k: round((v - l0[side].get(k, 0)) / (n - 2), 3) for k, v in l1[side].items()
                  if v != l0[side].get(k, 0)} for side in ("frontend", "filter")}
    syncs = sum(per["frontend"].values()) + sum(v for k, v in per["filter"].items() if k in FILTER_SYNCS)
    return S * (n - 2) / el, poses, per, round(syncs, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 11])
    ap.add_argument("--repeat", type=int, default=1, help="alternating runs of each composition")
    ap.add_argument("--dtype", choices=("f64", "f32"), default="f64")
    ap.add_argument("--landmarks", choices=("host", "device"), default=None,
                    help="keep the landmark archive (msckf_odometry.h) in every composition")
    ap.add_argument("--odometry", action="store_true", help="the frames' reads bring the pose covariance along")
    ap.add_argument("--zupt", action="store_true", help="the zero-velocity update (msckf_zupt.h) in every composition")
    ap.add_argument("--zupt-cue", choices=("veto", "either"), default=None,
                    help="with --zupt: the vision standstill cue (msckf_standstill.h) in this mode")
    a = ap.parse_args()
    if a.zupt_cue and not a.zupt:
        ap.error("--zupt-cue needs --zupt")
    opt = dict(landmarks=a.landmarks, odometry=a.odometry) if a.landmarks or a.odometry else {}
    tag = {}
    if a.zupt:
        from msckf_amd import VisionCue, ZuptConfig
        opt["zupt"] = ZuptConfig(vision=VisionCue(mode=a.zupt_cue) if a.zupt_cue else None)
        tag = {"zupt": True, "zupt_cue": a.zupt_cue}
    dtype = np.float64 if a.dtype == "f64" else np.float32
    W, H = 752, 480
    K = np.array([450.0, 450.0, 376.0, 240.0])
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    cfg = fe_mod.FrontendConfig(T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_distortion_coeffs=np.zeros(4),
                                cam1_distortion_coeffs=np.zeros(4), cam0_intrinsics=K, cam1_intrinsics=K)
    bad = False
    for S in a.lanes:
        streams = lane_streams(S, a.frames, W, H)         # rendered up front: not part of the timing
        ref = None
        for r, which in ((r, w) for r in range(a.repeat) for w in ("wired", "host", "device")):
            fps, poses, per, syncs = run(which, streams, cfg, dtype, opt)
            n_poses = sum(p is not None for lane in poses for p in lane)
            same = None
            if ref is None:
                ref = poses
            else:
                same = poses == ref
                bad |= not same
            print(json.dumps({"component": "images to poses, lanes", "composition": which, "run": r, "lanes": S,
                              "frames_per_lane": a.frames, "dtype": a.dtype, "resolution": [W, H],
                              "lane_frames_per_s": round(fps, 1), "device_calls_per_step": per,
                              "synchronisations_per_step": syncs, "poses": n_poses,
                              "poses_identical_to_first_wired": same,
                              **{k: v for k, v in opt.items() if k != "zupt"}, **tag,
                              "note": "timed from step 2 on; host bookkeeping in Python; synthetic stream"}),
                  flush=True)
            bad |= n_poses == 0
    if bad:
        raise SystemExit("a composition published no pose, or poses that differ from the hand-wired composition's")


if __name__ == "__main__":
    main()
