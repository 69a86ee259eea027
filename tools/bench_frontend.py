"""GPU stereo front-end throughput: the drop-in ImageProcessor
(msckf_amd.frontend) over a synthetic rectified stereo stream at the EuRoC
resolution (752 x 480; textured plane, known per-frame motion and disparity).
Prints one JSON line: frames/s end to end (host bookkeeping + uploads +
kernels), features published per frame, the per-operator wall times of one
frame, and the two-point RANSAC call (Frontend.two_point_ransac, wall time
through the binding: packing, one launch, one synchronisation) at 2 sets x 100
points (one frame's two cameras) and 22 sets x 100 points (the scheduler's 11
lanes), next to the numpy reference tests/ransac_ref.py on the host.

--device-pipeline runs the same stream a second time with
FrontendConfig.device_pipeline on (stereo_match and the detection + sieve of
add_new_features as single device calls, include/msckf_pipeline.h), checks that
it publishes the same messages, and adds to the JSON line its frames/s next to
the default path's and the wall time of one ImageProcessor.stereo_match at 200
points as the one call and as the composed six.

--lanes S runs S streams (distinct textures and motions) instead and prints its
own JSON line: (a) S ImageProcessor(device_pipeline=True) one after another,
frame by frame, against (b) one MultiImageProcessor (include/msckf_lanes.h:
one device call per stage for all lanes); the messages must be identical lane
by lane.  Lane-frames/s of both as the means of two alternated runs, the
device calls per step of each, and a cProfile split of (b)'s host time (a
further, untimed run).

--lanes S --device-tracks adds (c): the MultiImageProcessor with
FrontendConfig.device_tracks (include/msckf_tracks.h: the tracks on the device,
one call per tracked frame of all lanes).  Its messages must be identical too;
(b) and (c) alternate, two runs each, and the JSON line gains (c)'s
lane-frames/s, its device calls per step and a cProfile split of its host time.

--equalize {none,hist,clahe} sets FrontendConfig.equalize (include/msckf_equalize.h:
the images equalised on the device at upload) for the single stream and for the
lanes; --contrast C is the texture's contrast (default 110; 6 gives grey values
120..136, in which the fixed FAST threshold finds nothing without equalisation).
The JSON line names both.  --lanes S [--device-tracks] --stream-only runs the
MultiImageProcessor once and nothing else: the process to put under a kernel trace.

    python tools/bench_frontend.py [--frames 60] [--device-pipeline] [--lanes S [--device-tracks]]
                                   [--equalize none] [--contrast 110]
"""
import argparse
import cProfile
import pstats
import json
import os
import sys
import time
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import msckf_pkg  # noqa: E402,F401
import msckf_amd.frontend as fe_mod  # noqa: E402
import frontend_synth as fs  # noqa: E402
import ransac_ref as rr  # noqa: E402

StereoMsg = namedtuple("stereo_msg", ["vio_timestamp__", "cam0_image", "cam1_image", "cam0_msg", "cam1_msg"])
ImgMsg = namedtuple("img_msg", ["vio_timestamp__", "image"])
ImuMsg = namedtuple("imu_msg", ["vio_timestamp__", "angular_velocity", "linear_acceleration"])


def ransac_leg(fe, n_sets, n=100, n_hyp=7, reps=50):
    """Median wall time (ms) of the device call and of the host reference."""
    sets = [rr.synth_correspondences(n, seed=i, model=i % 2)["set"] for i in range(n_sets)]
    draws = np.random.default_rng(0).integers(0, 1 << 32, size=(n_sets, n_hyp, 2), dtype=np.uint32)
    for _ in range(3):
        fe.two_point_ransac(sets, 3.0, n_hyp, draws)
    dev, host = [], []
    for _ in range(reps):
        t1 = time.perf_counter()
        fe.two_point_ransac(sets, 3.0, n_hyp, draws)
        dev.append((time.perf_counter() - t1) * 1e3)
    for _ in range(5):
        t1 = time.perf_counter()
        rr.ransac_sets(sets, 3.0, n_hyp, draws)
        host.append((time.perf_counter() - t1) * 1e3)
    return {"device_ms": round(float(np.median(dev)), 4), "numpy_reference_ms": round(float(np.median(host)), 3)}


def run_stream(cfg, frames):
    """(ImageProcessor, frames/s from frame 2 on, features per frame, messages)."""
    ip = fe_mod.ImageProcessor(cfg)
    nfeat, msgs = [], []
    t0 = None
    for k, (c0, c1) in enumerate(frames):
        t = 0.05 * k
        for j in range(10):
            ip.imu_callback(ImuMsg(t - 0.05 + 0.005 * j, np.zeros(3), np.array([0.0, 0.0, 9.81])))
        if k == 2:
            t0 = time.perf_counter()
        msg = ip.stareo_callback(StereoMsg(t, c0, c1, ImgMsg(t, c0), ImgMsg(t, c1)))
        nfeat.append(len(msg.vio_features))
        msgs.append(msg)
    el = time.perf_counter() - t0
    return ip, (len(frames) - 2) / el, nfeat, msgs


def stereo_leg(ip, c0, c1, pts, reps=30):
    """Median wall time (ms) of ImageProcessor.stereo_match on the pair (c0, c1)."""
    ip.cam0_curr_img_msg, ip.cam1_curr_img_msg = ImgMsg(0.0, c0), ImgMsg(0.0, c1)
    ip.create_image_pyramids()
    for _ in range(3):
        ip.stereo_match(pts)
    ms = []
    for _ in range(reps):
        t1 = time.perf_counter()
        ip.stereo_match(pts)
        ms.append((time.perf_counter() - t1) * 1e3)
    return round(float(np.median(ms)), 3)


def lane_streams(S, n, W, H, contrast=110.0):
    """S streams of n rendered stereo pairs: texture seed, motion and disparity
    differ per lane.  As in the single stream the motion starts over every 40
    frames, so 40 pairs per lane are rendered."""
    streams = []
    for i in range(S):
        f = fs.texture_fn(4 + i, W=W, H=H, contrast=contrast)
        vx, vy, disp = 1.5 - 0.25 * (i % 5), -0.5 + 0.2 * (i % 4), 12.0 - 0.5 * (i % 3)
        pairs = [(fs.render(f, W, H, vx * k, vy * k), fs.render(f, W, H, vx * k - disp, vy * k))
                 for k in range(min(n, 40))]
        streams.append([pairs[k % 40] for k in range(n)])
    return streams


def lane_messages(k, streams):
    t = 0.05 * k
    imu = [ImuMsg(t - 0.05 + 0.005 * j, np.zeros(3), np.array([0.0, 0.0, 9.81])) for j in range(10)]
    return imu, [StereoMsg(t, c0, c1, ImgMsg(t, c0), ImgMsg(t, c1)) for c0, c1 in (st[k] for st in streams)]


def run_singles(cfg, streams):
    """(a): (lane-frames/s from step 2 on, messages per lane, device calls per step)."""
    S, n = len(streams), len(streams[0])
    ips = [fe_mod.ImageProcessor(fe_mod.FrontendConfig(**vars(cfg))) for _ in range(S)]
    calls = [0]
    for ip in ips:
        def serve(req, inner=ip._serve):
            calls[0] += (len(req[1]) if req[0] == "upload" else
                         sum(1 for a in req[1] if len(a[0])) if req[0] == "undistort" else 1)
            return inner(req)
        ip._serve = serve
    msgs = [[] for _ in range(S)]
    for k in range(n):
        imu, stereo = lane_messages(k, streams)
        if k == 2:
            t0, c0 = time.perf_counter(), calls[0]
        for i, ip in enumerate(ips):
            for m in imu:
                ip.imu_callback(m)
            msgs[i].append(ip.stareo_callback(stereo[i]))
    el = time.perf_counter() - t0
    for ip in ips:
        ip.fe.close()
    return S * (n - 2) / el, msgs, (calls[0] - c0) / (n - 2)


def run_multi(cfg, streams, profile=None):
    """(b): the same through one MultiImageProcessor."""
    S, n = len(streams), len(streams[0])
    mp = fe_mod.MultiImageProcessor(S, config=cfg)
    msgs = [[] for _ in range(S)]
    for k in range(n):
        imu, stereo = lane_messages(k, streams)
        if k == 2:
            t0, c0 = time.perf_counter(), sum(mp.launches.values())
            if profile:
                profile.enable()
        for i in range(S):
            for m in imu:
                mp.imu_callback(i, m)
        out = mp.stereo_callbacks(dict(enumerate(stereo)))
        for i in range(S):
            msgs[i].append(out[i])
    if profile:
        profile.disable()
    el = time.perf_counter() - t0
    calls = (sum(mp.launches.values()) - c0) / (n - 2)
    mp.close()
    return S * (n - 2) / el, msgs, calls


def profile_split(prof):
    """Cumulative seconds of (b)'s steps by where they go: each set call of
    Frontend (packing, the device call, unpacking), the lanes' generators
    between requests (per-feature Python) and the rest of stereo_callbacks."""
    st = pstats.Stats(prof).stats
    cum = lambda name: sum(v[3] for (f, _, fn), v in st.items() if fn == name and f.endswith("frontend.py"))
    total = cum("stereo_callbacks")
    dev = {k: round(cum(k), 4) for k in ("upload_many", "lk_sets", "stereo_match_sets", "two_point_ransac",
                                         "fast_grid_sets", "undistort_sets")}
    adv = cum("_advance")
    return {"stereo_callbacks_s": round(total, 4), "set_calls_s": dev, "set_calls_total_s": round(sum(dev.values()), 4),
            "lane_generators_s": round(adv, 4), "scheduling_rest_s": round(total - adv - sum(dev.values()), 4)}


def profile_split_tracks(prof):
    """Cumulative seconds of (c)'s steps: the two device calls of a tracked
    frame through the binding, the host work per lane before the call
    (_tracks_lane: IMU integration, draws, homography) and the rest (building
    the messages)."""
    st = pstats.Stats(prof).stats
    cum = lambda name: sum(v[3] for (f, _, fn), v in st.items() if fn == name and f.endswith("frontend.py"))
    total = cum("stereo_callbacks")
    dev = {k: round(cum(k), 4) for k in ("upload_many", "tracks_step")}
    args = cum("_tracks_lane")
    return {"stereo_callbacks_s": round(total, 4), "device_calls_s": dev, "device_calls_total_s": round(sum(dev.values()), 4),
            "lane_arguments_s": round(args, 4), "messages_rest_s": round(total - args - sum(dev.values()), 4)}


def tracks_leg(cfg, streams, msgs_a, fb):
    """(c) next to (b): b, c, b, c after lanes_main's first (b)."""
    cfg_t = fe_mod.FrontendConfig(**{**vars(cfg), "device_tracks": True})
    fc, msgs_c, calls_c = run_multi(cfg_t, streams)
    for i, (ma, mc) in enumerate(zip(msgs_a, msgs_c)):
        if ma != mc:
            raise SystemExit("lane %d: MultiImageProcessor with device_tracks published different messages" % i)
    runs_b, runs_c = [fb, run_multi(cfg, streams)[0]], [fc, run_multi(cfg_t, streams)[0]]
    prof = cProfile.Profile()
    run_multi(cfg_t, streams, profile=prof)
    return {"lane_frames_per_s": {"multi_image_processor": [round(v, 1) for v in runs_b],
                                  "device_tracks": [round(v, 1) for v in runs_c]},
            "device_calls_per_step": round(calls_c, 2), "messages_identical": True,
            "host_profile": profile_split_tracks(prof)}


def lanes_main(a, cfg, W, H):
    cfg = fe_mod.FrontendConfig(**{**vars(cfg), "device_pipeline": True})
    streams = lane_streams(a.lanes, a.frames, W, H, a.contrast)   # rendered up front: not part of the timing
    if a.stream_only:
        rate, msgs, calls = run_multi(fe_mod.FrontendConfig(**{**vars(cfg), "device_tracks": a.device_tracks}), streams)
        print(json.dumps({"component": "stereo front-end (image.py) on GPU, lanes, one stream", "lanes": a.lanes,
                          "frames_per_lane": a.frames, "equalize": a.equalize, "contrast": a.contrast,
                          "device_tracks": a.device_tracks, "lane_frames_per_s": round(rate, 1),
                          "device_calls_per_step": round(calls, 2),
                          "features_per_frame": float(np.mean([len(m.vio_features) for lane in msgs for m in lane]))}))
        return
    fa, msgs_a, calls_a = run_singles(cfg, streams)
    fb, msgs_b, calls_b = run_multi(cfg, streams)
    for i, (ma, mb) in enumerate(zip(msgs_a, msgs_b)):
        if ma != mb:
            raise SystemExit("lane %d: MultiImageProcessor published different messages" % i)
    tracks = {"device_tracks": tracks_leg(cfg, streams, msgs_a, fb)} if a.device_tracks else {}
    fa = 0.5 * (fa + run_singles(cfg, streams)[0])        # a, b, a, b: the means of two runs each
    fb = 0.5 * (fb + run_multi(cfg, streams)[0])
    prof = cProfile.Profile()
    run_multi(cfg, streams, profile=prof)
    nfeat = float(np.mean([len(m.vio_features) for lane in msgs_b for m in lane]))
    print(json.dumps({"component": "stereo front-end (image.py) on GPU, lanes", "resolution": [W, H],
                      "lanes": a.lanes, "frames_per_lane": a.frames, "equalize": a.equalize, "contrast": a.contrast,
                      "messages_identical": True,
                      "lane_frames_per_s": {"single_processors": round(fa, 1), "multi_image_processor": round(fb, 1)},
                      "device_calls_per_step": {"single_processors": round(calls_a, 2),
                                                "multi_image_processor": round(calls_b, 2)},
                      "features_per_frame": nfeat, "multi_host_profile": profile_split(prof), **tracks,
                      "note": "timed from step 2 on; the profile is a separate run under cProfile, which slows "
                              "the host: read it as shares, not as times"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--lanes", type=int, default=0,
                    help="run this many streams through single processors and through MultiImageProcessor")
    ap.add_argument("--device-pipeline", action="store_true",
                    help="also run the stream with FrontendConfig.device_pipeline on")
    ap.add_argument("--device-tracks", action="store_true",
                    help="with --lanes: also run the MultiImageProcessor with FrontendConfig.device_tracks")
    ap.add_argument("--equalize", choices=sorted(fe_mod.EQ_MODES), default="none",
                    help="FrontendConfig.equalize: equalise every image on the device at upload")
    ap.add_argument("--contrast", type=float, default=110.0, help="contrast of the synthetic texture")
    ap.add_argument("--stream-only", action="store_true",
                    help="with --lanes: one run of the MultiImageProcessor alone (what a kernel trace should see)")
    a = ap.parse_args()
    if (a.device_tracks or a.stream_only) and not a.lanes:
        ap.error("--device-tracks and --stream-only need --lanes")
    W, H = 752, 480
    f = fs.texture_fn(4, W=W, H=H, contrast=a.contrast)
    K = np.array([450.0, 450.0, 376.0, 240.0])
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    cfg = fe_mod.FrontendConfig(T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_distortion_coeffs=np.zeros(4),
                                cam1_distortion_coeffs=np.zeros(4), cam0_intrinsics=K, cam1_intrinsics=K, equalize=a.equalize)
    if a.lanes:
        return lanes_main(a, cfg, W, H)
    frames = []
    for k in range(a.frames):   # rendered up front: not part of the timing
        dx, dy = 1.5 * (k % 40), -0.5 * (k % 40)
        frames.append((fs.render(f, W, H, dx, dy), fs.render(f, W, H, dx - 12.0, dy)))
    ip, fps, nfeat, msgs = run_stream(cfg, frames)
    extra = {}
    if a.device_pipeline:
        cfg_on = fe_mod.FrontendConfig(**{**vars(cfg), "device_pipeline": True})
        ip_on, fps_on, nfeat_on, msgs_on = run_stream(cfg_on, frames)
        if msgs_on != msgs:
            raise SystemExit("the device pipeline published different messages")
        fps = 0.5 * (fps + run_stream(cfg, frames)[1])          # off, on, off, on: the means of two runs each
        fps_on = 0.5 * (fps_on + run_stream(cfg_on, frames)[1])
        pts = ip.fe.fast(ip._slot_c0, 15)[0][:200].astype(float)
        extra = {"frames_per_s_device_pipeline": round(fps_on, 1), "messages_identical": True,
                 "stereo_match_200pts_ms": {"one_call": stereo_leg(ip_on, *frames[0], pts),
                                            "composed_six_calls": stereo_leg(ip, *frames[0], pts)}}
        ip_on.fe.close()
    fe = ip.fe
    c0 = frames[0][0]
    ops = {}
    t1 = time.perf_counter(); fe.upload(0, c0); ops["upload_pyramid_ms"] = (time.perf_counter() - t1) * 1e3
    t1 = time.perf_counter(); xy, _ = fe.fast(0, 15); ops["fast_ms"] = (time.perf_counter() - t1) * 1e3
    pts = xy[:200]
    fe.upload(1, frames[1][0])
    t1 = time.perf_counter(); fe.lk(0, 1, pts, pts); ops["lk_200pts_ms"] = (time.perf_counter() - t1) * 1e3
    ransac = {"%dx100" % s: ransac_leg(fe, s) for s in (2, 22)}
    print(json.dumps({"component": "stereo front-end (image.py) on GPU", "resolution": [W, H],
                      "equalize": a.equalize, "contrast": a.contrast,
                      "frames_per_s": round(fps, 1), **extra, "features_per_frame": float(np.mean(nfeat)),
                      "fast_keypoints_frame0": int(len(xy)), "op_wall_ms": {k: round(v, 3) for k, v in ops.items()},
                      "two_point_ransac_n_hyp7": ransac,
                      "note": "host bookkeeping in Python; synthetic stream; cv2 absent (no reference timing)"}))


if __name__ == "__main__":
    main()
