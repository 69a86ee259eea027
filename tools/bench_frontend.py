"""GPU stereo front-end throughput: the drop-in ImageProcessor
(msckf_amd.frontend) over a synthetic rectified stereo stream at the EuRoC
resolution (752 x 480; textured plane, known per-frame motion and disparity).
Prints one JSON line: frames/s end to end (host bookkeeping + uploads +
kernels), features published per frame, the per-operator wall times of one
frame, and the two-point RANSAC call (Frontend.two_point_ransac, wall time
through the binding: packing, one launch, one synchronisation) at 2 sets x 100
points (one frame's two cameras) and 22 sets x 100 points (the scheduler's 11
lanes), next to the numpy reference tests/ransac_ref.py on the host.

    python tools/bench_frontend.py [--frames 60]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    a = ap.parse_args()
    W, H = 752, 480
    f = fs.texture_fn(4, W=W, H=H)
    K = np.array([450.0, 450.0, 376.0, 240.0])
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    cfg = fe_mod.FrontendConfig(T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_distortion_coeffs=np.zeros(4),
                                cam1_distortion_coeffs=np.zeros(4), cam0_intrinsics=K, cam1_intrinsics=K)
    frames = []
    for k in range(a.frames):   # rendered up front: not part of the timing
        dx, dy = 1.5 * (k % 40), -0.5 * (k % 40)
        frames.append((fs.render(f, W, H, dx, dy), fs.render(f, W, H, dx - 12.0, dy)))
    ip = fe_mod.ImageProcessor(cfg)
    nfeat = []
    t0 = None
    for k, (c0, c1) in enumerate(frames):
        t = 0.05 * k
        for j in range(10):
            ip.imu_callback(ImuMsg(t - 0.05 + 0.005 * j, np.zeros(3), np.array([0.0, 0.0, 9.81])))
        if k == 2:
            t0 = time.perf_counter()
        msg = ip.stareo_callback(StereoMsg(t, c0, c1, ImgMsg(t, c0), ImgMsg(t, c1)))
        nfeat.append(len(msg.vio_features))
    el = time.perf_counter() - t0
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
                      "frames_per_s": round((a.frames - 2) / el, 1), "features_per_frame": float(np.mean(nfeat)),
                      "fast_keypoints_frame0": int(len(xy)), "op_wall_ms": {k: round(v, 3) for k, v in ops.items()},
                      "two_point_ransac_n_hyp7": ransac,
                      "note": "host bookkeeping in Python; synthetic stream; cv2 absent (no reference timing)"}))


if __name__ == "__main__":
    main()
