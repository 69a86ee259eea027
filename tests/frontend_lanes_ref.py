"""CPU stand-in of msckf_amd.frontend.Frontend with the set calls of
include/msckf_lanes.h: tests/frontend_pipeline_ref.py's OracleFrontend plus
``*_sets`` methods that loop its own single methods, so that
MultiImageProcessor runs without a device.  ``calls`` logs ONE entry per set
call (the single calls inside a loop are not logged); ``fast`` and
``two_point_ransac`` log under their own names.

Also the golden scenes of tests/frontend_ref_scenes.py as per-frame message
lists, for drivers that step several streams together."""
import numpy as np

import frontend_pipeline_ref as pr
import frontend_synth as fs
import ransac_ref as rr
from frontend_ref_scenes import StereoMsg, ImgMsg, ImuMsg


class LanesOracleFrontend(pr.OracleFrontend):
    def __init__(self, width, height, nslot=4, max_level=3, max_points=4096, device=0):
        super().__init__(width, height, nslot, max_level, max_points, device)
        self.nslot, self.max_points = nslot, max_points

    def _quiet(self, fn, *a, **kw):
        n = len(self.calls)
        try:
            return fn(*a, **kw)
        finally:
            del self.calls[n:]

    def upload_many(self, slots, images):
        self.calls.append("upload_many")
        if len(set(int(s) for s in slots)) != len(slots):
            raise pr.fe_mod._lib.MsckfError("mfe: a slot is named twice (rc=-1)")
        for s, im in zip(slots, images):
            self.upload(int(s), im)

    def lk_sets(self, sets, **lk):
        self.calls.append("lk_sets")
        return [self._quiet(self.lk, *s, **lk) for s in sets]

    def stereo_match_sets(self, sets, **lk):
        self.calls.append("stereo_match_sets")
        return [self._quiet(self.stereo_match, *s, **lk) for s in sets]

    def fast_grid_sets(self, sets, threshold, grid_row, grid_col, k, max_kp=1 << 16):
        self.calls.append("fast_grid_sets")
        return [self._quiet(self.fast_grid, s[0], threshold, s[1], grid_row, grid_col, k, max_kp) for s in sets]

    def undistort_sets(self, sets):
        self.calls.append("undistort_sets")
        return [self._quiet(self.undistort, *s) if len(s[0]) else np.zeros((0, 2)) for s in sets]

    def two_point_ransac(self, sets, inlier_error, n_hyp, draws):
        self.calls.append("two_point_ransac")
        return rr.as_ransac_fn(sets, inlier_error, n_hyp, draws)


def scene_frames(g, name):
    """[(imu messages, stereo message)] per frame, as frontend_ref_scenes.run_scene feeds them."""
    W, H = (int(v) for v in g["size"])
    f = fs.texture_fn(int(g[name + "_seed"]), W=W, H=H)
    return stream_frames(f, W, H, int(g[name + "_frames"]), g[name + "_step"], g[name + "_gyro"],
                         float(g[name + "_disparity"]))


def stream_frames(f, W, H, n, step, gyro, disparity):
    out = []
    for k in range(n):
        t = 0.05 * k
        imu = [ImuMsg(t - 0.05 + 0.005 * j, np.array(gyro, float), np.array([0.0, 0.0, 9.81])) for j in range(10)]
        dx, dy = np.array(step) * k
        im0, im1 = fs.render(f, W, H, dx, dy), fs.render(f, W, H, dx - disparity, dy)
        out.append((imu, StereoMsg(t, ImgMsg(t, im0), ImgMsg(t, im1))))
    return out


def unpack(msg):
    """(ids, uv (n, 4)) of a published message, as run_scene returns them."""
    ids = np.array([m.id for m in msg.vio_features], np.int64)
    uv = np.array([[m.u0, m.v0, m.u1, m.v1] for m in msg.vio_features], float).reshape(-1, 4)
    return ids, uv


def run_lanes(mp, streams, start=None, on_step=None):
    """Steps ``streams`` (one list of scene_frames per lane) through the
    MultiImageProcessor ``mp``, lane i from step start[i] on.  Returns one list
    of (ids, uv) per lane; ``on_step(step, lanes in it)`` runs after each step."""
    start = start or [0] * len(streams)
    got = [[] for _ in streams]
    for step in range(max(s + len(fr) for s, fr in zip(start, streams))):
        msgs = {}
        for i, (s, fr) in enumerate(zip(start, streams)):
            if 0 <= step - s < len(fr):
                imu, msg = fr[step - s]
                for m in imu:
                    mp.imu_callback(i, m)
                msgs[i] = msg
        out = mp.stereo_callbacks(msgs)
        assert sorted(out) == sorted(msgs)
        for i, m in out.items():
            got[i].append(unpack(m))
        if on_step:
            on_step(step, sorted(msgs))
    return got
