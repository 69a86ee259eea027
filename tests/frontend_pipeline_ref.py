"""CPU restatement of include/msckf_pipeline.h (the header's text is the
specification) on the oracle's operators (oracle/frontend_oracle.py): the
reference of tests/test_pipeline_ref.py and tests/test_gpu_pipeline.py.

``stereo_match`` also reports each point's *margins*: how far every compared
quantity stayed from its threshold.  A decision can be demanded of another
implementation (fp32 / fp64 arithmetic in another order, LK positions equal to
1e-4 px only) just where the margins are well above those differences:
  err        | err - 3 |                                   px
  disparity  | |g.y - c1.y| - 20 |                         px
  bounds     distance of c1 from the nearest image edge    px
  epipolar   | error - thr | / thr                         relative
(inf where the quantity is NaN, which fails no test).

``OracleFrontend`` is the CPU stand-in of msckf_amd.frontend.Frontend with the
two calls of the header added, so that ImageProcessor(device_pipeline=True)
runs without a device.
"""
import numpy as np

import msckf_amd.frontend as fe_mod
from oracle import frontend_oracle as fo

MODEL_NAMES = {0: "radtan", 1: "equidistant"}
GRID_MAX_K, GRID_MAX_CELLS = 16, 1024


def stereo_match(img0, img1, cam0_pts, cam0, cam1, R_guess, E, stereo_threshold,
                 win=15, max_level=3, max_iter=30, eps=0.01):
    """Header steps 1-4.  cam0 / cam1: (intrinsics, model, coeffs).  Returns
    (cam1_pts float32 (n, 2), inlier uint8, reason uint8, margins dict of (n,)
    arrays)."""
    pts = np.asarray(cam0_pts, float).reshape(-1, 2)
    n = len(pts)
    K0, m0, k0 = np.asarray(cam0[0], float), MODEL_NAMES[int(cam0[1])], np.asarray(cam0[2], float)
    K1, m1, k1 = np.asarray(cam1[0], float), MODEL_NAMES[int(cam1[1])], np.asarray(cam1[2], float)
    E = np.asarray(E, float).reshape(3, 3)
    H, W = img1.shape
    if n == 0:
        z = np.zeros(0)
        return (np.zeros((0, 2), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.uint8),
                dict(err=z, disparity=z, bounds=z, epipolar=z))
    # 1. the initial guess (a rejected fisheye solution's (-1e6, -1e6) is distorted like any point)
    g = fo.distort_points(fo.undistort_points(pts, K0, m0, k0, R=np.asarray(R_guess, float).reshape(3, 3)),
                          K1, m1, k1)
    c0 = pts.astype(np.float32)
    lk = dict(win=win, max_level=max_level, max_iter=max_iter, eps=eps)
    c1, status = fo.lk_track(img0, img1, c0, g.astype(np.float32), **lk)   # 2.
    back, _ = fo.lk_track(img1, img0, c1, c0.copy(), **lk)                 # 3.
    d = c0 - back
    err = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])                   # float32
    disparity = np.abs(g[:, 1] - c1[:, 1].astype(float))
    outside = (c1[:, 0] < 0) | (c1[:, 0] > W - 1) | (c1[:, 1] < 0) | (c1[:, 1] > H - 1)
    u0 = fo.undistort_points(c0, K0, m0, k0)
    u1 = fo.undistort_points(c1, K1, m1, k1)
    lx = E[0, 0] * u0[:, 0] + E[0, 1] * u0[:, 1] + E[0, 2]
    ly = E[1, 0] * u0[:, 0] + E[1, 1] * u0[:, 1] + E[1, 2]
    with np.errstate(all="ignore"):
        error = np.abs(u1[:, 0] * lx) / np.sqrt(lx * lx + ly * ly)
    thr = stereo_threshold * (4.0 / (K0[0] + K0[1] + K1[0] + K1[1]))
    reason = np.zeros(n, np.uint8)
    for i in range(n):
        if not status[i]:
            reason[i] = 1
        elif not err[i] < 3:
            reason[i] = 2
        elif not disparity[i] < 20:
            reason[i] = 3
        elif outside[i]:
            reason[i] = 4
        elif error[i] > thr:
            reason[i] = 5
    fin = lambda a: np.where(np.isfinite(a), a, np.inf)
    c1d = c1.astype(float)
    with np.errstate(all="ignore"):
        epi = np.abs(error - thr) / thr
    margins = dict(err=fin(np.abs(err.astype(float) - 3.0)), disparity=fin(np.abs(disparity - 20.0)),
                   bounds=fin(np.minimum.reduce([np.abs(c1d[:, 0]), np.abs(c1d[:, 0] - (W - 1)),
                                                 np.abs(c1d[:, 1]), np.abs(c1d[:, 1] - (H - 1))])),
                   epipolar=fin(epi))
    return c1, (reason == 0).astype(np.uint8), reason, margins


def clear_of_thresholds(margins, px=1e-3, rel=1e-6):
    """Points whose every margin is at least ``px`` pixels (``rel`` for the
    epipolar test)."""
    return ((margins["err"] >= px) & (margins["disparity"] >= px) & (margins["bounds"] >= px) &
            (margins["epipolar"] >= rel))


def occupancy_mask(W, H, occupied):
    """The header's mask: ones, each occupied point's 7 x 7 block cleared,
    clipped right and bottom; a point with x < 3 or y < 3 (or NaN) clears
    nothing."""
    mask = np.ones((H, W), np.uint8)
    for px, py in np.asarray(occupied, np.float32).reshape(-1, 2):
        if not (px >= 3 and py >= 3 and px < W + 3 and py < H + 3):
            continue
        x, y = int(px), int(py)
        mask[y - 3:y + 4, x - 3:x + 4] = 0
    return mask


def fast_grid(img, threshold, occupied, grid_row, grid_col, k, max_kp=1 << 16):
    """The header's mfe_fast_grid.  Returns (xy float32 (m, 2), response
    float32 (m,), cell_count int32 (cells,), n_total), or (None, None, None,
    n_total) where the device call returns its overflow error."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    assert W >= 16 and H >= 16 and 1 <= k <= GRID_MAX_K and 1 <= grid_row * grid_col <= GRID_MAX_CELLS
    xy, resp = fo.fast_detect(img, threshold, nonmax=True, mask=occupancy_mask(W, H, occupied))
    n_total = len(xy)
    if n_total > max_kp:
        return None, None, None, n_total
    gh, gw = -(-H // grid_row), -(-W // grid_col)
    cell = (xy[:, 1].astype(int) // gh) * grid_col + xy[:, 0].astype(int) // gw
    cells = grid_row * grid_col
    out = []
    for c in range(cells):
        idx = np.nonzero(cell == c)[0]                                  # raster order
        out.append(idx[np.argsort(-resp[idx], kind="stable")][:k])      # response descending, raster ties
    sel = np.concatenate(out) if out else np.zeros(0, int)
    return (xy[sel].astype(np.float32).reshape(-1, 2), resp[sel].astype(np.float32),
            np.bincount(cell, minlength=cells).astype(np.int32), n_total)


class OracleFrontend:
    """The mfe_* operators of msckf_amd.frontend.Frontend on the CPU oracle,
    the two calls of msckf_pipeline.h included; ``calls`` counts every
    operator call by name (uploads apart)."""

    def __init__(self, width, height, nslot=4, max_level=3, max_points=4096, device=0):
        self.W, self.H, self.slots, self.calls = int(width), int(height), {}, []

    def upload(self, slot, image):
        self.slots[slot] = np.ascontiguousarray(image, np.uint8)

    def fast(self, slot, threshold, mask=None, max_kp=1 << 16):
        self.calls.append("fast")
        xy, resp = fo.fast_detect(self.slots[slot], threshold, nonmax=True, mask=mask)
        return xy, resp.astype(np.float32)

    def lk(self, slot_prev, slot_next, prev_pts, next_pts, win=15, max_level=3, max_iter=30, eps=0.01):
        self.calls.append("lk")
        return fo.lk_track(self.slots[slot_prev], self.slots[slot_next], prev_pts, next_pts, win=win,
                           max_level=max_level, max_iter=max_iter, eps=eps)

    def undistort(self, pts, intrinsics, model, coeffs, R=None, new_intrinsics=None):
        self.calls.append("undistort")
        return fo.undistort_points(pts, intrinsics, MODEL_NAMES[int(model)], coeffs, np.eye(3) if R is None else R,
                                   (1, 1, 0, 0) if new_intrinsics is None else new_intrinsics)

    def distort(self, pts, intrinsics, model, coeffs):
        self.calls.append("distort")
        return fo.distort_points(pts, intrinsics, MODEL_NAMES[int(model)], coeffs)

    def stereo_match(self, slot_cam0, slot_cam1, cam0_pts, cam0, cam1, R_guess, E, stereo_threshold,
                     win=15, max_level=3, max_iter=30, eps=0.01):
        self.calls.append("stereo_match")
        c1, inl, rsn, _ = stereo_match(self.slots[slot_cam0], self.slots[slot_cam1], cam0_pts, cam0, cam1, R_guess,
                                       E, stereo_threshold, win=win, max_level=max_level, max_iter=max_iter, eps=eps)
        return c1, inl, rsn

    def fast_grid(self, slot, threshold, occupied, grid_row, grid_col, k, max_kp=1 << 16):
        self.calls.append("fast_grid")
        xy, resp, cnt, n_total = fast_grid(self.slots[slot], threshold, occupied, grid_row, grid_col, k, max_kp)
        if xy is None:
            raise fe_mod._lib.MsckfError("mfe: %d keypoints exceed the capacity of %d (rc=-3)" % (n_total, max_kp))
        return xy, resp, cnt, n_total

    def close(self):
        pass
