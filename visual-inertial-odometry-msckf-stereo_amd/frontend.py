"""GPU stereo front-end: drop-in host mirror of the
reference ``ImageProcessor`` (MSCKF/image.py:36-702).

The host keeps what the reference keeps in Python -- the grid bookkeeping,
feature ids and lifetimes, pruning, the stereo-match inlier logic and the
published message -- and every image operator runs in the HIP kernels of
``csrc/msckf_frontend.hip`` behind ``include/msckf_frontend.h``:

  reference (cv2)                              here
  FastFeatureDetector.detect (image.py:175,333) mfe_fast   (k_fast_sets, k_fast_rows_sets)
  calcOpticalFlowPyrLK (image.py:254,581,585)   mfe_lk     (k_lk_sets; pyramids + Scharr
                                                            built by mfe_upload)
  undistortPoints / fisheye (image.py:640-674)  mfe_undistort
  projectPoints / fisheye (image.py:676-702)    mfe_distort
  RANSAC stub (image.py:292-293)                mfe_two_point_ransac (k_two_point_ransac,
                                                include/msckf_ransac.h), opt-in
  stereo_match (image.py:554-638)               mfe_stereo_match (k_stereo_match_sets,
                                                include/msckf_pipeline.h), opt-in
  mask + detect + sieve (image.py:317-360)      mfe_fast_grid (include/msckf_pipeline.h), opt-in
  one stream per ImageProcessor                 MultiImageProcessor: S streams on one context,
                                                each stage one call over all lanes' sets
                                                (mfe_upload_many, mfe_lk_sets, mfe_stereo_match_sets,
                                                mfe_fast_grid_sets, mfe_undistort_sets,
                                                include/msckf_lanes.h)
  ids, lifetimes, grid lists (image.py:219-404)   with FrontendConfig.device_tracks the lanes' track
                                                tables live on the device and a tracked frame of
                                                all lanes is ONE call (mfe_tracks_step,
                                                include/msckf_tracks.h), opt-in
  (none: the image as it comes)                 FrontendConfig.equalize: equalizeHist / CLAHE on the
                                                device at upload (mfe_upload_many_eq,
                                                include/msckf_equalize.h), opt-in

cv2 is absent here and on the GPU box: the kernels restate the published
OpenCV 4.x algorithms (oracle/frontend_oracle.py), parity unpinned against cv2
itself.  Method names, arguments and the message layout follow the reference
(including its spelling ``stareo_callback``), so ``vio.py`` can construct this
class in place of its own.  The reference's stubs are kept as they are by
default: RANSAC marks every match an inlier (image.py:292-293) and
``rescale_points`` is unused.  ``FrontendConfig.ransac_enabled = True`` puts
the two-point RANSAC the stub stands for (Sun et al., msckf_vio) in its place:
one device call per frame over the cam0 and cam1 temporal matches with the
IMU-predicted rotations, ``ransac_threshold`` its inlier error in pixels, the
hypothesis draws from a seeded generator (``ransac_seed``) so that a replay
repeats.  ``FrontendConfig.device_pipeline = True`` makes ``stereo_match`` one
device call instead of six and the mask, detection and per-cell sieve of
``add_new_features`` one call instead of a host mask, ``mfe_fast`` and a Python
loop over every keypoint; the published messages are the same.  There is no
CPU fallback: without the HIP library or a GPU the
constructor raises.
"""
from __future__ import annotations

import ctypes as C
from collections import defaultdict, namedtuple
from dataclasses import dataclass, field
from itertools import chain

import numpy as np

from . import _lib
from .config import _default_T_imu_cam0
from .msckf import FeatureArrays, TrackMessage, message_arrays

RADTAN, EQUIDISTANT = 0, 1
_I32P = C.POINTER(C.c_int32)
_I64P = C.POINTER(C.c_int64)

FeatureMeasurement = namedtuple("FeatureMeasurement", ["id", "u0", "v0", "u1", "v1"])
FeatureMsg = namedtuple("vio_feature_msg__", ["timestamp", "vio_features"])


def _as_arrays(msg):
    """A FeatureMsg as msckf.FeatureArrays (an array message stays as it is; None stays None)."""
    if msg is None or isinstance(msg, FeatureArrays):
        return msg
    ids, uv = message_arrays(msg)
    return FeatureArrays(msg.timestamp, ids, uv)


class RansacInfo(namedtuple("RansacInfo", ["status", "n_raw", "scale", "unit", "mean_dist", "best_h", "best_count",
                                           "m_refit", "refit_err"])):
    """One set's info record of mfe_two_point_ransac (msckf_ransac.h).  status:
    0 = RANSAC ran, 1 = degenerate motion, 2 = fewer than 3 points after the
    pre-filter, 3 = no hypothesis qualified; undefined fields are NaN."""
    __slots__ = ()

    @classmethod
    def from_row(cls, row):
        r = np.asarray(row, float)
        return cls(int(r[0]), int(r[1]), float(r[2]), float(r[3]), float(r[4]), int(r[5]), int(r[6]),
                   r[7:10].copy(), float(r[10]))


def ransac_hypotheses(success_probability):
    """Number of two-point hypotheses for the given success probability at an
    assumed inlier share of 0.7 (msckf_vio): 7 at 0.99."""
    return int(np.ceil(np.log(1.0 - success_probability) / np.log(1.0 - 0.7 * 0.7)))


def _default_T_imu_cam1():
    return np.array([
        [0.012555267089103, 0.999598781151433, -0.025389800891747, -0.044901980682509],
        [-0.999755099723116, 0.013011905181504, 0.017900583825251, -0.020569771258915],
        [0.018223771455443, 0.025158836311552, 0.999517347077547, -0.008638135126028],
        [0, 0, 0, 1.000000000000000]])


@dataclass
class FrontendConfig:
    """Image-processor fields of the reference ConfigEuRoC (config.py:22-44,
    94-121); defaults are the reference's."""
    grid_row: int = 4
    grid_col: int = 5
    grid_min_feature_num: int = 3
    grid_max_feature_num: int = 5
    fast_threshold: int = 15
    ransac_threshold: float = 3
    stereo_threshold: float = 5
    max_iteration: int = 30
    track_precision: float = 0.01
    pyramid_levels: int = 3
    patch_size: int = 15
    T_imu_cam0: np.ndarray = field(default_factory=_default_T_imu_cam0)
    T_imu_cam1: np.ndarray = field(default_factory=_default_T_imu_cam1)
    cam0_distortion_model: str = "radtan"
    cam0_distortion_coeffs: np.ndarray = field(
        default_factory=lambda: np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05]))
    cam0_intrinsics: np.ndarray = field(default_factory=lambda: np.array([458.654, 457.296, 367.215, 248.375]))
    cam0_resolution: np.ndarray = field(default_factory=lambda: np.array([752, 480]))
    cam1_distortion_model: str = "radtan"
    cam1_distortion_coeffs: np.ndarray = field(
        default_factory=lambda: np.array([-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05]))
    cam1_intrinsics: np.ndarray = field(default_factory=lambda: np.array([457.587, 456.134, 379.999, 255.238]))
    cam1_resolution: np.ndarray = field(default_factory=lambda: np.array([752, 480]))
    # not in the reference: the two-point RANSAC its track_features stubs (off = the stub);
    # ransac_threshold above is its inlier error in pixels
    ransac_enabled: bool = False
    ransac_success_probability: float = 0.99
    ransac_seed: int = 0
    # not in the reference: stereo_match and the detection + sieve of add_new_features each as
    # one device call (include/msckf_pipeline.h) instead of Python around many small ones;
    # the published messages are the same
    device_pipeline: bool = False
    # not in the reference: a MultiImageProcessor keeps the feature tracks on the device and runs a
    # whole tracked frame of all lanes as one call (include/msckf_tracks.h); needs device_pipeline;
    # the published messages are the same
    device_tracks: bool = False
    # not in the reference: every uploaded image is equalised on the device before its pyramid is
    # built (include/msckf_equalize.h), "none" | "hist" (cv2.equalizeHist) | "clahe" (cv2.createCLAHE
    # with the two fields below, OpenCV's defaults); detection, tracking and the stereo match then
    # read the equalised image
    equalize: str = "none"
    clahe_clip_limit: float = 40.0
    clahe_tiles: tuple = (8, 8)
    # not in the reference: a device_tracks lane also leaves the frame's motion statistic on the
    # device (include/msckf_standstill.h): the track_motion_quantile of the squared pixel
    # displacement of the tracks that survived the frame's tracking; the messages are the same
    track_motion: bool = False
    track_motion_quantile: float = 0.5

    @property
    def grid_num(self):
        return self.grid_row * self.grid_col

    @classmethod
    def from_reference(cls, ref_cfg) -> "FrontendConfig":
        g = lambda n: getattr(ref_cfg, "_vio_%s__" % n)
        kw = {}
        for f in cls.__dataclass_fields__:
            try:
                kw[f] = g(f)
            except AttributeError:
                pass
        return cls(**kw)


EQ_MODES = {"none": _lib.EQ_NONE, "hist": _lib.EQ_HIST, "clahe": _lib.EQ_CLAHE}


def _check_tiles(tiles, W, H):
    """clahe_tiles as (tiles_x, tiles_y) of ints within msckf_equalize.h's limits for a W x H image."""
    try:
        tx, ty = (int(v) for v in tiles)
        if (tx, ty) != tuple(tiles):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("clahe_tiles = %r, expected two integers (tiles_x, tiles_y)" % (tiles,)) from None
    if not (1 <= tx <= min(_lib.EQ_MAX_TILES, W) and 1 <= ty <= min(_lib.EQ_MAX_TILES, H)):
        raise ValueError("clahe_tiles = %r outside [1, %d] or above the image size %dx%d"
                         % (tiles, _lib.EQ_MAX_TILES, W, H))
    return tx, ty


def _equalize_of(config, W, H):
    """The equalisation argument of Frontend.upload for a config: None for
    "none", else (mode, clip_limit, (tiles_x, tiles_y)); ValueError on a bad field."""
    if config.equalize not in EQ_MODES:
        raise ValueError("equalize = %r, expected one of %s" % (config.equalize, sorted(EQ_MODES)))
    tiles = _check_tiles(config.clahe_tiles, W, H)
    clip = float(config.clahe_clip_limit)
    if np.isnan(clip):
        raise ValueError("clahe_clip_limit is NaN")
    return None if config.equalize == "none" else (config.equalize, clip, tiles)


class FeatureMetaData:
    """Reference FeatureMetaData (image.py:11-20)."""
    __slots__ = ("id", "response", "lifetime", "cam0_point", "cam1_point")

    def __init__(self):
        self.id = None
        self.response = None
        self.lifetime = None
        self.cam0_point = None
        self.cam1_point = None


def _inv_T(T):
    T = np.asarray(T, float)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def _rodrigues(r):
    """cv2.Rodrigues of a rotation vector (image.py:482)."""
    r = np.asarray(r, float).reshape(3)
    th = float(np.linalg.norm(r))
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * K


def _skew(v):
    x, y, z = v
    return np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], float)


def _select(data, selectors):
    """Reference select (image.py:728-729)."""
    return [d for d, s in zip(data, selectors) if s]


class Frontend:
    """Device context of the image operators (C-ABI ``mfe_*``)."""

    def __init__(self, width, height, nslot=4, max_level=3, max_points=4096, device=0):
        self.lib = _lib.load_library()
        self.W, self.H, self.max_points = int(width), int(height), int(max_points)
        h = C.c_void_p()
        self._check(self.lib.mfe_create(device, self.W, self.H, nslot, max_level, self.max_points, C.byref(h)))
        self.h = h
        self.tracks_cap = 0   # tracks_create

    def _check(self, rc):
        if rc < 0:
            raise _lib.MsckfError("mfe: %s (rc=%d)" % (self.lib.mfe_last_error().decode(), rc))
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.mfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, slot, image, equalize=None):
        """mfe_upload; with ``equalize`` = (mode, clip_limit, (tiles_x, tiles_y)),
        mode "none" | "hist" | "clahe", the image is equalised on the device
        first (msckf_equalize.h): the set call ``upload_many`` with one image."""
        img = np.ascontiguousarray(image, np.uint8)
        if img.shape != (self.H, self.W):
            raise ValueError("image shape %s, context %dx%d" % (img.shape, self.W, self.H))
        if equalize is not None:
            mode, clip, tiles = equalize
            return self.upload_many([slot], img[None], ([mode], [clip], tiles))
        self._check(self.lib.mfe_upload(self.h, slot, img.ctypes.data_as(C.POINTER(C.c_uint8))))

    def download(self, slot, level=0):
        """mfe_download: level ``level`` of a slot as the device holds it, uint8 (h_l, w_l)."""
        w, h = self.W, self.H
        for _ in range(max(int(level), 0)):
            w, h = (w + 1) // 2, (h + 1) // 2
        out = np.zeros((h, w), np.uint8)
        self._check(self.lib.mfe_download(self.h, int(slot), int(level), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def download_deriv(self, slot, level=0):
        """mfe_download_deriv: the Scharr planes (ix, iy) of level ``level`` of a slot
        as the device holds them, int16 (h_l, w_l) each."""
        w, h = self.W, self.H
        for _ in range(max(int(level), 0)):
            w, h = (w + 1) // 2, (h + 1) // 2
        ix, iy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
        i16 = C.POINTER(C.c_int16)
        self._check(self.lib.mfe_download_deriv(self.h, int(slot), int(level), ix.ctypes.data_as(i16),
                                                iy.ctypes.data_as(i16)))
        return ix, iy

    def fast(self, slot, threshold, mask=None, max_kp=1 << 16):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        xy = np.zeros((max_kp, 2), np.float32)
        resp = np.zeros(max_kp, np.float32)
        n = C.c_int(0)
        self._check(self.lib.mfe_fast(self.h, slot, int(threshold),
                                      None if m is None else m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      max_kp, xy.ctypes.data_as(C.POINTER(C.c_float)),
                                      resp.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        k = min(n.value, max_kp)
        return xy[:k].copy(), resp[:k].copy()

    def lk(self, slot_prev, slot_next, prev_pts, next_pts, win=15, max_level=3, max_iter=30, eps=0.01):
        p = np.ascontiguousarray(np.asarray(prev_pts, np.float32).reshape(-1, 2))
        q = np.ascontiguousarray(np.asarray(next_pts, np.float32).reshape(-1, 2)).copy()
        n = len(p)
        st = np.zeros(n, np.uint8)
        if n == 0:
            return q, st
        if n > self.max_points:
            raise ValueError("%d points exceed the context's %d" % (n, self.max_points))
        self._check(self.lib.mfe_lk(self.h, slot_prev, slot_next, n, p.ctypes.data_as(C.POINTER(C.c_float)),
                                    q.ctypes.data_as(C.POINTER(C.c_float)), st.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    int(win), int(max_level), int(max_iter), float(eps)))
        return q, st

    def _cam(self, fn, pts, *args):
        p = np.ascontiguousarray(np.asarray(pts, float).reshape(-1, 2))
        out = np.zeros_like(p)
        if len(p) == 0:
            return out
        if len(p) > self.max_points:
            raise ValueError("%d points exceed the context's %d" % (len(p), self.max_points))
        dp = C.POINTER(C.c_double)
        conv = [a.ctypes.data_as(dp) if isinstance(a, np.ndarray) else a for a in args]
        self._check(fn(self.h, len(p), p.ctypes.data_as(dp), out.ctypes.data_as(dp), *conv))
        return out

    def undistort(self, pts, intrinsics, model, coeffs, R=None, new_intrinsics=None):
        f64 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, float).ravel())
        return self._cam(self.lib.mfe_undistort, pts, f64(intrinsics), int(model), f64(coeffs), f64(R),
                         f64(new_intrinsics))

    def distort(self, pts, intrinsics, model, coeffs):
        f64 = lambda a: np.ascontiguousarray(np.asarray(a, float).ravel())
        return self._cam(self.lib.mfe_distort, pts, f64(intrinsics), int(model), f64(coeffs))

    def two_point_ransac(self, sets, inlier_error, n_hyp, draws):
        """mfe_two_point_ransac (include/msckf_ransac.h) over a list of point
        sets in one launch.  ``sets``: (pts_prev, pts_curr, R_p_c, intrinsics,
        model, coeffs) per set, points in pixels; ``draws``: uint32 (n_sets,
        n_hyp, 2).  Returns one (inliers bool array, RansacInfo) per set."""
        S = len(sets)
        prev = [np.asarray(s[0], float).reshape(-1, 2) for s in sets]
        curr = [np.asarray(s[1], float).reshape(-1, 2) for s in sets]
        for p, q in zip(prev, curr):
            if len(p) != len(q):
                raise ValueError("a set's point lists differ in length (%d, %d)" % (len(p), len(q)))
        off = np.zeros(S + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in prev])
        T = int(off[-1])
        draws = np.ascontiguousarray(draws, np.uint32)
        if draws.shape != (S, int(n_hyp), 2):
            raise ValueError("draws of shape %s, expected %s" % (draws.shape, (S, int(n_hyp), 2)))
        cat = lambda a, w: np.ascontiguousarray(np.concatenate(a).reshape(-1, w)) if a else np.zeros((0, w))
        pp, pc = cat(prev, 2), cat(curr, 2)
        R = cat([np.asarray(s[2], float).reshape(1, 9) for s in sets], 9)
        K = cat([np.asarray(s[3], float).reshape(1, 4) for s in sets], 4)
        model = np.array([int(s[4]) for s in sets], np.int32)
        k = cat([np.asarray(s[5], float).reshape(1, 4) for s in sets], 4)
        inl = np.zeros(T, np.uint8)
        # the record of an empty set; a call without points launches nothing and leaves it
        info = np.full((S, _lib.RANSAC_INFO_LEN), np.nan)
        info[:, [0, 1, 5, 6, 11]] = [2.0, 0.0, -1.0, 0.0, 0.0]
        dp = C.POINTER(C.c_double)
        ip = C.POINTER(C.c_int32)
        self._check(self.lib.mfe_two_point_ransac(
            self.h, S, off.ctypes.data_as(ip), pp.ctypes.data_as(dp), pc.ctypes.data_as(dp), R.ctypes.data_as(dp),
            K.ctypes.data_as(dp), model.ctypes.data_as(ip), k.ctypes.data_as(dp), float(inlier_error), int(n_hyp),
            draws.ctypes.data_as(C.POINTER(C.c_uint32)), inl.ctypes.data_as(C.POINTER(C.c_uint8)),
            info.ctypes.data_as(dp)))
        return [(inl[off[s]:off[s + 1]].astype(bool), RansacInfo.from_row(info[s])) for s in range(S)]

    def stereo_match(self, slot_cam0, slot_cam1, cam0_pts, cam0, cam1, R_guess, E, stereo_threshold,
                     win=15, max_level=3, max_iter=30, eps=0.01):
        """mfe_stereo_match (include/msckf_pipeline.h): ImageProcessor.stereo_match
        in one device call.  ``cam0`` / ``cam1``: (intrinsics, model, coeffs);
        ``R_guess``: the rotation of the initial guess; ``E``: the essential
        matrix.  Returns (cam1_pts float32 (n, 2), inlier uint8, reason uint8);
        the forward LK status is ``reason != 1``."""
        p = np.ascontiguousarray(np.asarray(cam0_pts, float).reshape(-1, 2))
        n = len(p)
        c1 = np.zeros((n, 2), np.float32)
        inl, rsn = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        if n == 0:
            return c1, inl, rsn
        if n > self.max_points:
            raise ValueError("%d points exceed the context's %d" % (n, self.max_points))
        f64 = lambda a, m: np.ascontiguousarray(np.asarray(a, float).ravel()[:m])
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        K0, k0, K1, k1 = f64(cam0[0], 4), f64(cam0[2], 4), f64(cam1[0], 4), f64(cam1[2], 4)
        R, Em = f64(R_guess, 9), f64(E, 9)
        if min(len(K0), len(k0), len(K1), len(k1)) < 4 or len(R) < 9 or len(Em) < 9:
            raise ValueError("camera arguments: 4 intrinsics, 4 coefficients, 3x3 R_guess and E")
        self._check(self.lib.mfe_stereo_match(
            self.h, int(slot_cam0), int(slot_cam1), n, p.ctypes.data_as(dp), K0.ctypes.data_as(dp), int(cam0[1]),
            k0.ctypes.data_as(dp), K1.ctypes.data_as(dp), int(cam1[1]), k1.ctypes.data_as(dp), R.ctypes.data_as(dp),
            Em.ctypes.data_as(dp), int(win), int(max_level), int(max_iter), float(eps), float(stereo_threshold),
            c1.ctypes.data_as(C.POINTER(C.c_float)), inl.ctypes.data_as(u8), rsn.ctypes.data_as(u8)))
        return c1, inl, rsn

    def fast_grid(self, slot, threshold, occupied, grid_row, grid_col, k, max_kp=1 << 16):
        """mfe_fast_grid (include/msckf_pipeline.h): masked FAST detection and the
        per-cell selection in one device call.  ``occupied``: float32 xy of the
        points whose 7 x 7 neighbourhoods are masked out.  Returns (xy float32
        (m, 2), response float32 (m,), cell_count int32 (grid_row * grid_col,),
        n_total): the kept keypoints grouped by cell, response-descending with
        raster ties; raises if n_total exceeds ``max_kp``."""
        occ = np.ascontiguousarray(np.asarray(occupied, np.float32).reshape(-1, 2))
        if len(occ) > self.max_points:
            raise ValueError("%d points exceed the context's %d" % (len(occ), self.max_points))
        cells = int(grid_row) * int(grid_col)
        if not (1 <= int(k) <= _lib.GRID_MAX_K and int(grid_row) >= 1 and int(grid_col) >= 1 and
                cells <= _lib.GRID_MAX_CELLS):
            raise ValueError("grid %dx%d, k = %d outside the limits of msckf_pipeline.h" % (grid_row, grid_col, k))
        xy = np.zeros((cells * int(k), 2), np.float32)
        resp = np.zeros(cells * int(k), np.float32)
        cnt = np.zeros(cells, np.int32)
        n = C.c_int(0)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_fast_grid(self.h, int(slot), int(threshold), len(occ),
                                           occ.ctypes.data_as(fp) if len(occ) else None, int(grid_row),
                                           int(grid_col), int(k), int(max_kp), xy.ctypes.data_as(fp),
                                           resp.ctypes.data_as(fp), cnt.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.byref(n)))
        m = int(np.minimum(cnt, int(k)).sum())
        return xy[:m].copy(), resp[:m].copy(), cnt, n.value

    # ---- the calls over many streams' sets (include/msckf_lanes.h): one device call for a
    # list of sets, one result per set in the shape of the single method ----
    def _set_off(self, lens):
        off = np.zeros(len(lens) + 1, np.int32)
        np.cumsum(lens, out=off[1:])
        if int(off[-1]) > self.max_points:
            raise ValueError("%d points in all sets exceed the context's %d" % (off[-1], self.max_points))
        return off

    def upload_many(self, slots, images, equalize=None):
        """mfe_upload_many: ``images[i]`` into ``slots[i]`` (distinct), all
        pyramids built by launches over the image index.  With ``equalize`` =
        (modes, clip_limits, (tiles_x, tiles_y)), one mode ("none" | "hist" |
        "clahe", or its MFE_EQ_* number) and one clip limit per image, it is
        mfe_upload_many_eq (msckf_equalize.h): each image is equalised on the
        device before its pyramid is built."""
        sl = np.ascontiguousarray(slots, np.int32)
        imgs = np.ascontiguousarray(images, np.uint8)
        if imgs.shape != (len(sl), self.H, self.W):
            raise ValueError("images of shape %s, expected %s" % (imgs.shape, (len(sl), self.H, self.W)))
        if equalize is None:
            self._check(self.lib.mfe_upload_many(self.h, len(sl), sl.ctypes.data_as(_I32P),
                                                 imgs.ctypes.data_as(C.POINTER(C.c_uint8))))
            return
        modes, clips, tiles = equalize
        try:
            mode = np.array([EQ_MODES[m] if isinstance(m, str) else int(m) for m in modes], np.int32)
        except KeyError as e:
            raise ValueError("equalisation mode %s, expected one of %s" % (e, sorted(EQ_MODES))) from None
        clip = np.ascontiguousarray(clips, np.float32).reshape(-1)
        if len(mode) != len(sl) or len(clip) != len(sl):
            raise ValueError("%d modes and %d clip limits for %d images" % (len(mode), len(clip), len(sl)))
        self._check(self.lib.mfe_upload_many_eq(self.h, len(sl), sl.ctypes.data_as(_I32P),
                                                imgs.ctypes.data_as(C.POINTER(C.c_uint8)), mode.ctypes.data_as(_I32P),
                                                clip.ctypes.data_as(C.POINTER(C.c_float)), int(tiles[0]),
                                                int(tiles[1])))

    def lk_sets(self, sets, win=15, max_level=3, max_iter=30, eps=0.01):
        """mfe_lk_sets.  ``sets``: (slot_prev, slot_next, prev_pts, next_pts) per
        set.  Returns one (next_pts float32 (n, 2), status uint8) per set."""
        prev = [np.asarray(s[2], np.float32).reshape(-1, 2) for s in sets]
        nxt = [np.asarray(s[3], np.float32).reshape(-1, 2) for s in sets]
        for p, q in zip(prev, nxt):
            if len(p) != len(q):
                raise ValueError("a set's point lists differ in length (%d, %d)" % (len(p), len(q)))
        off = self._set_off([len(p) for p in prev])
        T = int(off[-1])
        p = np.ascontiguousarray(np.concatenate(prev)) if sets else np.zeros((0, 2), np.float32)
        q = np.ascontiguousarray(np.concatenate(nxt)) if sets else np.zeros((0, 2), np.float32)
        st = np.zeros(T, np.uint8)
        s0 = np.array([int(s[0]) for s in sets], np.int32)
        s1 = np.array([int(s[1]) for s in sets], np.int32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_lk_sets(self.h, len(sets), off.ctypes.data_as(_I32P), s0.ctypes.data_as(_I32P),
                                         s1.ctypes.data_as(_I32P), p.ctypes.data_as(fp), q.ctypes.data_as(fp),
                                         st.ctypes.data_as(C.POINTER(C.c_uint8)), int(win), int(max_level),
                                         int(max_iter), float(eps)))
        return [(q[off[i]:off[i + 1]], st[off[i]:off[i + 1]]) for i in range(len(sets))]

    def stereo_match_sets(self, sets, win=15, max_level=3, max_iter=30, eps=0.01):
        """mfe_stereo_match_sets.  ``sets``: (slot_cam0, slot_cam1, cam0_pts,
        cam0, cam1, R_guess, E, stereo_threshold) per set, the arguments of
        ``stereo_match``.  Returns one (cam1_pts, inlier, reason) per set."""
        S = len(sets)
        pts = [np.asarray(s[2], float).reshape(-1, 2) for s in sets]
        off = self._set_off([len(p) for p in pts])
        T = int(off[-1])
        p = np.ascontiguousarray(np.concatenate(pts)) if sets else np.zeros((0, 2))
        row = lambda get, w: np.ascontiguousarray(
            np.array([np.asarray(get(s), float).ravel()[:w] for s in sets], float).reshape(S, w))
        K0, k0 = row(lambda s: s[3][0], 4), row(lambda s: s[3][2], 4)
        K1, k1 = row(lambda s: s[4][0], 4), row(lambda s: s[4][2], 4)
        R, E = row(lambda s: s[5], 9), row(lambda s: s[6], 9)
        thr = np.array([float(s[7]) for s in sets], float)
        i32 = lambda get: np.array([int(get(s)) for s in sets], np.int32)
        s0, s1, m0, m1 = i32(lambda s: s[0]), i32(lambda s: s[1]), i32(lambda s: s[3][1]), i32(lambda s: s[4][1])
        c1 = np.zeros((T, 2), np.float32)
        inl, rsn = np.zeros(T, np.uint8), np.zeros(T, np.uint8)
        dp, u8 = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        self._check(self.lib.mfe_stereo_match_sets(
            self.h, S, off.ctypes.data_as(_I32P), s0.ctypes.data_as(_I32P), s1.ctypes.data_as(_I32P),
            p.ctypes.data_as(dp), K0.ctypes.data_as(dp), m0.ctypes.data_as(_I32P), k0.ctypes.data_as(dp),
            K1.ctypes.data_as(dp), m1.ctypes.data_as(_I32P), k1.ctypes.data_as(dp), R.ctypes.data_as(dp),
            E.ctypes.data_as(dp), thr.ctypes.data_as(dp), int(win), int(max_level), int(max_iter), float(eps),
            c1.ctypes.data_as(C.POINTER(C.c_float)), inl.ctypes.data_as(u8), rsn.ctypes.data_as(u8)))
        return [(c1[off[i]:off[i + 1]], inl[off[i]:off[i + 1]], rsn[off[i]:off[i + 1]]) for i in range(S)]

    def fast_grid_sets(self, sets, threshold, grid_row, grid_col, k, max_kp=1 << 16):
        """mfe_fast_grid_sets.  ``sets``: (slot, occupied) per set.  Returns one
        (xy, response, cell_count, n_total) per set, as ``fast_grid``; raises
        if any set's n_total exceeds ``max_kp``."""
        S = len(sets)
        occ = [np.asarray(s[1], np.float32).reshape(-1, 2) for s in sets]
        off = self._set_off([len(o) for o in occ])
        cells, k = int(grid_row) * int(grid_col), int(k)
        if not (1 <= k <= _lib.GRID_MAX_K and int(grid_row) >= 1 and int(grid_col) >= 1 and
                cells <= _lib.GRID_MAX_CELLS):
            raise ValueError("grid %dx%d, k = %d outside the limits of msckf_pipeline.h" % (grid_row, grid_col, k))
        o = np.ascontiguousarray(np.concatenate(occ)) if sets else np.zeros((0, 2), np.float32)
        sl = np.array([int(s[0]) for s in sets], np.int32)
        xy = np.zeros((S, cells * k, 2), np.float32)
        resp = np.zeros((S, cells * k), np.float32)
        cnt = np.zeros((S, cells), np.int32)
        tot = np.zeros(S, np.int32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_fast_grid_sets(
            self.h, S, sl.ctypes.data_as(_I32P), off.ctypes.data_as(_I32P), o.ctypes.data_as(fp) if len(o) else None,
            int(threshold), int(grid_row), int(grid_col), k, int(max_kp), xy.ctypes.data_as(fp),
            resp.ctypes.data_as(fp), cnt.ctypes.data_as(_I32P), tot.ctypes.data_as(_I32P)))
        m = np.minimum(cnt, k).sum(axis=1)
        return [(xy[i, :m[i]].copy(), resp[i, :m[i]].copy(), cnt[i], int(tot[i])) for i in range(S)]

    def undistort_sets(self, sets):
        """mfe_undistort_sets.  ``sets``: (pts, intrinsics, model, coeffs, R,
        new_intrinsics) per set, the arguments of ``undistort`` (R and
        new_intrinsics may be None).  Returns one float64 (n, 2) per set."""
        S = len(sets)
        pts = [np.asarray(s[0], float).reshape(-1, 2) for s in sets]
        off = self._set_off([len(p) for p in pts])
        p = np.ascontiguousarray(np.concatenate(pts)) if sets else np.zeros((0, 2))
        out = np.zeros_like(p)
        row = lambda j, w, dflt: np.ascontiguousarray(np.array(
            [np.asarray(dflt if s[j] is None else s[j], float).ravel()[:w] for s in sets], float).reshape(S, w))
        K, k = row(1, 4, None), row(3, 4, None)
        R, nK = row(4, 9, np.identity(3)), row(5, 4, (1.0, 1.0, 0.0, 0.0))
        model = np.array([int(s[2]) for s in sets], np.int32)
        dp = C.POINTER(C.c_double)
        self._check(self.lib.mfe_undistort_sets(self.h, S, off.ctypes.data_as(_I32P), p.ctypes.data_as(dp),
                                                out.ctypes.data_as(dp), K.ctypes.data_as(dp),
                                                model.ctypes.data_as(_I32P), k.ctypes.data_as(dp),
                                                R.ctypes.data_as(dp), nK.ctypes.data_as(dp)))
        return [out[off[i]:off[i + 1]] for i in range(S)]

    # ---- the feature tracks kept on the device (include/msckf_tracks.h) ----
    def tracks_create(self, n_lanes, cap, grid_row, grid_col, grid_min, grid_max):
        """mfe_tracks_create: two tables of ``cap`` rows per lane, in this context."""
        self._check(self.lib.mfe_tracks_create(self.h, int(n_lanes), int(cap), int(grid_row), int(grid_col),
                                               int(grid_min), int(grid_max)))
        self.tracks_cap = int(cap)

    def tracks_put(self, lane, ids, lifetimes, cam0, cam1, next_id):
        """mfe_tracks_put: the lane's current table (rows in publish order)."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        life = np.ascontiguousarray(lifetimes, np.int32).reshape(-1)
        c0 = np.ascontiguousarray(np.asarray(cam0, np.float32).reshape(-1, 2))
        c1 = np.ascontiguousarray(np.asarray(cam1, np.float32).reshape(-1, 2))
        if not len(ids) == len(life) == len(c0) == len(c1):
            raise ValueError("table columns of %d, %d, %d, %d rows" % (len(ids), len(life), len(c0), len(c1)))
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_tracks_put(self.h, int(lane), len(ids), ids.ctypes.data_as(_I64P),
                                            life.ctypes.data_as(_I32P), c0.ctypes.data_as(fp), c1.ctypes.data_as(fp),
                                            int(next_id)))

    def tracks_get(self, lane):
        """mfe_tracks_get: (ids int64, lifetimes int32, cam0 float32 (n, 2), cam1, next_id)."""
        cap = self.tracks_cap
        ids, life = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        c0, c1 = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        n, nxt = C.c_int32(0), C.c_int64(0)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_tracks_get(self.h, int(lane), C.byref(n), ids.ctypes.data_as(_I64P),
                                            life.ctypes.data_as(_I32P), c0.ctypes.data_as(fp), c1.ctypes.data_as(fp),
                                            C.byref(nxt)))
        k = n.value
        return ids[:k].copy(), life[:k].copy(), c0[:k].copy(), c1[:k].copy(), nxt.value

    # ---- the motion statistic (include/msckf_standstill.h) ----
    def motion_sets(self, sets, q=0.5):
        """mfe_motion_sets: per set (prev, curr) of float32 (n, 2) pixel pairs
        the q-quantile (k = floor(q (n - 1))) of the squared displacement.
        Returns (n int32 [S], d2 float32 [S]); an empty set gives NaN."""
        prev = [np.asarray(p, np.float32).reshape(-1, 2) for p, _ in sets]
        curr = [np.asarray(c, np.float32).reshape(-1, 2) for _, c in sets]
        if any(len(p) != len(c) for p, c in zip(prev, curr)):
            raise ValueError("a set's prev and curr differ in length")
        S = len(sets)
        off = self._set_off([len(p) for p in prev])
        P = np.ascontiguousarray(np.concatenate(prev) if S else np.zeros((0, 2)), np.float32)
        Q = np.ascontiguousarray(np.concatenate(curr) if S else np.zeros((0, 2)), np.float32)
        n, d2 = np.zeros(S, np.int32), np.zeros(S, np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.mfe_motion_sets(self.h, S, off.ctypes.data_as(_I32P), P.ctypes.data_as(fp),
                                             Q.ctypes.data_as(fp), float(q), n.ctypes.data_as(_I32P),
                                             d2.ctypes.data_as(fp)))
        return n, d2

    def tracks_motion_enable(self, on=True, q=0.5):
        """mfe_tracks_motion_enable: the steps of this context leave each named
        lane's motion record on the device (needs tracks_create)."""
        self._check(self.lib.mfe_tracks_motion_enable(self.h, int(bool(on)), float(q)))

    def tracks_motion_get(self, lane):
        """mfe_tracks_motion_get (synchronises): (valid, n, d2 float32) of the
        lane's record; (False, 0, NaN) without a valid one."""
        valid, n, d2 = C.c_int32(0), C.c_int32(0), C.c_float(0.0)
        self._check(self.lib.mfe_tracks_motion_get(self.h, int(lane), C.byref(valid), C.byref(n), C.byref(d2)))
        return bool(valid.value), int(n.value), np.float32(d2.value)

    def tracks_msg_put(self, lane, ids, uv):
        """mfe_tracks_msg_put (msckf_handoff.h): the lane's message, ids int64
        [n] and uv float64 [n][4], written from the host."""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 4)
        if len(ids) != len(uv):
            raise ValueError("a message of %d ids and %d coordinate rows" % (len(ids), len(uv)))
        self._check(self.lib.mfe_tracks_msg_put(self.h, int(lane), len(ids), ids.ctypes.data_as(_I64P),
                                                uv.ctypes.data_as(C.POINTER(C.c_double))))

    def tracks_msg_get(self, lane):
        """mfe_tracks_msg_get: (valid, ids int64 [n], uv float64 [n][4]) of
        the lane's message; empty arrays without a valid one."""
        cap = self.tracks_cap
        ids, uv = np.zeros(cap, np.int64), np.zeros((cap, 4))
        valid, n = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.mfe_tracks_msg_get(self.h, int(lane), C.byref(valid), C.byref(n),
                                                ids.ctypes.data_as(_I64P), uv.ctypes.data_as(C.POINTER(C.c_double))))
        return bool(valid.value), ids[:n.value].copy(), uv[:n.value].copy()

    def tracks_step(self, lanes, threshold, max_kp=1 << 16, inlier_error=0.0, n_hyp=0, win=15, max_level=3,
                    max_iter=30, eps=0.01, to_message=False):
        """mfe_tracks_step: one tracked frame for each ``TracksLane`` of
        ``lanes``.  Returns one ``TracksResult`` per lane.  If a lane's
        detection exceeds ``max_kp`` the MsckfError raised carries every
        lane's ``n_total`` and no table has changed.  ``to_message``:
        mfe_tracks_step_msg (msckf_handoff.h) -- ids and uv stay on the device
        as the lanes' messages, and the results carry None in their place."""
        S, cap = len(lanes), self.tracks_cap
        i32 = lambda get: np.array([int(get(a)) for a in lanes], np.int32)
        row = lambda get, w: np.ascontiguousarray(
            np.array([np.asarray(get(a), float).ravel()[:w] for a in lanes], float).reshape(S, w))
        ln, sp, s0, s1 = i32(lambda a: a.lane), i32(lambda a: a.slot_prev), i32(lambda a: a.slot_c0), \
            i32(lambda a: a.slot_c1)
        Hp = row(lambda a: a.Hpred, 9)
        K0, k0, m0 = row(lambda a: a.cam0[0], 4), row(lambda a: a.cam0[2], 4), i32(lambda a: a.cam0[1])
        K1, k1, m1 = row(lambda a: a.cam1[0], 4), row(lambda a: a.cam1[2], 4), i32(lambda a: a.cam1[1])
        Rg, E = row(lambda a: a.R_guess, 9), row(lambda a: a.E, 9)
        thr = np.array([float(a.stereo_threshold) for a in lanes], float)
        flag = i32(lambda a: a.ransac is not None)
        n_hyp = int(n_hyp)
        R0, R1 = np.zeros((S, 9)), np.zeros((S, 9))
        draws = np.zeros((S, 2, max(n_hyp, 0), 2), np.uint32)
        for i, a in enumerate(lanes):
            if a.ransac is not None:
                R0[i], R1[i] = np.asarray(a.ransac[0], float).ravel(), np.asarray(a.ransac[1], float).ravel()
                dr = np.asarray(a.ransac[2], np.uint32)
                if dr.shape != draws.shape[1:]:
                    raise ValueError("draws of shape %s, expected %s" % (dr.shape, draws.shape[1:]))
                draws[i] = dr
        n = np.zeros(S, np.int32)
        ctr = np.zeros((S, _lib.TRACKS_COUNTERS), np.int32)
        tot = np.zeros(S, np.int32)
        nxt = np.zeros(S, np.int64)
        dp = C.POINTER(C.c_double)
        if to_message:
            outs = ()
            fn = self.lib.mfe_tracks_step_msg
        else:
            ids = np.zeros((S, cap), np.int64)
            uv = np.zeros((S, cap, 4))
            outs = (ids.ctypes.data_as(_I64P), uv.ctypes.data_as(dp))
            fn = self.lib.mfe_tracks_step
        rc = fn(
            self.h, S, ln.ctypes.data_as(_I32P), sp.ctypes.data_as(_I32P), s0.ctypes.data_as(_I32P),
            s1.ctypes.data_as(_I32P), Hp.ctypes.data_as(dp), K0.ctypes.data_as(dp), m0.ctypes.data_as(_I32P),
            k0.ctypes.data_as(dp), K1.ctypes.data_as(dp), m1.ctypes.data_as(_I32P), k1.ctypes.data_as(dp),
            Rg.ctypes.data_as(dp), E.ctypes.data_as(dp), thr.ctypes.data_as(dp), flag.ctypes.data_as(_I32P),
            R0.ctypes.data_as(dp), R1.ctypes.data_as(dp), draws.ctypes.data_as(C.POINTER(C.c_uint32)), int(win),
            int(max_level), int(max_iter), float(eps), int(threshold), int(max_kp), float(inlier_error), n_hyp,
            n.ctypes.data_as(_I32P), *outs, ctr.ctypes.data_as(_I32P), tot.ctypes.data_as(_I32P),
            nxt.ctypes.data_as(_I64P))
        if rc == -3:
            err = _lib.MsckfError("mfe: %s (rc=%d)" % (self.lib.mfe_last_error().decode(), rc))
            err.n_total = tot.copy()
            raise err
        self._check(rc)
        if to_message:
            return [TracksResult(int(n[i]), None, None, ctr[i].copy(), int(tot[i]), int(nxt[i])) for i in range(S)]
        return [TracksResult(int(n[i]), ids[i, :n[i]].copy(), uv[i, :n[i]].copy(), ctr[i].copy(), int(tot[i]),
                             int(nxt[i])) for i in range(S)]


# one lane's arguments of Frontend.tracks_step (include/msckf_tracks.h): cam0 / cam1 are (intrinsics,
# model, coeffs); ransac is None or (R0, R1, draws uint32 (2, n_hyp, 2))
TracksLane = namedtuple("TracksLane", ["lane", "slot_prev", "slot_c0", "slot_c1", "Hpred", "cam0", "cam1", "R_guess",
                                       "E", "stereo_threshold", "ransac"])
# counters: before_tracking, after_tracking, after_matching, after_ransac
TracksResult = namedtuple("TracksResult", ["n", "ids", "uv", "counters", "n_total", "next_id"])
TRACKS_COUNTER_NAMES = ("before_tracking", "after_tracking", "after_matching", "after_ransac")


def _model(name):
    return EQUIDISTANT if name == "equidistant" else RADTAN


class ImageProcessor:
    """Reference ImageProcessor (image.py:36-702) on the GPU image operators.
    Messages: stereo_msg with ``cam0_msg`` / ``cam1_msg`` (each ``image`` and
    ``vio_timestamp__``), imu_msg with ``vio_timestamp__`` and
    ``angular_velocity`` (dataset.py:56-57, 101, 169-170)."""

    # image slots: the previous cam0 image and the current pair rotate over three
    def __init__(self, config=None, device=0, ransac_fn=None, fe=None, slot_base=0):
        """``ransac_fn`` (signature of Frontend.two_point_ransac) replaces the
        device call of the two-point RANSAC when config.ransac_enabled.
        ``fe`` / ``slot_base``: a shared device context and the first of this
        stream's three slots in it (MultiImageProcessor's lanes); by default
        the processor makes its own."""
        if config is None:
            config = FrontendConfig()
        elif not isinstance(config, FrontendConfig):
            config = FrontendConfig.from_reference(config)
        self.config = config
        if config.device_tracks and not config.device_pipeline:
            raise ValueError("device_tracks needs device_pipeline")
        if config.device_tracks and fe is None:
            raise ValueError("device_tracks is a switch of MultiImageProcessor's lanes (one lane serves one stream)")
        self.is_first_img = True
        self.next_feature_id = 0
        self.imu_msg_buffer = []
        self.cam0_prev_img_msg = None
        self.cam0_curr_img_msg = None
        self.cam1_curr_img_msg = None
        self.prev_features = [[] for _ in range(config.grid_num)]
        self.curr_features = [[] for _ in range(config.grid_num)]
        self.num_features = defaultdict(int)
        self.cam0_resolution = np.asarray(config.cam0_resolution)
        self.cam0_intrinsics = np.asarray(config.cam0_intrinsics, float)
        self.cam0_distortion_model = config.cam0_distortion_model
        self.cam0_distortion_coeffs = np.asarray(config.cam0_distortion_coeffs, float)
        self.cam1_resolution = np.asarray(config.cam1_resolution)
        self.cam1_intrinsics = np.asarray(config.cam1_intrinsics, float)
        self.cam1_distortion_model = config.cam1_distortion_model
        self.cam1_distortion_coeffs = np.asarray(config.cam1_distortion_coeffs, float)
        self.T_cam0_imu = _inv_T(config.T_imu_cam0)
        self.R_cam0_imu = self.T_cam0_imu[:3, :3]
        self.t_cam0_imu = self.T_cam0_imu[:3, 3]
        self.T_cam1_imu = _inv_T(config.T_imu_cam1)
        self.R_cam1_imu = self.T_cam1_imu[:3, :3]
        self.t_cam1_imu = self.T_cam1_imu[:3, 3]
        W, H = int(self.cam0_resolution[0]), int(self.cam0_resolution[1])
        self._equalize = _equalize_of(config, W, H)   # None: the uploads stay as they are
        self.fe = fe if fe is not None else Frontend(W, H, nslot=3, max_level=config.pyramid_levels,
                                                     max_points=1 << 16, device=device)
        self._slot_prev, self._slot_c0, self._slot_c1 = slot_base, slot_base + 1, slot_base + 2
        self.lk_kw = dict(win=config.patch_size, max_level=config.pyramid_levels,
                          max_iter=config.max_iteration, eps=config.track_precision)
        self.ransac_fn = ransac_fn   # None: self.fe.two_point_ransac
        self.ransac_n_hyp = ransac_hypotheses(config.ransac_success_probability)
        self.ransac_rng = np.random.default_rng(config.ransac_seed)   # advanced once per tracked frame

    # ---- callbacks (image.py:95-147) ----
    def stareo_callback(self, stereo_msg):
        return self._drive(self._frame_steps(stereo_msg))

    stereo_callback = stareo_callback

    def _end_frame(self):
        self.cam0_prev_img_msg = self.cam0_curr_img_msg
        self.prev_features = self.curr_features
        # the current cam0 slot becomes the previous one (its pyramid stays on the device)
        self._slot_prev, self._slot_c0 = self._slot_c0, self._slot_prev
        self.curr_features = [[] for _ in range(self.config.grid_num)]

    def imu_callback(self, msg):
        self.imu_msg_buffer.append(msg)

    def create_image_pyramids(self):
        """image.py:149-164 -- here the device builds the pyramids (and the
        Scharr derivatives LK needs) once per image."""
        return self._drive(self._upload_steps())

    # ---- detection / tracking (image.py:166-404) ----
    def _grid_code(self, pt, gh, gw):
        return int(pt[1] / gh) * self.config.grid_col + int(pt[0] / gw)

    def _assign_new(self, cam0_points, responses, cam1_points, inliers):
        gh, gw = self.get_grid_size(self.cam0_curr_img_msg.image)
        grid_new = [[] for _ in range(self.config.grid_num)]
        for i, ok in enumerate(inliers):
            if not ok:
                continue
            f = FeatureMetaData()
            f.response = responses[i]
            f.cam0_point = cam0_points[i]
            f.cam1_point = cam1_points[i]
            grid_new[self._grid_code(cam0_points[i], gh, gw)].append(f)
        for i, feats in enumerate(grid_new):
            for f in sorted(feats, key=lambda x: x.response, reverse=True)[:self.config.grid_min_feature_num]:
                self.curr_features[i].append(f)
                f.id = self.next_feature_id
                f.lifetime = 1
                self.next_feature_id += 1

    def initialize_first_frame(self):
        """image.py:166-217."""
        return self._drive(self._first_frame_steps())

    def track_features(self):
        """image.py:219-313."""
        return self._drive(self._track_steps())

    def two_point_ransac(self, prev_cam0, curr_cam0, prev_cam1, curr_cam1, cam0_R_p_c, cam1_R_p_c, draws):
        """The step the reference stubs (image.py:292-293), as in msckf_vio:
        the two-point RANSAC of cam0 prev -> curr and of cam1 prev -> curr, both
        in one device call; a feature stays only if it is an inlier of both."""
        return self._drive(self._ransac_steps(prev_cam0, curr_cam0, prev_cam1, curr_cam1, cam0_R_p_c, cam1_R_p_c,
                                              draws))

    def _ransac_steps(self, prev_cam0, curr_cam0, prev_cam1, curr_cam1, cam0_R_p_c, cam1_R_p_c, draws):
        sets = [(prev_cam0, curr_cam0, cam0_R_p_c, self.cam0_intrinsics, _model(self.cam0_distortion_model),
                 self.cam0_distortion_coeffs),
                (prev_cam1, curr_cam1, cam1_R_p_c, self.cam1_intrinsics, _model(self.cam1_distortion_model),
                 self.cam1_distortion_coeffs)]
        (in0, _), (in1, _) = yield ("ransac", sets, self.config.ransac_threshold, self.ransac_n_hyp, draws)
        return np.logical_and(in0, in1)

    def add_new_features(self):
        """image.py:317-390."""
        return self._drive(self._add_new_steps())

    def prune_features(self):
        """image.py:392-404."""
        for i, feats in enumerate(self.curr_features):
            if len(feats) <= self.config.grid_max_feature_num:
                continue
            self.curr_features[i] = sorted(feats, key=lambda x: x.lifetime,
                                           reverse=True)[:self.config.grid_max_feature_num]

    def publish(self):
        """image.py:406-438."""
        return self._drive(self._publish_steps())

    # ---- geometry helpers (image.py:440-702) ----
    def integrate_imu_data(self):
        """image.py:440-487."""
        begin = next((i for i, m in enumerate(self.imu_msg_buffer)
                      if m.vio_timestamp__ >= self.cam0_prev_img_msg.vio_timestamp__ - 0.01), None)
        end = next((i for i, m in enumerate(self.imu_msg_buffer)
                    if m.vio_timestamp__ >= self.cam0_curr_img_msg.vio_timestamp__ - 0.004), None)
        if begin is None or end is None:
            return np.identity(3), np.identity(3)
        mean = np.zeros(3)
        for i in range(begin, end):
            mean += self.imu_msg_buffer[i].angular_velocity
        if end > begin:
            mean /= (end - begin)
        cam0_w = self.R_cam0_imu.T @ mean
        cam1_w = self.R_cam1_imu.T @ mean
        dt = self.cam0_curr_img_msg.vio_timestamp__ - self.cam0_prev_img_msg.vio_timestamp__
        R0 = _rodrigues(cam0_w * dt).T
        R1 = _rodrigues(cam1_w * dt).T
        self.imu_msg_buffer = self.imu_msg_buffer[end:]
        return R0, R1

    def get_grid_size(self, img):
        """image.py:513-519."""
        return (int(np.ceil(img.shape[0] / self.config.grid_row)),
                int(np.ceil(img.shape[1] / self.config.grid_col)))

    def predict_feature_tracking(self, input_pts, R_p_c, intrinsics):
        """image.py:521-552."""
        if len(input_pts) == 0:
            return np.zeros((0, 2), np.float32)
        Hm = self._homography(R_p_c, intrinsics)
        p = np.concatenate([np.asarray(input_pts, float).reshape(-1, 2), np.ones((len(input_pts), 1))], 1)
        q = p @ Hm.T
        return (q[:, :2] / q[:, 2:3]).astype(np.float32)

    @staticmethod
    def _homography(R_p_c, intrinsics):
        """K R K^-1 of predict_feature_tracking (image.py:535-541)."""
        K = np.array([[intrinsics[0], 0.0, intrinsics[2]], [0.0, intrinsics[1], intrinsics[3]], [0.0, 0.0, 1.0]])
        return K @ R_p_c @ np.linalg.inv(K)

    def _stereo_extrinsics(self):
        """(R_cam0_cam1, E) of stereo_match (image.py:561, 611-614)."""
        R_cam0_cam1 = self.R_cam1_imu.T @ self.R_cam0_imu
        t_cam0_cam1 = self.R_cam1_imu.T @ (self.t_cam0_imu - self.t_cam1_imu)
        return R_cam0_cam1, _skew(t_cam0_cam1) @ R_cam0_cam1

    def stereo_match(self, cam0_points):
        """image.py:554-638: project into cam1 through the extrinsics, LK
        cam0 -> cam1 and back, and the vertical-disparity, round-trip and
        epipolar tests."""
        return self._drive(self._match_steps(cam0_points))

    def _match_steps(self, cam0_points):
        """The stereo match of the tracked and of the new features: one request
        with config.device_pipeline, otherwise composed on the spot from six
        single calls (no request: the generator ends without yielding)."""
        if self.config.device_pipeline:
            return (yield from self._stereo_match_steps(cam0_points))
        return self._stereo_match_composed(cam0_points)

    def _stereo_match_composed(self, cam0_points):
        cam0_points = np.asarray(cam0_points, float).reshape(-1, 2)
        if len(cam0_points) == 0:
            return [], []
        R_cam0_cam1, E = self._stereo_extrinsics()
        und = self.undistort_points(cam0_points, self.cam0_intrinsics, self.cam0_distortion_model,
                                    self.cam0_distortion_coeffs, R_cam0_cam1)
        cam1_points = self.distort_points(und, self.cam1_intrinsics, self.cam1_distortion_model,
                                          self.cam1_distortion_coeffs)
        cam1_copy = cam1_points.copy()
        c0 = cam0_points.astype(np.float32)
        c1, inliers = self.fe.lk(self._slot_c0, self._slot_c1, c0, cam1_points.astype(np.float32), **self.lk_kw)
        c0_back, _ = self.fe.lk(self._slot_c1, self._slot_c0, c1, c0.copy(), **self.lk_kw)
        err = np.linalg.norm(c0 - c0_back, axis=1)
        disparity = np.abs(cam1_copy[:, 1] - c1[:, 1])
        inliers = np.logical_and.reduce([inliers.reshape(-1).astype(bool), err < 3, disparity < 20])
        img1 = self.cam1_curr_img_msg.image
        for i, p in enumerate(c1):
            if not inliers[i]:
                continue
            if p[0] < 0 or p[0] > img1.shape[1] - 1 or p[1] < 0 or p[1] > img1.shape[0] - 1:
                inliers[i] = False
        u0 = self.undistort_points(c0, self.cam0_intrinsics, self.cam0_distortion_model, self.cam0_distortion_coeffs)
        u1 = self.undistort_points(c1, self.cam1_intrinsics, self.cam1_distortion_model, self.cam1_distortion_coeffs)
        norm_pixel_unit = 4.0 / (self.cam0_intrinsics[0] + self.cam0_intrinsics[1] +
                                 self.cam1_intrinsics[0] + self.cam1_intrinsics[1])
        for i in range(len(u0)):
            if not inliers[i]:
                continue
            pt0 = np.array([u0[i][0], u0[i][1], 1.0])
            pt1 = np.array([u1[i][0], u1[i][1], 1.0])
            line = E @ pt0
            error = abs((pt1 * line)[0]) / np.linalg.norm(line[:2])
            if error > self.config.stereo_threshold * norm_pixel_unit:
                inliers[i] = False
        return [tuple(p) for p in c1], list(inliers)

    # ---- the frame as generators of device requests ----
    # The frame logic is written once, as generators that yield a request wherever a
    # device call is due and receive its result (as MSCKF._frame_steps does for the
    # filter).  The public methods above drive them with the single calls (_serve);
    # MultiImageProcessor drives many lanes' _frame_steps and serves each kind for all
    # waiting lanes with one set call.  config.device_pipeline is consulted in two places:
    # _match_steps (one stereo_match request, or six single calls composed on the spot)
    # and _add_new_steps (a fast_grid request, or a fast request and the host sieve).
    # Requests:
    #   ("upload", [(slot, image), ...][, (mode, clip_limit, tiles)])        -> None  (the third item
    #                                                  only with config.equalize: Frontend.upload's)
    #   ("fast", slot, threshold[, mask])                                    -> Frontend.fast
    #   ("lk", slot_prev, slot_next, prev_pts, next_pts)                     -> Frontend.lk
    #   ("stereo_match", slot0, slot1, pts, cam0, cam1, R_guess, E, thr)     -> Frontend.stereo_match
    #   ("ransac", sets, inlier_error, n_hyp, draws)                         -> Frontend.two_point_ransac
    #   ("fast_grid", slot, threshold, occupied, grid_row, grid_col, k)      -> Frontend.fast_grid
    #   ("undistort", [(pts, intrinsics, model, coeffs, R, new_intrinsics)]) -> [points per set]
    # The LK parameters (self.lk_kw) are not part of a request: they are per processor, and
    # lanes of one MultiImageProcessor agree on them.
    def _drive(self, gen):
        try:
            req = next(gen)
            while True:
                req = gen.send(self._serve(req))
        except StopIteration as e:
            return e.value

    def _serve(self, req):
        kind = req[0]
        if kind == "upload":
            for slot, image in req[1]:
                self.fe.upload(slot, image, *req[2:])
            return None
        if kind == "fast":
            return self.fe.fast(*req[1:])
        if kind == "lk":
            return self.fe.lk(*req[1:], **self.lk_kw)
        if kind == "stereo_match":
            return self.fe.stereo_match(*req[1:], **self.lk_kw)
        if kind == "ransac":
            fn = self.ransac_fn if self.ransac_fn is not None else self.fe.two_point_ransac
            return fn(*req[1:])
        if kind == "fast_grid":
            return self.fe.fast_grid(*req[1:])
        if kind == "undistort":
            return [self.fe.undistort(*a) if len(a[0]) else np.zeros((0, 2)) for a in req[1]]
        raise ValueError("unknown device request %r" % (kind,))

    def _frame_steps(self, stereo_msg):
        """stareo_callback; returns the published message."""
        self.cam0_curr_img_msg = stereo_msg.cam0_msg
        self.cam1_curr_img_msg = stereo_msg.cam1_msg
        yield from self._upload_steps()
        if self.is_first_img:
            yield from self._first_frame_steps()
            self.is_first_img = False
        else:
            yield from self._track_steps()
            yield from self._add_new_steps()
            self.prune_features()
        try:
            return (yield from self._publish_steps())
        finally:
            self._end_frame()

    def _upload_steps(self):
        pairs = [(self._slot_c0, self.cam0_curr_img_msg.image), (self._slot_c1, self.cam1_curr_img_msg.image)]
        if self._equalize is None:
            yield ("upload", pairs)
        else:
            yield ("upload", pairs, self._equalize)

    def _first_frame_steps(self):
        xy, resp = yield ("fast", self._slot_c0, self.config.fast_threshold)
        yield from self._collect_new_steps([tuple(p) for p in xy], list(resp))

    def _collect_new_steps(self, cam0_points, responses):
        cam1_points, inliers = yield from self._match_steps(cam0_points)
        self._assign_new(cam0_points, responses, cam1_points, inliers)

    def _track_steps(self):
        """track_features (image.py:219-313) around its requests."""
        img = self.cam0_curr_img_msg.image
        gh, gw = self.get_grid_size(img)
        cam0_R_p_c, cam1_R_p_c = self.integrate_imu_data()
        if self.config.ransac_enabled:   # once per tracked frame, whatever the frame holds: a replay repeats
            draws = self.ransac_rng.integers(0, 1 << 32, size=(2, self.ransac_n_hyp, 2), dtype=np.uint32)
        prev_ids, prev_lifetime, prev_cam0_points, prev_cam1_points = [], [], [], []
        for f in chain.from_iterable(self.prev_features):
            prev_ids.append(f.id)
            prev_lifetime.append(f.lifetime)
            prev_cam0_points.append(f.cam0_point)
            prev_cam1_points.append(f.cam1_point)
        prev_cam0_points = np.array(prev_cam0_points, dtype=np.float32).reshape(-1, 2)
        self.num_features["before_tracking"] = len(prev_cam0_points)
        if len(prev_cam0_points) == 0:
            return
        curr_cam0_points = self.predict_feature_tracking(prev_cam0_points, cam0_R_p_c, self.cam0_intrinsics)
        curr_cam0_points, track_inliers = yield ("lk", self._slot_prev, self._slot_c0, prev_cam0_points,
                                                 curr_cam0_points)
        track_inliers = track_inliers.astype(bool)
        for i, p in enumerate(curr_cam0_points):
            if not track_inliers[i]:
                continue
            if p[0] < 0 or p[0] > img.shape[1] - 1 or p[1] < 0 or p[1] > img.shape[0] - 1:
                track_inliers[i] = False
        prev_tracked_ids = _select(prev_ids, track_inliers)
        prev_tracked_lifetime = _select(prev_lifetime, track_inliers)
        curr_tracked_cam0_points = _select(curr_cam0_points, track_inliers)
        self.num_features["after_tracking"] = len(curr_tracked_cam0_points)
        curr_cam1_points, match_inliers = yield from self._match_steps(curr_tracked_cam0_points)
        prev_matched_ids = _select(prev_tracked_ids, match_inliers)
        prev_matched_lifetime = _select(prev_tracked_lifetime, match_inliers)
        curr_matched_cam0_points = _select(curr_tracked_cam0_points, match_inliers)
        curr_matched_cam1_points = _select(curr_cam1_points, match_inliers)
        self.num_features["after_matching"] = len(curr_matched_cam0_points)
        ransac_inliers = None
        if self.config.ransac_enabled:
            ransac_inliers = yield from self._ransac_steps(
                _select(_select(prev_cam0_points, track_inliers), match_inliers), curr_matched_cam0_points,
                _select(_select(prev_cam1_points, track_inliers), match_inliers), curr_matched_cam1_points,
                cam0_R_p_c, cam1_R_p_c, draws)
        after_ransac = 0
        for i in range(len(curr_matched_cam0_points)):   # RANSAC stub: all inliers (image.py:292-293)
            if ransac_inliers is not None and not ransac_inliers[i]:
                continue
            f = FeatureMetaData()
            f.id = prev_matched_ids[i]
            f.lifetime = prev_matched_lifetime[i] + 1
            f.cam0_point = curr_matched_cam0_points[i]
            f.cam1_point = curr_matched_cam1_points[i]
            self.curr_features[self._grid_code(curr_matched_cam0_points[i], gh, gw)].append(f)
            after_ransac += 1
        self.num_features["after_ransac"] = after_ransac

    def _stereo_args(self):
        """(cam0, cam1, R_guess, E, stereo_threshold) of mfe_stereo_match and
        mfe_tracks_step.  The equidistant quirk of undistort_points (no
        rectification) is kept by passing the identity as the rotation of the
        initial guess."""
        R_cam0_cam1, E = self._stereo_extrinsics()
        model0 = _model(self.cam0_distortion_model)
        return ((self.cam0_intrinsics, model0, self.cam0_distortion_coeffs),
                (self.cam1_intrinsics, _model(self.cam1_distortion_model), self.cam1_distortion_coeffs),
                np.identity(3) if model0 == EQUIDISTANT else R_cam0_cam1, E, self.config.stereo_threshold)

    def _stereo_match_steps(self, cam0_points):
        """stereo_match as the one call mfe_stereo_match."""
        cam0_points = np.asarray(cam0_points, float).reshape(-1, 2)
        if len(cam0_points) == 0:
            return [], []
        c1, inliers, _ = yield ("stereo_match", self._slot_c0, self._slot_c1, cam0_points, *self._stereo_args())
        return [tuple(p) for p in c1], list(inliers.astype(bool))

    def _tracks_lane(self, lane):
        """This lane's arguments of Frontend.tracks_step for the frame at hand:
        what _track_steps does on the host before its first request (the IMU
        rotations, the RANSAC draws, the homography of predict_feature_tracking)
        and the stereo arguments of _stereo_match_steps."""
        R0, R1 = self.integrate_imu_data()
        ransac = None
        if self.config.ransac_enabled:   # once per tracked frame, as in _track_steps
            ransac = (R0, R1, self.ransac_rng.integers(0, 1 << 32, size=(2, self.ransac_n_hyp, 2), dtype=np.uint32))
        return TracksLane(lane, self._slot_prev, self._slot_c0, self._slot_c1,
                          self._homography(R0, self.cam0_intrinsics), *self._stereo_args(), ransac)

    def _add_new_steps(self):
        """add_new_features (image.py:317-390).  With config.device_pipeline the
        mask, the detection and the per-cell sieve are the one call
        mfe_fast_grid: a cell comes back response-descending with raster ties
        where the host sieve leaves a cell of at most grid_max_feature_num in
        raster order; _assign_new sorts every cell by response with a stable
        sort, so the features and their ids are the same."""
        cfg = self.config
        if cfg.device_pipeline:
            occ = np.array([f.cam0_point for f in chain.from_iterable(self.curr_features)], np.float32).reshape(-1, 2)
            xy, resp, _, _ = yield ("fast_grid", self._slot_c0, cfg.fast_threshold, occ, cfg.grid_row, cfg.grid_col,
                                    cfg.grid_max_feature_num)
            return (yield from self._collect_new_steps([tuple(p) for p in xy], list(resp)))
        img = self.cam0_curr_img_msg.image
        gh, gw = self.get_grid_size(img)
        mask = np.ones(img.shape[:2], dtype=np.uint8)
        for f in chain.from_iterable(self.curr_features):
            x, y = map(int, f.cam0_point)
            mask[y - 3:y + 4, x - 3:x + 4] = 0   # the reference's slice, negative starts included
        xy, resp = yield ("fast", self._slot_c0, cfg.fast_threshold, mask)
        sieve = [[] for _ in range(cfg.grid_num)]
        for p, r in zip(xy, resp):
            sieve[self._grid_code(p, gh, gw)].append((tuple(p), r))
        picked = []
        for feats in sieve:
            if len(feats) > cfg.grid_max_feature_num:
                feats = sorted(feats, key=lambda x: x[1], reverse=True)[:cfg.grid_max_feature_num]
            picked.extend(feats)
        yield from self._collect_new_steps([p for p, _ in picked], [r for _, r in picked])

    def _publish_steps(self):
        """publish: both cameras' points undistorted by one request."""
        ids, c0, c1 = [], [], []
        for f in chain.from_iterable(self.curr_features):
            ids.append(f.id)
            c0.append(f.cam0_point)
            c1.append(f.cam1_point)
        u0, u1 = yield ("undistort", [
            self._undistort_args(c0, self.cam0_intrinsics, self.cam0_distortion_model, self.cam0_distortion_coeffs),
            self._undistort_args(c1, self.cam1_intrinsics, self.cam1_distortion_model, self.cam1_distortion_coeffs)])
        feats = [FeatureMeasurement(ids[i], u0[i][0], u0[i][1], u1[i][0], u1[i][1]) for i in range(len(ids))]
        return FeatureMsg(self.cam0_curr_img_msg.vio_timestamp__, feats)

    def _undistort_args(self, pts_in, intrinsics, distortion_model, distortion_coeffs):
        """The arguments undistort_points (below) gives Frontend.undistort
        without a rectification, the equidistant quirk included."""
        model = _model(distortion_model)
        R = np.identity(3)   # K_new of [1 1 0 0] in the R slot, or no rectification: the identity either way
        return (pts_in, intrinsics, model, distortion_coeffs, R, np.array([1.0, 1.0, 0.0, 0.0]))

    def undistort_points(self, pts_in, intrinsics, distortion_model, distortion_coeffs,
                         rectification_matrix=np.identity(3), new_intrinsics=np.array([1, 1, 0, 0])):
        """image.py:640-674 (cv2.undistortPoints / cv2.fisheye.undistortPoints).
        Quirk kept: for 'equidistant' the reference passes its rectification
        matrix in cv2.fisheye.undistortPoints' output slot and K_new in its R
        slot (image.py:669-670, positional arguments), so cv2 rotates by K_new
        and returns normalised points; the rectification is never applied."""
        if len(pts_in) == 0:
            return np.zeros((0, 2))
        model = _model(distortion_model)
        if model == EQUIDISTANT:
            n = np.asarray(new_intrinsics, float)
            K_new = np.array([[n[0], 0.0, n[2]], [0.0, n[1], n[3]], [0.0, 0.0, 1.0]])
            return self.fe.undistort(pts_in, intrinsics, model, distortion_coeffs, K_new, np.array([1.0, 1.0, 0.0, 0.0]))
        return self.fe.undistort(pts_in, intrinsics, model, distortion_coeffs, rectification_matrix, new_intrinsics)

    def distort_points(self, pts_in, intrinsics, distortion_model, distortion_coeffs):
        """image.py:676-702 (cv2.projectPoints / cv2.fisheye.distortPoints)."""
        if len(pts_in) == 0:
            return np.zeros((0, 2))
        return self.fe.distort(pts_in, intrinsics, _model(distortion_model), distortion_coeffs)


# pipeline order of a frame's device requests: a lane waiting at an earlier stage is served first
_REQUEST_ORDER = {"upload": 0, "fast": 1, "lk": 2, "stereo_match": 3, "ransac": 4, "fast_grid": 5, "undistort": 6}
# what the set calls share between lanes (msckf_lanes.h): the image size and these fields
_SHARED_FIELDS = ("pyramid_levels", "patch_size", "max_iteration", "track_precision", "fast_threshold", "grid_row",
                  "grid_col")


class MultiImageProcessor:
    """``n`` stereo streams (lanes) on one device context: the image-side
    counterpart of ``scheduler.MultiMSCKF``.  Every lane is an
    ``ImageProcessor(device_pipeline=True)`` with its own bookkeeping
    (features, ids, IMU buffer, RANSAC generator) and three slots of the
    shared context; ``stereo_callbacks`` advances the lanes' frames in lock
    step and serves each kind of device request for all waiting lanes with ONE
    call of include/msckf_lanes.h:

      upload       -> mfe_upload_many          lk        -> mfe_lk_sets
      stereo_match -> mfe_stereo_match_sets    ransac    -> mfe_two_point_ransac
      fast_grid    -> mfe_fast_grid_sets       undistort -> mfe_undistort_sets

    ``fast`` (a stream's first frame, no per-cell cap) is served per lane with
    the single call.  Lanes whose frames diverge (one starts late, one runs
    RANSAC) wait at the earliest stage of ``_REQUEST_ORDER`` first, so requests
    of one kind merge again.  The set calls compute every set as the single
    call does, so each lane publishes what an ImageProcessor alone publishes.

    Lanes may differ in calibration, grid_min / grid_max_feature_num,
    stereo_threshold and the RANSAC switch, threshold and seed; they must
    agree on the resolution and the fields of ``_SHARED_FIELDS``.  Each lane
    has its own ``equalize`` mode and clip limit (msckf_equalize.h: the upload
    becomes mfe_upload_many_eq as soon as one lane of the step equalises, still
    one call); the lanes agree on ``clahe_tiles``.

    With ``device_tracks`` in every lane's config the per-feature bookkeeping
    leaves the host: the lanes' track tables live on the device
    (include/msckf_tracks.h) and a step is ``mfe_upload_many`` plus ONE
    ``mfe_tracks_step`` for all tracking lanes; a lane's first frame runs as
    above and enters its table through ``mfe_tracks_put``.  The lanes then
    also agree on grid_min / grid_max_feature_num and, among the RANSAC lanes,
    on the threshold and success probability.  ``tracks(i)`` reads a table.

    With ``track_motion`` (all lanes, needs ``device_tracks``) every tracked
    frame also leaves the lane's motion record on the device
    (include/msckf_standstill.h): the ``track_motion_quantile`` of the squared
    pixel displacement of the tracks that survived the frame.
    ``track_motion(i)`` reads it; an array message carries it as ``motion``,
    a ``TrackMessage`` names the lane whose record the filter reads in place."""

    def __init__(self, n, config=None, lane_configs=None, device=0):
        if lane_configs is None:
            if config is None:
                config = FrontendConfig()
            elif not isinstance(config, FrontendConfig):
                config = FrontendConfig.from_reference(config)
            cfgs = [FrontendConfig(**{**vars(config), "device_pipeline": True}) for _ in range(n)]
        else:
            cfgs = [c if isinstance(c, FrontendConfig) else FrontendConfig.from_reference(c) for c in lane_configs]
        if len(cfgs) != n or n < 1:
            raise ValueError("%d lane configs for %d lanes" % (len(cfgs), n))
        if 3 * n > _lib.MAX_SLOTS:
            raise ValueError("%d lanes need %d slots, a context holds %d" % (n, 3 * n, _lib.MAX_SLOTS))
        res = lambda c: (tuple(int(v) for v in c.cam0_resolution), tuple(int(v) for v in c.cam1_resolution))
        for i, c in enumerate(cfgs):
            if not c.device_pipeline:
                raise ValueError("lane %d: device_pipeline is off" % i)
            if res(c) != res(cfgs[0]) or res(c)[0] != res(c)[1]:
                raise ValueError("lane %d: resolution %s differs from lane 0's %s" % (i, res(c), res(cfgs[0])))
            for f in _SHARED_FIELDS:
                if getattr(c, f) != getattr(cfgs[0], f):
                    raise ValueError("lane %d: %s = %r differs from lane 0's %r"
                                     % (i, f, getattr(c, f), getattr(cfgs[0], f)))
            # mfe_upload_many_eq has one tile grid per call
            _equalize_of(c, *res(c)[0])
            if _check_tiles(c.clahe_tiles, *res(c)[0]) != _check_tiles(cfgs[0].clahe_tiles, *res(c)[0]):
                raise ValueError("lane %d: clahe_tiles = %r differs from lane 0's %r"
                                 % (i, c.clahe_tiles, cfgs[0].clahe_tiles))
        # device_tracks: all lanes or none, and what mfe_tracks_step shares between lanes
        self.device_tracks = bool(cfgs[0].device_tracks)
        ransac = [i for i, c in enumerate(cfgs) if c.ransac_enabled]
        for i, c in enumerate(cfgs):
            if bool(c.device_tracks) != self.device_tracks:
                raise ValueError("lane %d: device_tracks = %r differs from lane 0's %r"
                                 % (i, c.device_tracks, cfgs[0].device_tracks))
            if not self.device_tracks:
                if c.track_motion:
                    raise ValueError("lane %d: track_motion needs device_tracks" % i)
                continue
            # the motion statistic is a switch of the context (msckf_standstill.h)
            shared = [("grid_min_feature_num", 0), ("grid_max_feature_num", 0), ("track_motion", 0),
                      ("track_motion_quantile", 0)]
            if c.ransac_enabled:   # the RANSAC lanes among themselves
                shared += [("ransac_threshold", ransac[0]), ("ransac_success_probability", ransac[0])]
            for f, j in shared:
                if getattr(c, f) != getattr(cfgs[j], f):
                    raise ValueError("lane %d: %s = %r differs from lane %d's %r (device_tracks)"
                                     % (i, f, getattr(c, f), j, getattr(cfgs[j], f)))
        (W, H), _ = res(cfgs[0])
        # a call's point limit covers all lanes: a first frame matches every keypoint it detects
        self.fe = Frontend(W, H, nslot=3 * n, max_level=cfgs[0].pyramid_levels, max_points=n << 16, device=device)
        self.lanes = [ImageProcessor(c, device=device, fe=self.fe, slot_base=3 * i) for i, c in enumerate(cfgs)]
        self.lk_kw = self.lanes[0].lk_kw
        self.launches = defaultdict(int)   # device calls per request kind
        if self.device_tracks:   # the smallest tables the grid allows
            c = cfgs[0]
            self.fe.tracks_create(n, c.grid_num * (c.grid_min_feature_num + c.grid_max_feature_num), c.grid_row,
                                  c.grid_col, c.grid_min_feature_num, c.grid_max_feature_num)
            self._tracks_ransac = ((cfgs[ransac[0]].ransac_threshold, self.lanes[ransac[0]].ransac_n_hyp)
                                   if ransac else (0.0, 0))
        self.track_motion_on = bool(self.device_tracks and cfgs[0].track_motion)
        if self.track_motion_on:
            try:
                self.fe.tracks_motion_enable(True, cfgs[0].track_motion_quantile)
            except BaseException:
                self.fe.close()
                raise

    def __len__(self):
        return len(self.lanes)

    def close(self):
        self.fe.close()

    def imu_callback(self, i, msg):
        self.lanes[i].imu_callback(msg)

    def stereo_callbacks(self, msgs, arrays=False, handoff=False):
        """``msgs``: {lane index: stereo_msg}.  Returns {lane index:
        FeatureMsg}, as the lanes' own stareo_callback would.  ``arrays``:
        array messages (msckf.FeatureArrays) instead -- with the tracks on the
        device straight from the step's ids / uv, no tuple per feature;
        otherwise converted once.  ``handoff`` (needs ``device_tracks``): the
        messages stay on the device (msckf_handoff.h) and every lane returns
        a ``msckf.TrackMessage`` naming its place; a first-frame lane
        publishes on the host as always and writes its message from there."""
        if handoff and not self.device_tracks:
            raise ValueError("handoff=True needs device_tracks: the message is handed over from the device tables")
        if self.device_tracks:
            return self._tracks_callbacks(msgs, arrays, handoff)
        gens, out = {}, {}
        for i, m in msgs.items():
            gens[i] = self.lanes[i]._frame_steps(m)
        self._pump(gens, out)
        return {i: _as_arrays(m) for i, m in out.items()} if arrays else out

    def _pump(self, gens, out):
        """Runs the lanes' generators to their ends, each kind of request served
        for all lanes waiting at it with one call; out[lane] = its generator's value."""
        pending = {}
        for i, gen in gens.items():
            self._advance(i, gen, None, pending, out, first=True)
        while pending:
            kind = min((r[0] for r in pending.values()), key=lambda k: _REQUEST_ORDER[k])
            group = [i for i, r in pending.items() if r[0] == kind]
            if kind == "ransac":       # inlier error and hypothesis count are per call
                group = [i for i in group if pending[i][2:4] == pending[group[0]][2:4]]
            elif kind == "fast_grid":  # and so is k (grid_max_feature_num)
                group = [i for i in group if pending[i][6] == pending[group[0]][6]]
            results = self._serve(kind, [pending[i] for i in group])
            for i, res in zip(group, results):
                del pending[i]
                self._advance(i, gens[i], res, pending, out)

    def tracks(self, i):
        """Lane i's track table on the device (device_tracks): (ids, lifetimes,
        cam0, cam1, next_id), rows in publish order."""
        return self.fe.tracks_get(i)

    def track_motion(self, i):
        """Lane i's motion record (``FrontendConfig.track_motion``): (valid, n,
        d2) -- d2 the configured quantile of the squared pixel displacement of
        the n tracks that survived the last frame's tracking; synchronises."""
        if not self.track_motion_on:
            raise ValueError("track_motion needs FrontendConfig(device_tracks=True, track_motion=True)")
        return self.fe.tracks_motion_get(i)

    def _tracks_callbacks(self, msgs, arrays=False, handoff=False):
        """stereo_callbacks with the tracks on the device: one upload for all
        lanes, the first-frame lanes on their generators (then tracks_put, and
        with ``handoff`` tracks_msg_put), and ONE tracks_step for all tracking
        lanes (with ``handoff`` in its to_message form)."""
        lanes, out = self.lanes, {}
        for i, m in msgs.items():
            lanes[i].cam0_curr_img_msg, lanes[i].cam1_curr_img_msg = m.cam0_msg, m.cam1_msg
        self._serve("upload", [next(lanes[i]._upload_steps()) for i in msgs])
        first = [i for i in msgs if lanes[i].is_first_img]
        if first:
            self._pump({i: self._first_frame_tracks_steps(i, handoff) for i in first}, out)
        tracking = [i for i in msgs if i not in first]
        if tracking:
            self.launches["tracks_step"] += 1
            inlier_error, n_hyp = self._tracks_ransac
            kw = dict(self.lk_kw, to_message=True) if handoff else self.lk_kw   # the default call stays as it was
            res = self.fe.tracks_step([lanes[i]._tracks_lane(i) for i in tracking], lanes[0].config.fast_threshold,
                                      inlier_error=inlier_error, n_hyp=n_hyp, **kw)
            for i, r in zip(tracking, res):
                ip = lanes[i]
                ip.num_features.update(zip(TRACKS_COUNTER_NAMES, (int(v) for v in r.counters)))
                ip.next_feature_id = r.next_id
                if handoff:
                    out[i] = TrackMessage(ip.cam0_curr_img_msg.vio_timestamp__, self.fe, i, r.n)
                elif arrays:
                    motion = None
                    if self.track_motion_on:   # the record the step just wrote, for the host's cue
                        self.launches["tracks_motion_get"] += 1
                        _, mn, md2 = self.fe.tracks_motion_get(i)
                        motion = (mn, md2)
                    out[i] = FeatureArrays(ip.cam0_curr_img_msg.vio_timestamp__, np.asarray(r.ids, np.int64),
                                           np.asarray(r.uv, np.float64).reshape(-1, 4), motion)
                else:
                    out[i] = FeatureMsg(ip.cam0_curr_img_msg.vio_timestamp__,
                                        [FeatureMeasurement(k, *u) for k, u in zip(r.ids.tolist(), r.uv.tolist())])
                ip._end_frame()
        if arrays and not handoff:   # the first-frame lanes' messages come from the existing path
            out = {i: _as_arrays(m) for i, m in out.items()}
        return out

    def _first_frame_tracks_steps(self, i, handoff=False):
        """A lane's first frame (the images are uploaded) on the existing path;
        its features then enter the lane's device table -- and with
        ``handoff`` what it published becomes the lane's message."""
        ip = self.lanes[i]
        yield from ip._first_frame_steps()
        ip.is_first_img = False
        try:
            msg = yield from ip._publish_steps()
            feats = list(chain.from_iterable(ip.curr_features))
            self.launches["tracks_put"] += 1
            self.fe.tracks_put(i, [f.id for f in feats], [f.lifetime for f in feats], [f.cam0_point for f in feats],
                               [f.cam1_point for f in feats], ip.next_feature_id)
            if handoff:
                arr = _as_arrays(msg)
                self.launches["tracks_msg_put"] += 1
                self.fe.tracks_msg_put(i, arr.ids, arr.uv)
                return TrackMessage(arr.timestamp, self.fe, i, len(arr.ids))
            return msg
        finally:
            ip._end_frame()

    def _advance(self, i, gen, value, pending, out, first=False):
        try:
            pending[i] = next(gen) if first else gen.send(value)
        except StopIteration as e:
            out[i] = e.value

    def _serve(self, kind, reqs):
        fe = self.fe
        if kind == "fast":
            self.launches[kind] += len(reqs)
            return [fe.fast(*r[1:]) for r in reqs]
        self.launches[kind] += 1
        if kind == "upload":
            pairs = [p for r in reqs for p in r[1]]
            eq = ()
            if any(len(r) > 2 for r in reqs):   # some lane equalises: a mode and a clip limit per image
                per = [(r[2] if len(r) > 2 else ("none", 0.0, None), len(r[1])) for r in reqs]
                eq = (([e[0] for e, k in per for _ in range(k)], [e[1] for e, k in per for _ in range(k)],
                       next(e[2] for e, _ in per if e[2] is not None)),)   # the lanes agree on the tiles
            fe.upload_many([s for s, _ in pairs], np.stack([np.asarray(im, np.uint8) for _, im in pairs]), *eq)
            return [None] * len(reqs)
        if kind == "lk":
            return fe.lk_sets([r[1:] for r in reqs], **self.lk_kw)
        if kind == "stereo_match":
            return fe.stereo_match_sets([r[1:] for r in reqs], **self.lk_kw)
        if kind == "ransac":
            res = fe.two_point_ransac([s for r in reqs for s in r[1]], reqs[0][2], reqs[0][3],
                                      np.concatenate([r[4] for r in reqs]))
            return [res[2 * j:2 * j + 2] for j in range(len(reqs))]
        if kind == "fast_grid":
            return fe.fast_grid_sets([(r[1], r[3]) for r in reqs], *reqs[0][2:3], *reqs[0][4:7])
        if kind == "undistort":
            res = fe.undistort_sets([a for r in reqs for a in r[1]])
            return [res[2 * j:2 * j + 2] for j in range(len(reqs))]
        raise ValueError("unknown device request %r" % (kind,))
