"""ctypes binding of libmsckf_hip.so (C-ABI in include/msckf_hip.h).

Fails loudly: if the shared library is missing, or no HIP device is usable,
constructing a context raises -- there is no CPU fallback anywhere in the
product path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

from .config import FilterConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmsckf_hip.so")

IMU_LEN = 42
CAM_LEN = 11
TRIANGULATE = 1

# IMU record field offsets (msckf_hip.h)
I_Q, I_P, I_V, I_BG, I_BA, I_QN, I_PN, I_VN, I_RIC, I_TCI, I_G, I_ALIAS = 0, 4, 7, 10, 13, 16, 20, 23, 26, 35, 38, 41


class MsckfConfigT(C.Structure):
    _fields_ = [
        ("gyro_noise", C.c_double), ("acc_noise", C.c_double),
        ("gyro_bias_noise", C.c_double), ("acc_bias_noise", C.c_double),
        ("observation_noise", C.c_double),
        ("R_cam0_cam1", C.c_double * 9), ("t_cam0_cam1", C.c_double * 3),
        ("huber_epsilon", C.c_double), ("estimation_precision", C.c_double),
        ("initial_damping", C.c_double),
        ("outer_loop_max_iteration", C.c_int32), ("inner_loop_max_iteration", C.c_int32),
    ]


class MsckfError(RuntimeError):
    pass


_lib = None
_lib_lock = threading.Lock()

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)
_U8 = C.POINTER(C.c_uint8)

_SIGS = {
    "msckf_create": (C.c_int, [C.POINTER(MsckfConfigT), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "msckf_destroy": (C.c_int, [_P]),
    "msckf_last_error": (C.c_char_p, []),
    "msckf_scalar_bytes": (C.c_int, [_P]),
    "msckf_device_info": (C.c_int, [_P, _I, C.c_char_p, C.c_int]),
    "msckf_set_state": (C.c_int, [_P, C.c_int, _D, C.c_int, _D, _D]),
    "msckf_get_state": (C.c_int, [_P, C.c_int, _D, _D, _D, _I]),
    "msckf_get_cov_diag": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D]),
    "msckf_propagate": (C.c_int, [_P, C.c_int, C.c_int, _D, _D, _D]),
    "msckf_augment": (C.c_int, [_P, C.c_int]),
    "msckf_triangulate": (C.c_int, [_P, C.c_int, C.c_int, _I, _I, _D, _D, _U8]),
    "msckf_update": (C.c_int, [_P, C.c_int, C.c_int, _I, _I, _D, _D, _D, C.c_int, _U8, _D, _I]),
    "msckf_prune": (C.c_int, [_P, C.c_int, C.c_int, _I]),
    "msckf_propagate_batch": (C.c_int, [_P, C.c_int, _I, _I, _D, _D, _D]),
    "msckf_augment_batch": (C.c_int, [_P, C.c_int, _I]),
    "msckf_prune_batch": (C.c_int, [_P, C.c_int, _I, _I, _I]),
    "msckf_get_states_batch": (C.c_int, [_P, C.c_int, _I, _D, _D, _I]),
    "msckf_get_cov_diag_batch": (C.c_int, [_P, C.c_int, _I, C.c_int, C.c_int, _D]),
    "msckf_readback": (C.c_int, [_P, C.c_int, _I, _D, _D, _I, C.c_int, C.c_int, _D, _U8, _D, _D, _U8, _I]),
    "msckf_batch_triangulate": (C.c_int, [_P]),
    "msckf_batch_load": (C.c_int, [_P, _I, _I, _I, _D, _D, _D]),
    "msckf_batch_update": (C.c_int, [_P, C.c_int, C.c_int]),
    "msckf_batch_results": (C.c_int, [_P, _U8, _D, _D, _U8, _I]),
    "msckf_snapshot": (C.c_int, [_P]),
    "msckf_restore": (C.c_int, [_P]),
    "msckf_sync": (C.c_int, [_P]),
    "msckf_set_profiling": (C.c_int, [_P, C.c_int]),
    "msckf_set_profiling_stage": (C.c_int, [_P, C.c_char_p]),
    "msckf_kernel_times": (C.c_int, [_P, C.c_int, _D, _I, C.c_char_p, C.c_int]),
}

EXPORTED = tuple(_SIGS)

_F = C.POINTER(C.c_float)
# GPU stereo front-end (include/msckf_frontend.h), same library
FRONTEND_SIGS = {
    "mfe_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "mfe_destroy": (C.c_int, [_P]),
    "mfe_last_error": (C.c_char_p, []),
    "mfe_upload": (C.c_int, [_P, C.c_int, _U8]),
    "mfe_fast": (C.c_int, [_P, C.c_int, C.c_int, _U8, C.c_int, _F, _F, _I]),
    "mfe_lk": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _F, _F, _U8, C.c_int, C.c_int, C.c_int, C.c_double]),
    "mfe_undistort": (C.c_int, [_P, C.c_int, _D, _D, _D, C.c_int, _D, _D, _D]),
    "mfe_distort": (C.c_int, [_P, C.c_int, _D, _D, _D, C.c_int, _D]),
}
FRONTEND_EXPORTED = tuple(FRONTEND_SIGS)

_U32 = C.POINTER(C.c_uint32)
# two-point RANSAC of the front-end (include/msckf_ransac.h), same library and context
RANSAC_INFO_LEN = 12
RANSAC_MAX_SET_POINTS = 4096
RANSAC_MAX_HYP = 256
FRONTEND_RANSAC_SIGS = {
    "mfe_two_point_ransac": (C.c_int, [_P, C.c_int, _I, _D, _D, _D, _D, _I, _D, C.c_double, C.c_int, _U32, _U8, _D]),
}
FRONTEND_RANSAC_EXPORTED = tuple(FRONTEND_RANSAC_SIGS)

# stereo matching and grid-selected detection as single device calls
# (include/msckf_pipeline.h), same library and context
GRID_MAX_K = 16
GRID_MAX_CELLS = 1024
FRONTEND_PIPELINE_SIGS = {
    "mfe_stereo_match": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _D, _D, C.c_int, _D, _D, C.c_int, _D, _D, _D,
                                   C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _F, _U8, _U8]),
    "mfe_fast_grid": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _F, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, _I,
                                _I]),
}
FRONTEND_PIPELINE_EXPORTED = tuple(FRONTEND_PIPELINE_SIGS)

# the front-end's calls over many streams' sets (include/msckf_lanes.h), same library and context
MAX_SLOTS = 96
MAX_SETS = 1024
FRONTEND_LANES_SIGS = {
    "mfe_upload_many": (C.c_int, [_P, C.c_int, _I, _U8]),
    "mfe_lk_sets": (C.c_int, [_P, C.c_int, _I, _I, _I, _F, _F, _U8, C.c_int, C.c_int, C.c_int, C.c_double]),
    "mfe_stereo_match_sets": (C.c_int, [_P, C.c_int, _I, _I, _I, _D, _D, _I, _D, _D, _I, _D, _D, _D, _D,
                                        C.c_int, C.c_int, C.c_int, C.c_double, _F, _U8, _U8]),
    "mfe_fast_grid_sets": (C.c_int, [_P, C.c_int, _I, _I, _F, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F,
                                     _I, _I]),
    "mfe_undistort_sets": (C.c_int, [_P, C.c_int, _I, _D, _D, _D, _I, _D, _D, _D]),
}
FRONTEND_LANES_EXPORTED = tuple(FRONTEND_LANES_SIGS)

_I64 = C.POINTER(C.c_int64)
# the feature tracks kept on the device, one call per tracked frame (include/msckf_tracks.h),
# same library and context
TRACKS_COUNTERS = 4
FRONTEND_TRACKS_SIGS = {
    "mfe_tracks_create": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mfe_tracks_put": (C.c_int, [_P, C.c_int, C.c_int, _I64, _I, _F, _F, C.c_int64]),
    "mfe_tracks_get": (C.c_int, [_P, C.c_int, _I, _I64, _I, _F, _F, _I64]),
    "mfe_tracks_step": (C.c_int, [_P, C.c_int, _I, _I, _I, _I, _D, _D, _I, _D, _D, _I, _D, _D, _D, _D, _I, _D, _D,
                                  _U32, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                  C.c_int, _I, _I64, _D, _I, _I, _I64]),
}
TRACKS_EXPORTED = tuple(FRONTEND_TRACKS_SIGS)

_U64 = C.POINTER(C.c_uint64)
# the filter's feature map kept on the device (include/msckf_map.h), same library and context
MAP_LOAD_LOST, MAP_LOAD_PRUNE_TRI, MAP_LOAD_PRUNE_UPDATE = 0, 1, 2
MAP_INFO = 4
MAP_SIGS = {
    "msckf_map_create": (C.c_int, [_P, C.c_int, _D]),
    "msckf_map_clear": (C.c_int, [_P, C.c_int, _I]),
    "msckf_map_put": (C.c_int, [_P, C.c_int, C.c_int, _I64, _U64, _D, _D, _U8]),
    "msckf_map_get": (C.c_int, [_P, C.c_int, _I, _I64, _U64, _D, _D, _U8]),
    "msckf_map_add_lost": (C.c_int, [_P, C.c_int, _I, _I, _I64, _D, _I, _I, _I, _I64, _I]),
    "msckf_map_prune_select": (C.c_int, [_P, C.c_int, _I, _I, _I, _I, _I64, _I]),
    "msckf_map_load": (C.c_int, [_P, C.c_int, C.c_int, _I, _I, _I, _I, _D]),
    "msckf_map_prune_commit": (C.c_int, [_P, C.c_int, _I, _I, _I, _U8, _D]),
}
MAP_EXPORTED = tuple(MAP_SIGS)

# the keyframe choice on the device, fused into the prune select (include/msckf_keyframes.h), same library and
# context; the reference's thresholds (msckf.py:711): rotation [rad], translation [m], tracking rate
KEYFRAME_ROT_THR, KEYFRAME_TRANS_THR, KEYFRAME_RATE_THR = 0.2618, 0.4, 0.5
KEYFRAME_SIGS = {
    "msckf_keyframe_select": (C.c_int, [_P, C.c_int, _I, _D, C.c_double, C.c_double, C.c_double, _I, _I, _I64, _I,
                                        _U8, _D, _D, _U8, _I]),
}
KEYFRAME_EXPORTED = tuple(KEYFRAME_SIGS)

# the frame's message handed from the front-end's tracks to the filter's map on the device
# (include/msckf_handoff.h), same library, both contexts
HANDOFF_SIGS = {
    "mfe_tracks_msg_put": (C.c_int, [_P, C.c_int, C.c_int, _I64, _D]),
    "mfe_tracks_msg_get": (C.c_int, [_P, C.c_int, _I, _I, _I64, _D]),
    "mfe_tracks_step_msg": (C.c_int, [_P, C.c_int, _I, _I, _I, _I, _D, _D, _I, _D, _D, _I, _D, _D, _D, _D, _I, _D, _D,
                                      _U32, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double,
                                      C.c_int, _I, _I, _I, _I64]),
    "msckf_map_add_lost_tracks": (C.c_int, [_P, _P, C.c_int, _I, _I, _I, _I, _I, _I64, _I]),
}
HANDOFF_EXPORTED = tuple(HANDOFF_SIGS)

# histogram equalisation / CLAHE at upload and the read-back of a slot (include/msckf_equalize.h),
# same library and context
EQ_NONE, EQ_HIST, EQ_CLAHE = 0, 1, 2
EQ_MAX_TILES = 16
EQUALIZE_SIGS = {
    "mfe_upload_many_eq": (C.c_int, [_P, C.c_int, _I, _U8, _I, _F, C.c_int, C.c_int]),
    "mfe_download": (C.c_int, [_P, C.c_int, C.c_int, _U8]),
    "mfe_download_deriv": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int16), C.POINTER(C.c_int16)]),
}
EQUALIZE_EXPORTED = tuple(EQUALIZE_SIGS)

# the landmark archive on the device and the pose / velocity covariance of a frame's read
# (include/msckf_odometry.h), same library and context
LANDMARKS_MAX_CAP = 65536
ODOMETRY_SIGS = {
    "msckf_landmarks_create": (C.c_int, [_P, C.c_int]),
    "msckf_landmarks_clear": (C.c_int, [_P, C.c_int, _I]),
    "msckf_landmarks_archive": (C.c_int, [_P, C.c_int, _I, _I, _I, _I]),
    "msckf_landmarks_get": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int, _I64, _I64, _I64, _D, _I, _D, _I]),
    "msckf_readback_odom": (C.c_int, [_P, C.c_int, _I, _D, _D, _I, C.c_int, C.c_int, _D, _U8, _D, _D, _U8, _I, _D, _D,
                                      _D]),
}
ODOMETRY_EXPORTED = tuple(ODOMETRY_SIGS)

# the zero-velocity update (include/msckf_zupt.h), same library and context
ZUPT_VEL, ZUPT_GYRO, ZUPT_ACC = 1, 2, 4


class MsckfZuptParamsT(C.Structure):
    _fields_ = [("vel_noise", C.c_double), ("gyro_noise", C.c_double), ("acc_noise", C.c_double),
                ("chi2", C.c_double), ("max_speed", C.c_double), ("rows", C.c_int32)]


ZUPT_SIGS = {
    "msckf_zupt_batch": (C.c_int, [_P, C.c_int, _I, _D, _D, C.POINTER(MsckfZuptParamsT)]),
    "msckf_zupt_results": (C.c_int, [_P, C.c_int, _I, _I, _D, _I64]),
}
ZUPT_EXPORTED = tuple(ZUPT_SIGS)

# the vision standstill cue (include/msckf_standstill.h): the front-end's motion statistic and the cued ZUPT
CUE_MOVING, CUE_STILL, CUE_UNKNOWN = 0, 1, 2
CUE_MODES = {"veto": 0, "either": 1}        # MSCKF_CUE_MODE_*
CUE_UNKNOWNS = {"imu": 0, "reject": 1}      # MSCKF_CUE_UNKNOWN_*


class MsckfZuptCueT(C.Structure):
    _fields_ = [("max_px", C.c_double), ("min_tracks", C.c_int32), ("mode", C.c_int32), ("unknown", C.c_int32)]


STANDSTILL_SIGS = {
    "mfe_motion_sets": (C.c_int, [_P, C.c_int, _I, _F, _F, C.c_double, _I, _F]),
    "mfe_tracks_motion_enable": (C.c_int, [_P, C.c_int, C.c_double]),
    "mfe_tracks_motion_get": (C.c_int, [_P, C.c_int, _I, _I, _F]),
    "msckf_zupt_batch_cued": (C.c_int, [_P, _P, C.c_int, _I, _I, _I, _F, _D, _D, C.POINTER(MsckfZuptParamsT),
                                        C.POINTER(MsckfZuptCueT)]),
    "msckf_zupt_cue_results": (C.c_int, [_P, C.c_int, _I, _I, _D, _I64, _I, _I, _F]),
}
STANDSTILL_EXPORTED = tuple(STANDSTILL_SIGS)

# the aiding fixes (include/msckf_aid.h), same library and context
AID_POS, AID_VEL, AID_BVEL, AID_DIR = 0x007, 0x038, 0x1c0, 0xe00


class MsckfAidParamsT(C.Structure):
    _fields_ = [("lever", C.c_double * 3), ("R_body", C.c_double * 9), ("dir_w", C.c_double * 3),
                ("chi2", C.c_double * 12)]


class MsckfAidFixT(C.Structure):
    _fields_ = [("z", C.c_double * 12), ("var", C.c_double * 12), ("dt", C.c_double), ("rows", C.c_int32)]


def aid_fix(z, var, dt, rows):
    """A msckf_aid_fix_t from z (12), var (12), the age dt and the row mask."""
    f = MsckfAidFixT()
    f.z[:] = [float(x) for x in z]
    f.var[:] = [float(x) for x in var]
    f.dt, f.rows = float(dt), int(rows)
    return f


AID_SIGS = {
    "msckf_aid_batch": (C.c_int, [_P, C.c_int, _I, C.POINTER(MsckfAidFixT), C.POINTER(MsckfAidParamsT)]),
    "msckf_aid_results": (C.c_int, [_P, C.c_int, _I, _I, _D, _I, _I64]),
}
AID_EXPORTED = tuple(AID_SIGS)

# the delayed aiding fixes (include/msckf_aid_delayed.h), same library and context
AID_DELAYED_POS, AID_DELAYED_DIR = 0x07, 0x38
AID_DELAYED_NONE, AID_DELAYED_APPLIED, AID_DELAYED_GATED, AID_DELAYED_NOT_PD, AID_DELAYED_BAD_SLOT = -1, 0, 1, 2, 3


class MsckfAidDelayedFixT(C.Structure):
    _fields_ = [("z", C.c_double * 6), ("var", C.c_double * 6), ("lam", C.c_double), ("rows", C.c_int32),
                ("slot", C.c_int32)]


def aid_delayed_fix(z, var, slot, lam, rows):
    """A msckf_aid_delayed_fix_t from z (6), var (6), the clone slot, the
    fraction lambda towards slot + 1 and the 6-bit row mask."""
    f = MsckfAidDelayedFixT()
    f.z[:] = [float(x) for x in z]
    f.var[:] = [float(x) for x in var]
    f.lam, f.rows, f.slot = float(lam), int(rows), int(slot)
    return f


AID_DELAYED_SIGS = {
    "msckf_aid_delayed_batch": (C.c_int, [_P, C.c_int, _I, C.POINTER(MsckfAidDelayedFixT),
                                          C.POINTER(MsckfAidParamsT)]),
    "msckf_aid_delayed_results": (C.c_int, [_P, C.c_int, _I, _I, _D, _I, _I, _I64]),
}
AID_DELAYED_EXPORTED = tuple(AID_DELAYED_SIGS)

# the anchor fixes (include/msckf_anchor.h), same library and context
ANCHOR_MAX = 64
ANCHOR_USED, ANCHOR_GATED, ANCHOR_DEPTH, ANCHOR_NOT_PD = 0, 1, 2, 3


class MsckfAnchorT(C.Structure):
    _fields_ = [("p_w", C.c_double * 3), ("cov", C.c_double * 6), ("z", C.c_double * 4)]


class MsckfAnchorParamsT(C.Structure):
    _fields_ = [("obs_var", C.c_double), ("chi2", C.c_double), ("min_depth", C.c_double),
                ("min_anchors", C.c_int32)]


ANCHOR_DTYPE = np.dtype([("p_w", "<f8", 3), ("cov", "<f8", 6), ("z", "<f8", 4)])   # msckf_anchor_t, packed doubles


def pack_anchors(p, cov, z):
    """msckf_anchor_t records of p (K, 3), cov (K, 3, 3) and z (K, 4): cov's six upper entries xx xy xz yy yz zz."""
    p, cov, z = np.asarray(p, float).reshape(-1, 3), np.asarray(cov, float).reshape(-1, 3, 3), \
        np.asarray(z, float).reshape(-1, 4)
    a = np.zeros(len(p), ANCHOR_DTYPE)
    a["p_w"], a["z"] = p, z
    a["cov"] = cov[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    return a


ANCHOR_SIGS = {
    "msckf_anchor_batch": (C.c_int, [_P, C.c_int, _I, _I, C.POINTER(MsckfAnchorT), C.POINTER(MsckfAnchorParamsT)]),
    "msckf_anchor_results": (C.c_int, [_P, C.c_int, _I, _I, _I, _I, _I64]),
    "msckf_anchor_status": (C.c_int, [_P, C.c_int, C.c_int, _U8, _D, _I]),
}
ANCHOR_EXPORTED = tuple(ANCHOR_SIGS)

# multi-GPU replica transport, RCCL (include/msckf_replicas.h), same library
REPLICA_SIGS = {
    "msckf_rccl_unique_id": (C.c_int, [_U8]),
    "msckf_rccl_init": (C.c_int, [_U8, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(_P)]),
    "msckf_rccl_allreduce": (C.c_int, [_P, _D, C.c_int, C.c_int]),
    "msckf_rccl_allgather": (C.c_int, [_P, C.c_void_p, C.c_int, C.c_void_p]),
    "msckf_rccl_set_timeout": (C.c_int, [_P, C.c_double]),
    "msckf_rccl_count": (C.c_int, [_P, _I, _I]),
    "msckf_rccl_destroy": (C.c_int, [_P]),
    "msckf_rccl_last_error": (C.c_char_p, []),
}
REPLICA_EXPORTED = tuple(REPLICA_SIGS)
RCCL_ID_BYTES = 128


def load_library(path: str = LIB_PATH):
    """Load and type the shared library (no device work)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(path):
            raise MsckfError("HIP extension %s is missing -- build it with `make` "
                             "(or __graft_entry__.build()); there is no CPU fallback" % path)
        lib = C.CDLL(path)
        for name, (res, args) in (list(_SIGS.items()) + list(FRONTEND_SIGS.items()) +
                                  list(FRONTEND_RANSAC_SIGS.items()) + list(FRONTEND_PIPELINE_SIGS.items()) +
                                  list(FRONTEND_LANES_SIGS.items()) + list(FRONTEND_TRACKS_SIGS.items()) +
                                  list(MAP_SIGS.items()) + list(KEYFRAME_SIGS.items()) + list(HANDOFF_SIGS.items()) +
                                  list(EQUALIZE_SIGS.items()) + list(ODOMETRY_SIGS.items()) +
                                  list(ZUPT_SIGS.items()) + list(STANDSTILL_SIGS.items()) + list(AID_SIGS.items()) + list(ANCHOR_SIGS.items()) +
                                  list(AID_DELAYED_SIGS.items()) +
                                  list(REPLICA_SIGS.items())):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def make_config(cfg: FilterConfig) -> MsckfConfigT:
    c = MsckfConfigT()
    c.gyro_noise, c.acc_noise = cfg.gyro_noise, cfg.acc_noise
    c.gyro_bias_noise, c.acc_bias_noise = cfg.gyro_bias_noise, cfg.acc_bias_noise
    c.observation_noise = cfg.observation_noise
    R01 = np.asarray(cfg.T_cn_cnm1, float)[:3, :3].ravel()
    t01 = np.asarray(cfg.T_cn_cnm1, float)[:3, 3]
    for i in range(9):
        c.R_cam0_cam1[i] = R01[i]
    for i in range(3):
        c.t_cam0_cam1[i] = t01[i]
    oc = cfg.optimization
    c.huber_epsilon, c.estimation_precision = oc.huber_epsilon, oc.estimation_precision
    c.initial_damping = oc.initial_damping
    c.outer_loop_max_iteration = oc.outer_loop_max_iteration
    c.inner_loop_max_iteration = oc.inner_loop_max_iteration
    return c


class Context:
    """One device context = ``n_filters`` independent filter slots of one
    scalar type on one HIP device.  Methods mirror the C-ABI one to one."""

    def __init__(self, cfg: FilterConfig, n_filters=1, n_cam_capacity=32, dtype=np.float64, device=0):
        self.lib = load_library()
        self.cfg = cfg
        self.dtype = np.dtype(dtype)
        self.B = n_filters
        self.Nmax = n_cam_capacity
        self._ccfg = make_config(cfg)
        h = _P()
        self._check(self.lib.msckf_create(C.byref(self._ccfg), device, self.dtype.itemsize,
                                          n_filters, n_cam_capacity, C.byref(h)))
        self.h = h
        self.lock = threading.RLock()
        self._pending = None   # the loaded batch's results, not read back yet (Pending)
        self.map_cap = None    # rows per filter of the feature map (map_create); None: the context has none
        self.landmark_cap = None   # rows per filter of the landmark rings (landmarks_create)

    def _check(self, rc):
        if rc < 0:
            raise MsckfError("msckf: %s (rc=%d)" % (self.lib.msckf_last_error().decode(), rc))
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.msckf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ----
    def set_state(self, f, imu, cams, P):
        imu = _f64(imu)
        n = 0 if cams is None else len(cams)
        cams_a = _f64(cams).reshape(n, CAM_LEN) if n else None
        P_a = _f64(P) if P is not None else None
        with self.lock:
            self._check(self.lib.msckf_set_state(self.h, f, _ptr(imu, C.c_double), n,
                                                 _ptr(cams_a, C.c_double), _ptr(P_a, C.c_double)))

    def get_state(self, f, want_P=True):
        imu = np.zeros(IMU_LEN)
        cams = np.zeros((self.Nmax, CAM_LEN))
        n = C.c_int32(0)
        with self.lock:
            self._check(self.lib.msckf_get_state(self.h, f, _ptr(imu, C.c_double), None, None, C.byref(n)))
            D = 21 + 6 * n.value
            P = np.zeros((D, D)) if want_P else None
            self._check(self.lib.msckf_get_state(self.h, f, _ptr(imu, C.c_double), _ptr(cams, C.c_double),
                                                 _ptr(P, C.c_double), C.byref(n)))
        return imu, cams[:n.value].copy(), P

    def cov_diag(self, f, i0, n):
        out = np.zeros(n)
        with self.lock:
            self._check(self.lib.msckf_get_cov_diag(self.h, f, i0, n, _ptr(out, C.c_double)))
        return out

    # ---- hot path ----
    def propagate(self, f, dt, gyro, acc):
        dt = _f64(dt)
        n = len(dt)
        if n == 0:
            return
        gyro = _f64(gyro, (n, 3))
        acc = _f64(acc, (n, 3))
        with self.lock:
            self._check(self.lib.msckf_propagate(self.h, f, n, _ptr(dt, C.c_double), _ptr(gyro, C.c_double),
                                                 _ptr(acc, C.c_double)))

    def augment(self, f):
        with self.lock:
            self._check(self.lib.msckf_augment(self.h, f))

    def triangulate(self, f, obs_off, obs_cam, obs_z):
        self.settle()
        obs_off, obs_cam = _i32(obs_off), _i32(obs_cam)
        nf = len(obs_off) - 1
        obs_z = _f64(obs_z, (len(obs_cam), 4))
        p = np.zeros((nf, 3))
        v = np.zeros(nf, np.uint8)
        with self.lock:
            self._check(self.lib.msckf_triangulate(self.h, f, nf, _ptr(obs_off, C.c_int32), _ptr(obs_cam, C.c_int32),
                                                   _ptr(obs_z, C.c_double), _ptr(p, C.c_double),
                                                   _ptr(v, C.c_uint8)))
        return p, v.astype(bool)

    def update(self, f, obs_off, obs_cam, obs_z, p_w, chi2, row_cap=0):
        self.settle()
        obs_off, obs_cam = _i32(obs_off), _i32(obs_cam)
        nf = len(obs_off) - 1
        obs_z = _f64(obs_z, (len(obs_cam), 4))
        p_w = _f64(p_w, (nf, 3))
        chi2 = _f64(chi2)
        acc = np.zeros(nf, np.uint8)
        gam = np.zeros(nf)
        rows = C.c_int32(0)
        with self.lock:
            self._check(self.lib.msckf_update(self.h, f, nf, _ptr(obs_off, C.c_int32), _ptr(obs_cam, C.c_int32),
                                              _ptr(obs_z, C.c_double), _ptr(p_w, C.c_double),
                                              _ptr(chi2, C.c_double), int(row_cap), _ptr(acc, C.c_uint8),
                                              _ptr(gam, C.c_double), C.byref(rows)))
        return acc.astype(bool), gam, rows.value

    def update_async(self, f, obs_off, obs_cam, obs_z, p_w, chi2, row_cap=0):
        """msckf_update without the wait: the batch of filter ``f`` is loaded
        and its chain (triangulation of the NaN rows of ``p_w`` fused in front,
        msckf_hip.h) enqueued; the returned Pending reads (accepted, gamma,
        p_w, valid, rows) on first use -- or when the next batch is loaded."""
        nf = len(obs_off) - 1
        feat_off = np.where(np.arange(self.B + 1) <= f, 0, nf).astype(np.int32)
        p_w = _f64(p_w, (nf, 3))
        self.batch_load(feat_off, obs_off, obs_cam, obs_z, p_w, chi2)
        self.batch_update(row_cap=row_cap, triangulate=not bool(np.isfinite(p_w).all()))
        return self.pending([(f, 0, nf)])[0]

    def pending(self, ranges):
        """Deferred results of the loaded batch, one view per (slot, first,
        end) feature range; the batch is read back once, for all of them."""
        self.settle()
        grp = _PendingBatch(self)
        self._pending = grp
        return [Pending(grp, s, a, b) for s, a, b in ranges]

    def settle(self):
        """Reads back the outstanding deferred batch (before its arena is
        reused by the next load)."""
        p, self._pending = self._pending, None
        if p is not None:
            p.read()

    def prune(self, f, slots):
        slots = _i32(slots)
        with self.lock:
            self._check(self.lib.msckf_prune(self.h, f, len(slots), _ptr(slots, C.c_int32)))

    # ---- multi-filter forms (one launch for a list of filter slots) ----
    def propagate_batch(self, filters, sample_off, dt, gyro, acc):
        filters, sample_off = _i32(filters), _i32(sample_off)
        n = int(sample_off[-1]) if len(sample_off) else 0
        dt = _f64(dt).reshape(n)
        gyro = _f64(gyro, (n, 3))
        acc = _f64(acc, (n, 3))
        with self.lock:
            self._check(self.lib.msckf_propagate_batch(self.h, len(filters), _ptr(filters, C.c_int32),
                                                       _ptr(sample_off, C.c_int32), _ptr(dt, C.c_double),
                                                       _ptr(gyro, C.c_double), _ptr(acc, C.c_double)))

    def augment_batch(self, filters):
        filters = _i32(filters)
        with self.lock:
            self._check(self.lib.msckf_augment_batch(self.h, len(filters), _ptr(filters, C.c_int32)))

    def prune_batch(self, filters, slot_off, slots):
        filters, slot_off, slots = _i32(filters), _i32(slot_off), _i32(slots)
        with self.lock:
            self._check(self.lib.msckf_prune_batch(self.h, len(filters), _ptr(filters, C.c_int32),
                                                   _ptr(slot_off, C.c_int32), _ptr(slots, C.c_int32)))

    def get_states_batch(self, filters, want_cams=True):
        """(imu records (n, IMU_LEN), list of cam arrays (n_cams_w, CAM_LEN))."""
        filters = _i32(filters)
        n = len(filters)
        imu = np.zeros((n, IMU_LEN))
        cams = np.zeros((n, self.Nmax, CAM_LEN)) if want_cams else None
        nc = np.zeros(n, np.int32)
        with self.lock:
            self._check(self.lib.msckf_get_states_batch(self.h, n, _ptr(filters, C.c_int32), _ptr(imu, C.c_double),
                                                        _ptr(cams, C.c_double), _ptr(nc, C.c_int32)))
        cl = [cams[w, :nc[w]].copy() for w in range(n)] if want_cams else [None] * n
        return imu, cl

    def cov_diag_batch(self, filters, i0, n):
        filters = _i32(filters)
        out = np.zeros((len(filters), n))
        with self.lock:
            self._check(self.lib.msckf_get_cov_diag_batch(self.h, len(filters), _ptr(filters, C.c_int32), i0, n,
                                                           _ptr(out, C.c_double)))
        return out

    def readback(self, filters, want_cams=True, cov=None):
        """A frame's sync point with ONE stream synchronisation (msckf_readback):
        (imu records (n, IMU_LEN), list of cam arrays, covariance diagonals
        (n, cov[1]) of [cov[0], cov[0] + cov[1]) or None).  An outstanding
        deferred batch (Pending) is read back in the same copy."""
        return self._readback(filters, want_cams, cov, None)

    def readback_odom(self, filters, R_body, want_cams=True, cov=None):
        """msckf_readback_odom (msckf_odometry.h): what ``readback`` returns,
        from the same single read, plus the listed filters' pose covariances
        (n, 6, 6) and velocity covariances (n, 3, 3) in the frame ``R_body``
        (3 x 3, the rotation of T_imu_body) rotates to."""
        return self._readback(filters, want_cams, cov, _f64(R_body, (3, 3)))

    def _readback(self, filters, want_cams, cov, R_body):
        filters = _i32(filters)
        n = len(filters)
        imu = np.zeros((n, IMU_LEN))
        cams = np.zeros((n, self.Nmax, CAM_LEN)) if want_cams else None
        nc = np.zeros(n, np.int32)
        i0, ncv = cov if cov else (0, 0)
        cv = np.zeros((n, ncv)) if ncv else None
        pend = self._pending if self._pending is not None and self._pending.res is None else None
        if pend is not None:
            nf = self._nf
            acc, gam, p, v = np.zeros(nf, np.uint8), np.zeros(nf), np.zeros((nf, 3)), np.zeros(nf, np.uint8)
            rows = np.zeros(self.B, np.int32)
        else:
            acc = gam = p = v = rows = None
        args = (self.h, n, _ptr(filters, C.c_int32), _ptr(imu, C.c_double), _ptr(cams, C.c_double),
                _ptr(nc, C.c_int32), int(i0), int(ncv), _ptr(cv, C.c_double), _ptr(acc, C.c_uint8),
                _ptr(gam, C.c_double), _ptr(p, C.c_double), _ptr(v, C.c_uint8), _ptr(rows, C.c_int32))
        with self.lock:
            if R_body is None:
                self._check(self.lib.msckf_readback(*args))
            else:
                pose_cov, vel_cov = np.zeros((n, 6, 6)), np.zeros((n, 3, 3))
                self._check(self.lib.msckf_readback_odom(*args, _ptr(R_body, C.c_double), _ptr(pose_cov, C.c_double),
                                                         _ptr(vel_cov, C.c_double)))
        if pend is not None:
            pend.res = (acc.astype(bool), gam, p, v.astype(bool), rows)
            self._pending = None
        cl = [cams[w, :nc[w]].copy() for w in range(n)] if want_cams else [None] * n
        return (imu, cl, cv) if R_body is None else (imu, cl, cv, pose_cov, vel_cov)

    def batch_triangulate(self):
        self._check(self.lib.msckf_batch_triangulate(self.h))

    # ---- throughput mode ----
    def batch_load(self, feat_off, obs_off, obs_cam, obs_z, p_w=None, chi2=None):
        self.settle()
        feat_off, obs_off, obs_cam = _i32(feat_off), _i32(obs_off), _i32(obs_cam)
        obs_z = _f64(obs_z, (len(obs_cam), 4))
        p_w = _f64(p_w) if p_w is not None else None
        chi2 = _f64(chi2) if chi2 is not None else None
        self._nf = int(feat_off[-1])
        with self.lock:
            self._check(self.lib.msckf_batch_load(self.h, _ptr(feat_off, C.c_int32), _ptr(obs_off, C.c_int32),
                                                  _ptr(obs_cam, C.c_int32), _ptr(obs_z, C.c_double),
                                                  _ptr(p_w, C.c_double), _ptr(chi2, C.c_double)))

    def batch_update(self, row_cap=0, triangulate=True):
        self._check(self.lib.msckf_batch_update(self.h, int(row_cap), TRIANGULATE if triangulate else 0))

    def batch_results(self):
        nf = self._nf
        acc = np.zeros(nf, np.uint8)
        gam = np.zeros(nf)
        p = np.zeros((nf, 3))
        v = np.zeros(nf, np.uint8)
        rows = np.zeros(self.B, np.int32)
        self._check(self.lib.msckf_batch_results(self.h, _ptr(acc, C.c_uint8), _ptr(gam, C.c_double),
                                                 _ptr(p, C.c_double), _ptr(v, C.c_uint8), _ptr(rows, C.c_int32)))
        return acc.astype(bool), gam, p, v.astype(bool), rows

    # ---- the feature map on the device (msckf_map.h) ----
    def map_create(self, cap):
        from .config import CHI2_05
        tab = _f64(CHI2_05[:99])
        with self.lock:
            self._check(self.lib.msckf_map_create(self.h, int(cap), _ptr(tab, C.c_double)))
        self.map_cap = int(cap)

    def map_clear(self, filters):
        filters = _i32(filters)
        with self.lock:
            self._check(self.lib.msckf_map_clear(self.h, len(filters), _ptr(filters, C.c_int32)))

    def map_put(self, f, ids, mask, z, p_w, init):
        """Writes filter ``f``'s table: ids [n], mask uint64 [n][2], z
        [n][n_cam_capacity][4], p_w [n][3], init [n]."""
        ids = np.ascontiguousarray(ids, np.int64)
        n = len(ids)
        mask = np.ascontiguousarray(mask, np.uint64).reshape(n, 2)
        z = _f64(z, (n, self.Nmax, 4))
        p_w = _f64(p_w, (n, 3))
        init = np.ascontiguousarray(init, np.uint8).reshape(n)
        with self.lock:
            self._check(self.lib.msckf_map_put(self.h, f, n, _ptr(ids, C.c_int64), _ptr(mask, C.c_uint64),
                                               _ptr(z, C.c_double), _ptr(p_w, C.c_double), _ptr(init, C.c_uint8)))

    def map_get(self, f):
        """Filter ``f``'s table: (ids, mask, z, p_w, init), n rows each."""
        cap = self.map_cap or 1   # without a map the library refuses (-1) before it writes anything
        n = C.c_int32(0)
        ids, mask = np.zeros(cap, np.int64), np.zeros((cap, 2), np.uint64)
        z, p_w, init = np.zeros((cap, self.Nmax, 4)), np.zeros((cap, 3)), np.zeros(cap, np.uint8)
        with self.lock:
            self._check(self.lib.msckf_map_get(self.h, f, C.byref(n), _ptr(ids, C.c_int64), _ptr(mask, C.c_uint64),
                                               _ptr(z, C.c_double), _ptr(p_w, C.c_double), _ptr(init, C.c_uint8)))
        n = n.value
        return ids[:n].copy(), mask[:n].copy(), z[:n].copy(), p_w[:n].copy(), init[:n].astype(bool)

    def _map_desc(self, nfilt):
        cap = self.map_cap or 1   # without a map the library refuses (-1) before it writes anything
        return np.zeros((nfilt, cap), np.int64), np.zeros((nfilt, cap, MAP_INFO), np.int32)

    def map_add_lost(self, filters, msg_off, ids, z):
        """One message per listed filter.  Returns per filter (tracked,
        n_before, candidate ids, candidate info [n][4] = M, 0, initialised, row)."""
        filters, msg_off = _i32(filters), _i32(msg_off)
        ids = np.ascontiguousarray(ids, np.int64)
        z = _f64(z, (len(ids), 4))
        k = len(filters)
        tracked, nbef, ncand = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        did, dinfo = self._map_desc(k)
        with self.lock:
            self._check(self.lib.msckf_map_add_lost(
                self.h, k, _ptr(filters, C.c_int32), _ptr(msg_off, C.c_int32), _ptr(ids, C.c_int64),
                _ptr(z, C.c_double), _ptr(tracked, C.c_int32), _ptr(nbef, C.c_int32), _ptr(ncand, C.c_int32),
                _ptr(did, C.c_int64), _ptr(dinfo, C.c_int32)))
        return [(int(tracked[w]), int(nbef[w]), did[w, :ncand[w]].copy(), dinfo[w, :ncand[w]].copy())
                for w in range(k)]

    def map_add_lost_tracks(self, filters, fe, lanes):
        """msckf_map_add_lost_tracks (msckf_handoff.h): listed filter w takes
        the message of lane ``lanes[w]`` of the front-end context ``fe`` (a
        ``frontend.Frontend``), read on the device.  Returns what
        ``map_add_lost`` returns."""
        filters, lanes = _i32(filters), _i32(lanes)
        k = len(filters)
        if len(lanes) != k:
            raise ValueError("%d lanes for %d filters" % (len(lanes), k))
        tracked, nbef, ncand = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.int32)
        did, dinfo = self._map_desc(k)
        with self.lock:
            self._check(self.lib.msckf_map_add_lost_tracks(
                self.h, fe.h, k, _ptr(filters, C.c_int32), _ptr(lanes, C.c_int32), _ptr(tracked, C.c_int32),
                _ptr(nbef, C.c_int32), _ptr(ncand, C.c_int32), _ptr(did, C.c_int64), _ptr(dinfo, C.c_int32)))
        return [(int(tracked[w]), int(nbef[w]), did[w, :ncand[w]].copy(), dinfo[w, :ncand[w]].copy())
                for w in range(k)]

    def map_prune_select(self, filters, slot_off, slots):
        """Per listed filter (involved ids, info [n][4] = M, involved count, initialised, row)."""
        filters, slot_off, slots = _i32(filters), _i32(slot_off), _i32(slots)
        k = len(filters)
        ninv = np.zeros(k, np.int32)
        did, dinfo = self._map_desc(k)
        with self.lock:
            self._check(self.lib.msckf_map_prune_select(
                self.h, k, _ptr(filters, C.c_int32), _ptr(slot_off, C.c_int32), _ptr(slots, C.c_int32),
                _ptr(ninv, C.c_int32), _ptr(did, C.c_int64), _ptr(dinfo, C.c_int32)))
        return [(did[w, :ninv[w]].copy(), dinfo[w, :ninv[w]].copy()) for w in range(k)]

    def keyframe_select(self, filters, rates, rot_thr=KEYFRAME_ROT_THR, trans_thr=KEYFRAME_TRANS_THR,
                        rate_thr=KEYFRAME_RATE_THR):
        """msckf_keyframe_select: the two cam slots of each listed filter chosen
        on the device from its cam states and ``rates`` (its tracking rate), and
        the prune select with them, one synchronisation.  Per listed filter
        (slots [2] ascending, involved ids, info [n][4] as map_prune_select).
        An outstanding deferred batch (Pending) is read back in the same copy."""
        filters = _i32(filters)
        k = len(filters)
        rates = _f64(rates, (k,))
        slots, ninv = np.zeros((k, 2), np.int32), np.zeros(k, np.int32)
        did, dinfo = self._map_desc(k)
        pend = self._pending if self._pending is not None and self._pending.res is None else None
        if pend is not None:
            nf = self._nf
            acc, gam, p, v = np.zeros(nf, np.uint8), np.zeros(nf), np.zeros((nf, 3)), np.zeros(nf, np.uint8)
            rows = np.zeros(self.B, np.int32)
        else:
            acc = gam = p = v = rows = None
        with self.lock:
            self._check(self.lib.msckf_keyframe_select(
                self.h, k, _ptr(filters, C.c_int32), _ptr(rates, C.c_double), float(rot_thr), float(trans_thr),
                float(rate_thr), _ptr(slots, C.c_int32), _ptr(ninv, C.c_int32), _ptr(did, C.c_int64),
                _ptr(dinfo, C.c_int32), _ptr(acc, C.c_uint8), _ptr(gam, C.c_double), _ptr(p, C.c_double),
                _ptr(v, C.c_uint8), _ptr(rows, C.c_int32)))
        if pend is not None:
            pend.res = (acc.astype(bool), gam, p, v.astype(bool), rows)
            self._pending = None
        return [(slots[w].copy(), did[w, :ninv[w]].copy(), dinfo[w, :ninv[w]].copy()) for w in range(k)]

    def map_load(self, mode, filters, feat_off, rows, counts, p_w=None):
        """msckf_map_load; the batch holds the features in ascending filter
        slot.  Returns {slot: (first, end)} feature ranges of the batch."""
        self.settle()
        filters, feat_off, rows, counts = _i32(filters), _i32(feat_off), _i32(rows), _i32(counts)
        p_w = _f64(p_w, (len(rows), 3)) if p_w is not None else None
        with self.lock:
            self._check(self.lib.msckf_map_load(self.h, int(mode), len(filters), _ptr(filters, C.c_int32),
                                                _ptr(feat_off, C.c_int32), _ptr(rows, C.c_int32),
                                                _ptr(counts, C.c_int32), _ptr(p_w, C.c_double)))
        self._nf = int(feat_off[-1]) if len(feat_off) else 0
        ranges, a = {}, 0
        for w in np.argsort(filters, kind="stable"):
            nfw = int(feat_off[w + 1] - feat_off[w])
            ranges[int(filters[w])] = (a, a + nfw)
            a += nfw
        return ranges

    def map_prune_commit(self, filters, ent_off, rows, valid, p_w):
        filters, ent_off, rows = _i32(filters), _i32(ent_off), _i32(rows)
        valid = np.ascontiguousarray(valid, np.uint8).reshape(len(rows))
        p_w = _f64(p_w, (len(rows), 3))
        with self.lock:
            self._check(self.lib.msckf_map_prune_commit(self.h, len(filters), _ptr(filters, C.c_int32),
                                                        _ptr(ent_off, C.c_int32), _ptr(rows, C.c_int32),
                                                        _ptr(valid, C.c_uint8), _ptr(p_w, C.c_double)))

    # ---- the landmark archive on the device (msckf_odometry.h) ----
    def landmarks_create(self, cap):
        with self.lock:
            self._check(self.lib.msckf_landmarks_create(self.h, int(cap)))
        self.landmark_cap = int(cap)

    def landmarks_clear(self, filters):
        filters = _i32(filters)
        with self.lock:
            self._check(self.lib.msckf_landmarks_clear(self.h, len(filters), _ptr(filters, C.c_int32)))

    def landmarks_archive(self, filters, feat_off, rows, stamps):
        """msckf_landmarks_archive: behind ``map_load(MAP_LOAD_LOST, filters,
        feat_off, rows, ..)`` and ``batch_update``, with the same lists; the
        accepted features go into the filters' rings on the device, stamped
        ``stamps[w]``.  Asynchronous, nothing comes back."""
        filters, feat_off, rows, stamps = _i32(filters), _i32(feat_off), _i32(rows), _i32(stamps)
        if len(stamps) != len(filters):
            raise ValueError("%d stamps for %d filters" % (len(stamps), len(filters)))
        with self.lock:
            self._check(self.lib.msckf_landmarks_archive(self.h, len(filters), _ptr(filters, C.c_int32),
                                                         _ptr(feat_off, C.c_int32), _ptr(rows, C.c_int32),
                                                         _ptr(stamps, C.c_int32)))

    def landmarks_get(self, f, first_seq=0, max_rows=None):
        """Filter ``f``'s ring from sequence number ``first_seq`` on, oldest
        first: (ids, p_w, n_obs, gamma, stamp, first_seq of the rows, seq)."""
        m = (self.landmark_cap or 1) if max_rows is None else int(max_rows)
        ids, p_w, n_obs = np.zeros(m, np.int64), np.zeros((m, 3)), np.zeros(m, np.int32)
        gam, stamp = np.zeros(m), np.zeros(m, np.int32)
        seq, first = C.c_int64(0), C.c_int64(0)
        with self.lock:
            k = self._check(self.lib.msckf_landmarks_get(
                self.h, f, int(first_seq), m, C.byref(seq), C.byref(first), _ptr(ids, C.c_int64),
                _ptr(p_w, C.c_double), _ptr(n_obs, C.c_int32), _ptr(gam, C.c_double), _ptr(stamp, C.c_int32)))
        return (ids[:k].copy(), p_w[:k].copy(), n_obs[:k].copy(), gam[:k].copy(), stamp[:k].copy(), first.value,
                seq.value)

    # ---- the zero-velocity update (msckf_zupt.h) ----
    def zupt_batch(self, filters, gyro_mean, acc_mean, prm):
        """msckf_zupt_batch: the gated standstill update of the listed filters
        with their mean angular rates / specific forces ([n][3] each) and the
        parameters ``prm`` (a ``MsckfZuptParamsT`` or a ``config.ZuptConfig``).
        Asynchronous, nothing comes back (``zupt_results``)."""
        filters = _i32(filters)
        n = len(filters)
        gyro_mean, acc_mean = _f64(gyro_mean, (n, 3)), _f64(acc_mean, (n, 3))
        if not isinstance(prm, MsckfZuptParamsT):
            prm = prm.params()
        with self.lock:
            self._check(self.lib.msckf_zupt_batch(self.h, n, _ptr(filters, C.c_int32), _ptr(gyro_mean, C.c_double),
                                                  _ptr(acc_mean, C.c_double), C.byref(prm)))

    def zupt_results(self, filters):
        """msckf_zupt_results (synchronises): (applied bool [n], gamma [n],
        count int64 [n] -- updates ever applied) of the listed filters."""
        filters = _i32(filters)
        n = len(filters)
        app, gam, cnt = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int64)
        with self.lock:
            self._check(self.lib.msckf_zupt_results(self.h, n, _ptr(filters, C.c_int32), _ptr(app, C.c_int32),
                                                    _ptr(gam, C.c_double), _ptr(cnt, C.c_int64)))
        return app.astype(bool), gam, cnt

    # ---- the cued zero-velocity update (msckf_standstill.h) ----
    def zupt_batch_cued(self, filters, gyro_mean, acc_mean, prm, cue, fe=None, lanes=None, cue_n=None, cue_d2=None):
        """msckf_zupt_batch_cued: ``zupt_batch`` with the vision cue ``cue`` (a
        ``MsckfZuptCueT`` or a ``config.VisionCue``) in the decision.  The cue's
        source is either the front-end context ``fe`` (a ``frontend.Frontend``)
        with listed filter w reading lane ``lanes[w]``'s motion record on the
        device, or the host arrays ``cue_n`` int32 [n] (< 0: no record) and
        ``cue_d2`` float32 [n].  Asynchronous (``zupt_cue_results``)."""
        filters = _i32(filters)
        n = len(filters)
        gyro_mean, acc_mean = _f64(gyro_mean, (n, 3)), _f64(acc_mean, (n, 3))
        if not isinstance(prm, MsckfZuptParamsT):
            prm = prm.params()
        if not isinstance(cue, MsckfZuptCueT):
            cue = cue.params()
        if fe is not None:
            lanes = _i32(lanes)
            if len(lanes) != n:
                raise ValueError("%d lanes for %d filters" % (len(lanes), n))
            cn = cd = None
        else:
            lanes = None
            cn = None if cue_n is None else _i32(cue_n)
            cd = None if cue_d2 is None else np.ascontiguousarray(cue_d2, np.float32).reshape(-1)
            if (cn is not None and len(cn) != n) or (cd is not None and len(cd) != n):
                raise ValueError("cue arrays do not match the %d filters" % n)
        with self.lock:
            self._check(self.lib.msckf_zupt_batch_cued(
                self.h, fe.h if fe is not None else None, n, _ptr(filters, C.c_int32), _ptr(lanes, C.c_int32),
                _ptr(cn, C.c_int32), _ptr(cd, C.c_float), _ptr(gyro_mean, C.c_double), _ptr(acc_mean, C.c_double),
                C.byref(prm), C.byref(cue)))

    def zupt_cue_results(self, filters):
        """msckf_zupt_cue_results (synchronises, one read): (applied bool [n],
        gamma [n], count int64 [n], cue int32 [n], cue_n int32 [n], cue_d2
        float32 [n]) of the listed filters."""
        filters = _i32(filters)
        n = len(filters)
        app, gam, cnt = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int64)
        cue, cn, cd = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        with self.lock:
            self._check(self.lib.msckf_zupt_cue_results(
                self.h, n, _ptr(filters, C.c_int32), _ptr(app, C.c_int32), _ptr(gam, C.c_double),
                _ptr(cnt, C.c_int64), _ptr(cue, C.c_int32), _ptr(cn, C.c_int32), _ptr(cd, C.c_float)))
        return app.astype(bool), gam, cnt, cue, cn, cd

    # ---- the aiding fixes (msckf_aid.h) ----
    def aid_batch(self, filters, fixes, prm):
        """msckf_aid_batch: the gated update of the listed filters, each with its
        own fix (``MsckfAidFixT``, see ``aid_fix``), and the parameters ``prm``
        (a ``MsckfAidParamsT`` or a ``config.AidingConfig``).  Asynchronous,
        nothing comes back (``aid_results``)."""
        filters = _i32(filters)
        n = len(filters)
        fixes = list(fixes)
        if len(fixes) != n:
            raise ValueError("aid_batch: %d filters but %d fixes" % (n, len(fixes)))
        arr = (MsckfAidFixT * max(n, 1))(*fixes)
        if not isinstance(prm, MsckfAidParamsT):
            prm = prm.params()
        with self.lock:
            self._check(self.lib.msckf_aid_batch(self.h, n, _ptr(filters, C.c_int32), arr, C.byref(prm)))

    def aid_results(self, filters):
        """msckf_aid_results (synchronises): (applied bool [n], gamma [n], rows
        int32 [n] -- the last fix's mask, count int64 [n] -- fixes ever applied)
        of the listed filters."""
        filters = _i32(filters)
        n = len(filters)
        app, gam, rows, cnt = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int64)
        with self.lock:
            self._check(self.lib.msckf_aid_results(self.h, n, _ptr(filters, C.c_int32), _ptr(app, C.c_int32),
                                                   _ptr(gam, C.c_double), _ptr(rows, C.c_int32),
                                                   _ptr(cnt, C.c_int64)))
        return app.astype(bool), gam, rows, cnt

    # ---- the delayed aiding fixes (msckf_aid_delayed.h) ----
    def aid_delayed_batch(self, filters, fixes, prm):
        """msckf_aid_delayed_batch: the gated update of the listed filters on
        their window clones, each with its own fix (``MsckfAidDelayedFixT``, see
        ``aid_delayed_fix``), and the parameters ``prm`` (a ``MsckfAidParamsT``
        or a ``config.AidingConfig``).  Asynchronous, nothing comes back
        (``aid_delayed_results``)."""
        filters = _i32(filters)
        n = len(filters)
        fixes = list(fixes)
        if len(fixes) != n:
            raise ValueError("aid_delayed_batch: %d filters but %d fixes" % (n, len(fixes)))
        arr = (MsckfAidDelayedFixT * max(n, 1))(*fixes)
        if not isinstance(prm, MsckfAidParamsT):
            prm = prm.params()
        with self.lock:
            self._check(self.lib.msckf_aid_delayed_batch(self.h, n, _ptr(filters, C.c_int32), arr, C.byref(prm)))

    def aid_delayed_results(self, filters):
        """msckf_aid_delayed_results (synchronises): (applied bool [n], gamma
        [n], rows int32 [n] -- the last fix's mask, status int32 [n] --
        ``AID_DELAYED_*``, count int64 [n] -- delayed fixes ever applied) of the
        listed filters."""
        filters = _i32(filters)
        n = len(filters)
        app, gam, rows, sta, cnt = (np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32),
                                    np.zeros(n, np.int64))
        with self.lock:
            self._check(self.lib.msckf_aid_delayed_results(self.h, n, _ptr(filters, C.c_int32), _ptr(app, C.c_int32),
                                                           _ptr(gam, C.c_double), _ptr(rows, C.c_int32),
                                                           _ptr(sta, C.c_int32), _ptr(cnt, C.c_int64)))
        return app.astype(bool), gam, rows, sta, cnt

    # ---- the anchor fixes (msckf_anchor.h) ----
    def anchor_batch(self, filters, anchors, prm):
        """msckf_anchor_batch: the gated update of the listed filters, each with
        its own anchors -- ``anchors[k]`` is ``(p (K, 3), cov (K, 3, 3), z (K,
        4))`` in the filter's world frame or a ``pack_anchors`` array -- and the
        parameters ``prm`` (a ``MsckfAnchorParamsT``).  Asynchronous, nothing
        comes back (``anchor_results``, ``anchor_status``)."""
        filters = _i32(filters)
        n = len(filters)
        anchors = [a if isinstance(a, np.ndarray) and a.dtype == ANCHOR_DTYPE else pack_anchors(*a) for a in anchors]
        if len(anchors) != n:
            raise ValueError("anchor_batch: %d filters but %d anchor lists" % (n, len(anchors)))
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(a) for a in anchors])
        arr = np.ascontiguousarray(np.concatenate(anchors)) if n else np.zeros(0, ANCHOR_DTYPE)
        if len(arr) == 0:
            arr = np.zeros(1, ANCHOR_DTYPE)
        with self.lock:
            self._check(self.lib.msckf_anchor_batch(self.h, n, _ptr(filters, C.c_int32), _ptr(off, C.c_int32),
                                                    arr.ctypes.data_as(C.POINTER(MsckfAnchorT)), C.byref(prm)))

    def anchor_results(self, filters):
        """msckf_anchor_results (synchronises): (applied bool [n], used int32
        [n], rows int32 [n], count int64 [n] -- updates ever applied) of the
        listed filters."""
        filters = _i32(filters)
        n = len(filters)
        app, used, rows, cnt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        with self.lock:
            self._check(self.lib.msckf_anchor_results(self.h, n, _ptr(filters, C.c_int32), _ptr(app, C.c_int32),
                                                      _ptr(used, C.c_int32), _ptr(rows, C.c_int32),
                                                      _ptr(cnt, C.c_int64)))
        return app.astype(bool), used, rows, cnt

    def anchor_status(self, filter):
        """msckf_anchor_status (synchronises): (status uint8 [K], gamma [K]) of
        the anchors of the filter's last call."""
        status, gamma, n = np.zeros(ANCHOR_MAX, np.uint8), np.zeros(ANCHOR_MAX), np.zeros(1, np.int32)
        with self.lock:
            self._check(self.lib.msckf_anchor_status(self.h, int(filter), ANCHOR_MAX, _ptr(status, C.c_uint8),
                                                     _ptr(gamma, C.c_double), _ptr(n, C.c_int32)))
        return status[:n[0]].copy(), gamma[:n[0]].copy()

    def device_info(self):
        """(HIP device index, PCI bus id) this context runs on."""
        dev = np.zeros(1, np.int32)
        buf = C.create_string_buffer(64)
        with self.lock:
            self._check(self.lib.msckf_device_info(self.h, _ptr(dev, C.c_int32), buf, 64))
        return int(dev[0]), buf.value.decode()

    def snapshot(self):
        self._check(self.lib.msckf_snapshot(self.h))

    def restore(self):
        self._check(self.lib.msckf_restore(self.h))

    def sync(self):
        self._check(self.lib.msckf_sync(self.h))

    def set_profiling(self, on=True):
        self._check(self.lib.msckf_set_profiling(self.h, 1 if on else 0))

    def set_profiling_stage(self, stage):
        """Time one stage only (None: profiling off)."""
        self._check(self.lib.msckf_set_profiling_stage(self.h, None if stage is None else stage.encode()))

    def kernel_times(self):
        ms = np.zeros(64)
        cnt = np.zeros(64, np.int32)
        buf = C.create_string_buffer(4096)
        k = self._check(self.lib.msckf_kernel_times(self.h, 64, _ptr(ms, C.c_double), _ptr(cnt, C.c_int32),
                                                    buf, 4096))
        names = buf.raw.split(b"\0")[:k]
        return {n.decode(): (float(ms[i]), int(cnt[i])) for i, n in enumerate(names)}


class _PendingBatch:
    """The results of one loaded batch, read back (one synchronisation) on demand."""
    __slots__ = ("ctx", "res")

    def __init__(self, ctx):
        self.ctx, self.res = ctx, None

    def read(self):
        if self.res is None:
            self.res = self.ctx.batch_results()
            if self.ctx._pending is self:
                self.ctx._pending = None
        return self.res


class Pending:
    """Deferred (accepted, gamma, p_w, valid, rows) of one filter's features."""
    __slots__ = ("grp", "slot", "a", "b")

    def __init__(self, grp, slot, a, b):
        self.grp, self.slot, self.a, self.b = grp, slot, a, b

    def get(self):
        acc, gam, p, v, rows = self.grp.read()
        a, b = self.a, self.b
        return acc[a:b].copy(), gam[a:b].copy(), p[a:b].copy(), v[a:b].copy(), int(rows[self.slot])


def pack_imu(q, p, v, bg, ba, q_null, p_null, v_null, R_imu_cam0, t_cam0_imu, gravity, alias):
    r = np.zeros(IMU_LEN)
    r[I_Q:I_Q + 4] = q
    r[I_P:I_P + 3] = p
    r[I_V:I_V + 3] = v
    r[I_BG:I_BG + 3] = bg
    r[I_BA:I_BA + 3] = ba
    r[I_QN:I_QN + 4] = q_null
    r[I_PN:I_PN + 3] = p_null
    r[I_VN:I_VN + 3] = v_null
    r[I_RIC:I_RIC + 9] = np.asarray(R_imu_cam0).ravel()
    r[I_TCI:I_TCI + 3] = t_cam0_imu
    r[I_G:I_G + 3] = gravity
    r[I_ALIAS] = 1.0 if alias else 0.0
    return r


def unpack_imu(r):
    return dict(q=r[I_Q:I_Q + 4].copy(), p=r[I_P:I_P + 3].copy(), v=r[I_V:I_V + 3].copy(),
                bg=r[I_BG:I_BG + 3].copy(), ba=r[I_BA:I_BA + 3].copy(), q_null=r[I_QN:I_QN + 4].copy(),
                p_null=r[I_PN:I_PN + 3].copy(), v_null=r[I_VN:I_VN + 3].copy(),
                R_imu_cam0=r[I_RIC:I_RIC + 9].reshape(3, 3).copy(), t_cam0_imu=r[I_TCI:I_TCI + 3].copy(),
                gravity=r[I_G:I_G + 3].copy(), alias=bool(r[I_ALIAS] != 0))


def pack_cams(q, p, q_null):
    q = np.atleast_2d(q)
    n = len(q)
    out = np.zeros((n, CAM_LEN))
    out[:, 0:4] = q
    out[:, 4:7] = np.atleast_2d(p)
    out[:, 7:11] = np.atleast_2d(q_null)
    return out
