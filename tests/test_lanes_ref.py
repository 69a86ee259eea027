"""CPU checks of MultiImageProcessor (the host side of include/msckf_lanes.h)
on the stand-in tests/frontend_lanes_ref.py, whose set calls loop the CPU
oracle's single operators:
  * two lanes, the rectified and the euroc scene of tests/golden/frontend_ref.npz
    (one size, two calibrations), publish the ids of the recorded reference
    frames and their coordinates to 1e-12, the bound of
    tests/test_pipeline_ref.py against this fixture -- stepped together, and
    again with lane 1 started two frames late, so that fast, lk and fast_grid
    requests of different lanes coexist;
  * the device calls of a step in which every lane tracks, for 2 and for 5
    lanes alike: one set call per stage;
  * lanes that cannot share a call are rejected by the constructor;
  * the new header against its binding table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from conftest import golden
from frontend_ref_scenes import SCENES, scene_config, reference_frames
import frontend_synth as fs
import frontend_lanes_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACK_STEP = ["upload_many", "lk_sets", "stereo_match_sets", "fast_grid_sets", "stereo_match_sets", "undistort_sets"]
TRACK_STEP_RANSAC = TRACK_STEP[:3] + ["two_point_ransac"] + TRACK_STEP[3:]


def golden_lanes(monkeypatch, **cfg_kw):
    monkeypatch.setattr(fe_mod, "Frontend", lr.LanesOracleFrontend)
    g = golden("frontend_ref")
    cfgs = []
    for name in SCENES:
        cfg = scene_config(g, name)
        cfg.device_pipeline = True
        for k, v in cfg_kw.items():
            setattr(cfg, k, v)
        cfgs.append(cfg)
    return g, fe_mod.MultiImageProcessor(len(SCENES), lane_configs=cfgs), [lr.scene_frames(g, n) for n in SCENES]


def check_against_reference(g, got):
    for name, lane in zip(SCENES, got):
        ref = reference_frames(g, name)
        assert len(lane) == len(ref)
        for k, ((ids, uv), (rids, ruv)) in enumerate(zip(lane, ref)):
            np.testing.assert_array_equal(ids, rids, err_msg="%s frame %d" % (name, k))
            np.testing.assert_allclose(uv, ruv, rtol=0, atol=1e-12, err_msg="%s frame %d" % (name, k))
        assert len(lane[-1][0]) >= 50


def test_two_lanes_in_step_vs_recorded_frames(monkeypatch):
    g, mp, streams = golden_lanes(monkeypatch)
    logs = []

    def on_step(step, lanes):
        logs.append((lanes, list(mp.fe.calls)))
        del mp.fe.calls[:]
    check_against_reference(g, lr.run_lanes(mp, streams, on_step=on_step))
    # both first frames in one step: the single fast per lane, everything else shared
    assert logs[0] == ([0, 1], ["upload_many", "fast", "fast", "stereo_match_sets", "undistort_sets"])
    for lanes, calls in logs[1:]:
        assert calls == TRACK_STEP, (lanes, calls)      # also once lane 1 (6 frames of 8) has ended
    assert mp.launches["fast"] == 2 and mp.launches["lk"] == len(logs) - 1
    assert mp.launches["stereo_match"] == 2 * len(logs) - 1 and mp.launches["upload"] == len(logs)


def test_lane_started_late_publishes_the_same(monkeypatch):
    g, mp, streams = golden_lanes(monkeypatch)
    logs = []

    def on_step(step, lanes):
        logs.append(list(mp.fe.calls))
        del mp.fe.calls[:]
    check_against_reference(g, lr.run_lanes(mp, streams, start=[0, 2], on_step=on_step))
    # step 2: lane 1's first frame next to lane 0's tracked frame -- its fast is served before lane 0's lk,
    # its stereo match joins lane 0's first one, and the undistort waits for lane 0's second
    assert logs[2] == ["upload_many", "fast", "lk_sets", "stereo_match_sets", "fast_grid_sets", "stereo_match_sets",
                       "undistort_sets"]
    assert logs[3] == TRACK_STEP


def small_lanes(monkeypatch, S, ransac=()):
    """S lanes on a textured 96 x 64 scene each (its own texture, motion and
    baseline), three frames; returns the stand-in's calls per step."""
    monkeypatch.setattr(fe_mod, "Frontend", lr.LanesOracleFrontend)
    W, H = 96, 64
    K = np.array([80.0, 80.0, 48.0, 32.0])
    cfgs, streams = [], []
    for i in range(S):
        Ti1 = np.eye(4)
        Ti1[0, 3] = -0.11 - 0.01 * i
        cfgs.append(fe_mod.FrontendConfig(
            T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_intrinsics=K, cam1_intrinsics=K,
            cam0_distortion_coeffs=np.zeros(4), cam1_distortion_coeffs=np.zeros(4),
            cam0_resolution=np.array([W, H]), cam1_resolution=np.array([W, H]), grid_row=2, grid_col=2,
            pyramid_levels=1, device_pipeline=True, ransac_enabled=i in ransac, ransac_seed=i))
        streams.append(lr.stream_frames(fs.texture_fn(3 + i, W=W, H=H), W, H, 3, (1.0 + 0.25 * i, -0.5),
                                        (0.0, 0.0, 0.0), 4.0))
    mp = fe_mod.MultiImageProcessor(S, lane_configs=cfgs)
    logs = []

    def on_step(step, lanes):
        logs.append(list(mp.fe.calls))
        del mp.fe.calls[:]
    got = lr.run_lanes(mp, streams, on_step=on_step)
    assert all(len(lane[-1][0]) > 0 for lane in got)
    return logs, mp


@pytest.mark.parametrize("S", [2, 5])
def test_call_counts_of_a_tracking_step(monkeypatch, S):
    logs, mp = small_lanes(monkeypatch, S)
    assert logs[0] == ["upload_many"] + ["fast"] * S + ["stereo_match_sets", "undistort_sets"]
    assert logs[1] == TRACK_STEP and logs[2] == TRACK_STEP
    assert dict(mp.launches) == {"upload": 3, "fast": S, "lk": 2, "stereo_match": 5, "fast_grid": 2, "undistort": 3}


@pytest.mark.parametrize("S,ransac", [(2, (0, 1)), (5, (1, 3))])
def test_call_counts_with_ransac(monkeypatch, S, ransac):
    """RANSAC on in all lanes or in some: one call after the first stereo
    match, the lanes without it waiting at fast_grid."""
    logs, mp = small_lanes(monkeypatch, S, ransac)
    assert logs[1] == TRACK_STEP_RANSAC and logs[2] == TRACK_STEP_RANSAC
    assert mp.launches["ransac"] == 2


def test_lanes_that_cannot_share_a_call_are_rejected(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", lr.LanesOracleFrontend)
    on = lambda **kw: fe_mod.FrontendConfig(device_pipeline=True, **kw)
    small = dict(cam0_resolution=np.array([376, 240]), cam1_resolution=np.array([376, 240]))
    with pytest.raises(ValueError, match="lane 1.*resolution"):
        fe_mod.MultiImageProcessor(2, lane_configs=[on(), on(**small)])
    with pytest.raises(ValueError, match="lane 2.*device_pipeline"):
        fe_mod.MultiImageProcessor(3, lane_configs=[on(), on(), fe_mod.FrontendConfig()])
    with pytest.raises(ValueError, match="lane 1.*patch_size"):
        fe_mod.MultiImageProcessor(2, lane_configs=[on(), on(patch_size=11)])
    with pytest.raises(ValueError):
        fe_mod.MultiImageProcessor(2, lane_configs=[on()])
    mp = fe_mod.MultiImageProcessor(3)          # builds its own configs: the switch is on
    assert len(mp) == 3 and all(ip.config.device_pipeline for ip in mp.lanes)
    assert [ip._slot_prev for ip in mp.lanes] == [0, 3, 6] and all(ip.fe is mp.fe for ip in mp.lanes)
    # three slots per lane, and a point limit for all lanes' first frames (each may match 2^16 keypoints)
    assert mp.fe.nslot == 9 and mp.fe.max_points == 3 << 16
    from msckf_amd.scheduler import MultiImageProcessor, MultiMSCKF   # exported next to MultiMSCKF
    assert MultiImageProcessor is fe_mod.MultiImageProcessor and MultiMSCKF is not None


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_lanes_exports_and_binding():
    """include/msckf_lanes.h is exported by the same library and typed one to
    one by the binding (its own table; msckf_frontend.h keeps its 8 symbols)."""
    syms = header_symbols("msckf_lanes.h", "mfe_")
    assert syms == ["mfe_fast_grid_sets", "mfe_lk_sets", "mfe_stereo_match_sets", "mfe_undistort_sets",
                    "mfe_upload_many"]
    assert sorted(_lib.FRONTEND_LANES_EXPORTED) == syms
    assert not set(syms) & (set(_lib.FRONTEND_EXPORTED) | set(_lib.FRONTEND_RANSAC_EXPORTED) |
                            set(_lib.FRONTEND_PIPELINE_EXPORTED))
    src = open(os.path.join(ROOT, "include", "msckf_lanes.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MFE_MAX_[A-Z_]+) (\d+)", src)}
    assert consts == {"MFE_MAX_SLOTS": _lib.MAX_SLOTS, "MFE_MAX_SETS": _lib.MAX_SETS}
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (_, args) in _lib.FRONTEND_LANES_SIGS.items():       # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
