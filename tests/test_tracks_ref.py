"""CPU checks of MultiImageProcessor with ``device_tracks`` (the host side of
include/msckf_tracks.h) on the stand-in tests/frontend_tracks_ref.py, whose
``tracks_step`` restates the header's steps 1-9 in numpy on the CPU oracle's
operators:
  * two lanes, the rectified and the euroc scene of tests/golden/frontend_ref.npz,
    publish the ids of the recorded reference frames and their coordinates to
    1e-12 (the bound of tests/test_lanes_ref.py against this fixture) -- in step,
    and with lane 1 started two frames late;
  * with RANSAC on in one lane the lanes publish exactly what they publish with
    the switch off on the same stand-in;
  * a step in which all lanes track is two device calls, for 2 and 5 lanes alike;
  * lanes that cannot share the call are rejected by the constructor;
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
import frontend_tracks_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_lanes(monkeypatch, tracks=True, **cfg_kw):
    monkeypatch.setattr(fe_mod, "Frontend", tr.TracksOracleFrontend)
    g = golden("frontend_ref")
    cfgs = []
    for i, name in enumerate(SCENES):
        cfg = scene_config(g, name)
        cfg.device_pipeline, cfg.device_tracks = True, tracks
        for k, v in cfg_kw.items():
            setattr(cfg, k, v[i] if isinstance(v, tuple) else v)
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
        logs.append((lanes, [c for c in mp.fe.calls if c != "tracks_create"]))
        del mp.fe.calls[:]
    check_against_reference(g, lr.run_lanes(mp, streams, on_step=on_step))
    assert logs[0] == ([0, 1], ["upload_many", "fast", "fast", "stereo_match_sets", "undistort_sets", "tracks_put",
                                "tracks_put"])
    for lanes, calls in logs[1:]:
        assert calls == ["upload_many", "tracks_step"], (lanes, calls)
    assert mp.launches["tracks_step"] == len(logs) - 1 and mp.launches["upload"] == len(logs)
    # the table is the published frame, and the counters reach num_features
    ids, life, cam0, cam1, next_id = mp.tracks(0)
    np.testing.assert_array_equal(ids, reference_frames(g, SCENES[0])[-1][0])
    assert len(life) == len(cam0) == len(cam1) == len(ids) and next_id == mp.lanes[0].next_feature_id > ids.max()
    nf = mp.lanes[0].num_features
    assert nf["before_tracking"] >= nf["after_tracking"] >= nf["after_matching"] == nf["after_ransac"] > 0


def test_lane_started_late_publishes_the_same(monkeypatch):
    g, mp, streams = golden_lanes(monkeypatch)
    logs = []

    def on_step(step, lanes):
        logs.append([c for c in mp.fe.calls if c != "tracks_create"])
        del mp.fe.calls[:]
    check_against_reference(g, lr.run_lanes(mp, streams, start=[0, 2], on_step=on_step))
    # step 2: lane 1's first frame on the existing path next to lane 0's tracked frame
    assert logs[2] == ["upload_many", "fast", "stereo_match_sets", "undistort_sets", "tracks_put", "tracks_step"]
    assert logs[1] == logs[3] == ["upload_many", "tracks_step"]


def test_ransac_lane_publishes_what_the_host_tables_publish(monkeypatch):
    kw = dict(ransac_enabled=(True, False), ransac_seed=5)
    g, mp, streams = golden_lanes(monkeypatch, **kw)
    got = lr.run_lanes(mp, streams)
    assert mp.fe.cover["empty_table"] == 0
    g, mp0, streams = golden_lanes(monkeypatch, tracks=False, **kw)
    want = lr.run_lanes(mp0, streams)
    assert mp0.launches["ransac"] > 0 and mp.launches["tracks_step"] > 0 and "lk" not in mp.launches
    for lane, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b)
        for k, ((ids, uv), (wids, wuv)) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(ids, wids, err_msg="lane %d frame %d" % (lane, k))
            assert uv.tobytes() == wuv.tobytes(), (lane, k)
    for ip, ip0 in zip(mp.lanes, mp0.lanes):
        assert dict(ip.num_features) == dict(ip0.num_features) and ip.next_feature_id == ip0.next_feature_id


def small_lanes(monkeypatch, S):
    """S lanes on a textured 96 x 64 scene each, three frames (the scenes of
    tests/test_lanes_ref.py); returns the stand-in's calls per step."""
    monkeypatch.setattr(fe_mod, "Frontend", tr.TracksOracleFrontend)
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
            pyramid_levels=1, device_pipeline=True, device_tracks=True, ransac_enabled=i == 1, ransac_seed=i))
        streams.append(lr.stream_frames(fs.texture_fn(3 + i, W=W, H=H), W, H, 3, (1.0 + 0.25 * i, -0.5),
                                        (0.0, 0.0, 0.0), 4.0))
    mp = fe_mod.MultiImageProcessor(S, lane_configs=cfgs)
    logs = []

    def on_step(step, lanes):
        logs.append([c for c in mp.fe.calls if c != "tracks_create"])
        del mp.fe.calls[:]
    got = lr.run_lanes(mp, streams, on_step=on_step)
    assert all(len(lane[-1][0]) > 0 for lane in got)
    return logs, mp


@pytest.mark.parametrize("S", [2, 5])
def test_a_tracking_step_is_two_device_calls(monkeypatch, S):
    logs, mp = small_lanes(monkeypatch, S)
    assert logs[0] == ["upload_many"] + ["fast"] * S + ["stereo_match_sets", "undistort_sets"] + ["tracks_put"] * S
    assert logs[1] == ["upload_many", "tracks_step"] and logs[2] == ["upload_many", "tracks_step"]
    assert dict(mp.launches) == {"upload": 3, "fast": S, "stereo_match": 1, "undistort": 1, "tracks_put": S,
                                 "tracks_step": 2}
    assert mp.fe.tracks_cap == 4 * (3 + 5)                 # the smallest tables the grid allows


def test_lanes_that_cannot_share_the_call_are_rejected(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", tr.TracksOracleFrontend)
    on = lambda **kw: fe_mod.FrontendConfig(device_pipeline=True, device_tracks=True, **kw)
    off = fe_mod.FrontendConfig(device_pipeline=True)
    with pytest.raises(ValueError, match="lane 1.*device_tracks"):
        fe_mod.MultiImageProcessor(2, lane_configs=[on(), off])
    with pytest.raises(ValueError, match="lane 2.*device_tracks"):
        fe_mod.MultiImageProcessor(3, lane_configs=[off, off, on()])
    with pytest.raises(ValueError, match="lane 1.*grid_min_feature_num"):
        fe_mod.MultiImageProcessor(2, lane_configs=[on(), on(grid_min_feature_num=2)])
    with pytest.raises(ValueError, match="lane 2.*grid_max_feature_num"):
        fe_mod.MultiImageProcessor(3, lane_configs=[on(), on(), on(grid_max_feature_num=6)])
    rs = lambda **kw: on(ransac_enabled=True, **kw)
    with pytest.raises(ValueError, match="lane 2.*ransac_threshold.*lane 1"):
        fe_mod.MultiImageProcessor(3, lane_configs=[on(), rs(), rs(ransac_threshold=2)])
    with pytest.raises(ValueError, match="lane 1.*ransac_success_probability"):
        fe_mod.MultiImageProcessor(2, lane_configs=[rs(), rs(ransac_success_probability=0.999)])
    # a lane without RANSAC may differ in its (unused) RANSAC fields; the switch needs device_pipeline
    mp = fe_mod.MultiImageProcessor(2, lane_configs=[on(ransac_threshold=7), rs()])
    assert mp.device_tracks and mp.fe.tracks_cap == 20 * 8 and mp._tracks_ransac == (3, 7)
    with pytest.raises(ValueError, match="device_pipeline"):
        fe_mod.ImageProcessor(fe_mod.FrontendConfig(device_tracks=True))
    mp = fe_mod.MultiImageProcessor(2, fe_mod.FrontendConfig(device_tracks=True))     # builds its lanes' configs
    assert mp.device_tracks and all(ip.config.device_tracks and ip.config.device_pipeline for ip in mp.lanes)
    assert not fe_mod.MultiImageProcessor(2).device_tracks and not fe_mod.FrontendConfig().device_tracks


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_tracks_exports_and_binding():
    """include/msckf_tracks.h is exported by the same library and typed one to
    one by the binding (its own table; the other headers keep their symbols)."""
    syms = header_symbols("msckf_tracks.h", "mfe_tracks_")
    assert syms == ["mfe_tracks_create", "mfe_tracks_get", "mfe_tracks_put", "mfe_tracks_step"]
    assert sorted(_lib.TRACKS_EXPORTED) == syms
    assert header_symbols("msckf_tracks.h", "mfe_") == syms
    assert not set(syms) & (set(_lib.FRONTEND_EXPORTED) | set(_lib.FRONTEND_RANSAC_EXPORTED) |
                            set(_lib.FRONTEND_PIPELINE_EXPORTED) | set(_lib.FRONTEND_LANES_EXPORTED))
    src = open(os.path.join(ROOT, "include", "msckf_tracks.h")).read()
    assert int(re.search(r"#define MFE_TRACKS_COUNTERS (\d+)", src).group(1)) == _lib.TRACKS_COUNTERS == \
        len(fe_mod.TRACKS_COUNTER_NAMES)
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (_, args) in _lib.FRONTEND_TRACKS_SIGS.items():      # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    lib = ctypes.CDLL(_lib.LIB_PATH)                               # the suite runs on a built tree
    for s in syms:
        assert hasattr(lib, s), s
