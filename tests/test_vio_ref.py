"""CPU checks of msckf_amd.vio (StereoVIO / MultiStereoVIO) on the stand-ins of
tests/vio_ref.py, one lane (RecordingContext.map_load serves one filter):

the ``euroc`` scene of tests/golden/frontend_ref.npz extended to 30 frames,
FilterConfig.max_cam_state_size = 4.  Gravity initialises at frame 20, so the
stream gives 11 results with update, triangulate and prune requests among
them (asserted, so the comparison cannot be vacuous).  StereoVIO with either
hand-off returns what MultiImageProcessor(device_tracks, arrays=True) wired by
hand into MultiMSCKF(device_map, device_keyframes) returns, leaves the same
``ctx.sent`` log and the same map; with "device" a tracked frame is
``upload_many, tracks_step`` in message form and the filter never takes a
message from the host.  Also: the TrackMessage rule, the constructor rules, the
new header against its binding table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd
import msckf_amd.frontend as fe_mod
import msckf_amd.scheduler as sched_mod
import msckf_amd.vio as vio_mod
from msckf_amd import _lib
from msckf_amd.msckf import MSCKF, FeatureArrays, TrackMessage
from conftest import golden
from frontend_ref_scenes import scene_config
import frontend_synth as fs
import frontend_lanes_ref as lr
import feature_map_ref as fr
import vio_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES = 30
_runs = {}


def stand_ins(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", vr.VioOracleFrontend)
    monkeypatch.setattr(_lib, "Context", vr.VioRecordingContext)


def euroc_stream():
    g = golden("frontend_ref")
    W, H = (int(v) for v in g["size"])
    f = fs.texture_fn(int(g["euroc_seed"]), W=W, H=H)
    frames = lr.stream_frames(f, W, H, N_FRAMES, g["euroc_step"], g["euroc_gyro"], float(g["euroc_disparity"]))
    return scene_config(g, "euroc"), frames


def filter_config():
    cfg = msckf_amd.FilterConfig()
    cfg.max_cam_state_size = 4
    return cfg


def run(monkeypatch, which):
    """``which``: "wired" (the two classes by hand), "host" or "device" (StereoVIO).
    Returns dict(results, sent, map, fe_calls per frame, map_calls, launches)."""
    if which in _runs:
        return _runs[which]
    stand_ins(monkeypatch)
    fcfg, frames = euroc_stream()
    results, fe_calls = [], []
    if which == "wired":
        fcfg.device_pipeline = fcfg.device_tracks = True
        mp = fe_mod.MultiImageProcessor(1, lane_configs=[fcfg])
        ms = sched_mod.MultiMSCKF(1, config=filter_config(), device_map=True, device_keyframes=True)
        fe, ctx = mp.fe, ms.ctx
        for imu, msg in frames:
            for m in imu:
                mp.imu_callback(0, m)
                ms.imu_callback(0, m)
            del fe.calls[:]
            feats = mp.stereo_callbacks({0: msg}, arrays=True)
            assert isinstance(feats[0], FeatureArrays)
            fe_calls.append(list(fe.calls))
            results.append(ms.feature_callbacks(feats)[0])
        launches = {"frontend": dict(mp.launches), "filter": dict(ms.launches)}
    else:
        vio = vio_mod.StereoVIO(filter_config(), fcfg, handoff=which)
        fe, ctx = vio.multi.frontend.fe, vio.multi.filters.ctx
        for imu, msg in frames:
            for m in imu:
                vio.imu_callback(m)
            del fe.calls[:]
            results.append(vio.stereo_callback(msg))
            fe_calls.append(list(fe.calls))
        launches = vio.launches
        vio.close()
        vio.close()                                   # twice is harmless
    _runs[which] = dict(results=results, sent=ctx.sent, map=ctx.map_get(0), fe_calls=fe_calls,
                        map_calls=list(ctx.map_calls), launches=launches, tracks=fe.tables[0])
    return _runs[which]


def same_results(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), k
        if x is None:
            continue
        assert x.timestamp == y.timestamp
        for p, q in ((x.pose, y.pose), (x.cam0_pose, y.cam0_pose)):
            assert np.asarray(p._vio_R__).tobytes() == np.asarray(q._vio_R__).tobytes(), k
            assert np.asarray(p._vio_t__).tobytes() == np.asarray(q._vio_t__).tobytes(), k
        assert np.asarray(x.velocity).tobytes() == np.asarray(y.velocity).tobytes(), k


def test_the_stream_reaches_every_request_kind(monkeypatch):
    w = run(monkeypatch, "wired")
    kinds = [r[0] for r in w["sent"]]
    assert sum(r is not None for r in w["results"]) == 11 and all(r is None for r in w["results"][:19])
    assert kinds.count("upd") == 7 and kinds.count("tri") == 4 and kinds.count("prune") == 4
    assert w["launches"]["filter"]["map_keyframe_select"] == 4
    assert w["map_calls"] == ["map_add_lost"] * 11
    assert len(w["map"][0]) > 0


@pytest.mark.parametrize("handoff", ["host", "device"])
def test_stereo_vio_equals_the_hand_wired_composition(monkeypatch, handoff):
    w, v = run(monkeypatch, "wired"), run(monkeypatch, handoff)
    same_results(v["results"], w["results"])
    assert [r[0] for r in v["sent"]] == [r[0] for r in w["sent"]]
    for k, (ra, rb) in enumerate(zip(v["sent"], w["sent"])):
        for x, y in zip(ra[1:], rb[1:]):
            np.testing.assert_array_equal(x, y, err_msg="request %d (%s)" % (k, ra[0]))
    for x, y in zip(v["map"], w["map"]):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(v["tracks"], w["tracks"]):
        np.testing.assert_array_equal(x, y)
    assert v["launches"]["filter"].get("map_update") == w["launches"]["filter"].get("map_update") > 0
    if handoff == "host":
        assert v["fe_calls"] == w["fe_calls"] and v["map_calls"] == w["map_calls"]
        assert v["launches"] == w["launches"]
        return
    # "device": the first frame publishes on the host and writes its message; a tracked frame is two calls
    assert v["fe_calls"][0] == w["fe_calls"][0] + ["tracks_msg_put"]
    assert w["fe_calls"][1] == ["upload_many", "tracks_step"]
    assert all(c == ["upload_many", "tracks_step_msg"] for c in v["fe_calls"][1:])
    # and the filter never takes a message from the host (before gravity it takes none at all)
    assert v["map_calls"] == ["map_add_lost_tracks"] * 11
    assert "map_add_lost" not in v["launches"]["filter"] and v["launches"]["filter"]["map_add_lost_tracks"] == 11
    assert v["launches"]["frontend"]["tracks_msg_put"] == 1


def test_a_track_message_needs_the_device_map(monkeypatch):
    stand_ins(monkeypatch)
    fe = vr.VioOracleFrontend(32, 32, nslot=3)
    msg = TrackMessage(0.0, fe, 0, 0)
    with pytest.raises(TypeError, match="device_map"):
        MSCKF().feature_callback(msg)
    with pytest.raises(TypeError, match="device_map"):
        sched_mod.MultiMSCKF(2).feature_callbacks({1: msg})
    assert MSCKF(device_map=True).feature_callback(msg) is None          # before gravity: as any message
    assert sched_mod._ORDER["map_add_lost_tracks"] == sched_mod._ORDER["map_add_lost"]
    assert msckf_amd.TrackMessage is TrackMessage and TrackMessage._fields == ("timestamp", "frontend", "lane", "n")
    with pytest.raises(ValueError, match="device_tracks"):
        fe_mod.MultiImageProcessor(1).stereo_callbacks({}, handoff=True)


def test_constructor_rules(monkeypatch):
    stand_ins(monkeypatch)
    made, closed = [], []

    class Counting(vr.VioOracleFrontend):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

        def close(self):
            closed.append(self)
    monkeypatch.setattr(fe_mod, "Frontend", Counting)
    bad = msckf_amd.FilterConfig()
    bad.optimization.translation_threshold = 0.2
    with pytest.raises(ValueError, match="translation_threshold"):       # the filters' rule; the front-end is closed
        vio_mod.StereoVIO(bad)
    assert len(made) == 1 and closed == made
    with pytest.raises(ValueError, match="lane 1.*translation_threshold"):
        vio_mod.MultiStereoVIO(2, lane_filter_configs=[msckf_amd.FilterConfig(), bad])
    assert len(made) == 2 and closed == made
    with pytest.raises(ValueError, match="lane 1.*grid_min_feature_num"):   # the front-end's rule, before any context
        vio_mod.MultiStereoVIO(2, lane_frontend_configs=[fe_mod.FrontendConfig(),
                                                         fe_mod.FrontendConfig(grid_min_feature_num=2)])
    with pytest.raises(ValueError, match="2 lane configs for 3 lanes"):
        vio_mod.MultiStereoVIO(3, lane_filter_configs=[msckf_amd.FilterConfig()] * 2)
    with pytest.raises(ValueError, match="handoff"):
        vio_mod.MultiStereoVIO(2, handoff="pinned")
    assert len(made) == 3 and closed == made
    with vio_mod.MultiStereoVIO(3, map_capacity=64, device_keyframes=False) as vio:
        assert len(vio) == 3 and vio.handoff == "device" and vio.filters.ctx.map_cap == 64
        assert vio.frontend.device_tracks and all(ip.config.device_pipeline for ip in vio.frontend.lanes)
        assert all(ln.device_map and not ln.device_keyframes for ln in vio.filters.lanes)
        assert set(vio.launches) == {"frontend", "filter"}
        assert len(vio.tracks(2)[0]) == 0
    assert closed == made and len(made) == 4
    one = vio_mod.StereoVIO(handoff="host")
    assert one.handoff == "host" and one.filter.device_keyframes and one.stareo_callback == one.stereo_callback
    assert sched_mod.MultiStereoVIO is vio_mod.MultiStereoVIO is msckf_amd.MultiStereoVIO
    assert sched_mod.StereoVIO is vio_mod.StereoVIO is msckf_amd.StereoVIO


def header_symbols(header, pattern):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src, sorted(set(re.findall(r"\b(%s)\s*\(" % pattern, src)))


def test_handoff_exports_and_binding():
    """include/msckf_handoff.h is exported by the same library and typed one to
    one by the binding (its own table; the other headers keep their symbols)."""
    decl, syms = header_symbols("msckf_handoff.h", r"(?:mfe|msckf)_[a-z_]+")
    assert syms == ["mfe_tracks_msg_get", "mfe_tracks_msg_put", "mfe_tracks_step_msg", "msckf_map_add_lost_tracks"]
    assert sorted(_lib.HANDOFF_EXPORTED) == syms
    assert not set(syms) & (set(_lib.TRACKS_EXPORTED) | set(_lib.MAP_EXPORTED) | set(_lib.EXPORTED))
    for name, (_, args) in _lib.HANDOFF_SIGS.items():                  # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    # the step's message form takes mfe_tracks_step's arguments without ids_out and uv_out
    assert len(_lib.HANDOFF_SIGS["mfe_tracks_step_msg"][1]) == len(_lib.FRONTEND_TRACKS_SIGS["mfe_tracks_step"][1]) - 2
    for method in ("tracks_msg_put", "tracks_msg_get"):
        assert callable(getattr(fe_mod.Frontend, method))
    assert callable(_lib.Context.map_add_lost_tracks)
    lib = ctypes.CDLL(_lib.LIB_PATH)                                   # the suite runs on a built tree
    for s in syms:
        assert hasattr(lib, s), s
