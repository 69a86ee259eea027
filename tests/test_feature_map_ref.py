"""CPU checks of the feature map kept on the device (include/msckf_map.h), on
the stand-in tests/feature_map_ref.py whose map calls are the numpy reference:
  * MSCKF(device_map=True) sends down, for every triangulate and update
    request, the same (obs_off, obs_cam, obs_z, NaN pattern of p_w, chi2,
    row_cap) as MSCKF(), and the same prune slots; it ends with the same logs
    and the same map -- on the golden sequence_s1 stream and the scheduler
    test's second and third streams; every branch of the reference is taken;
  * tuple and array messages give the same result on the host-map path;
  * the constructor rules;
  * the header against its binding table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd
import msckf_amd.msckf as msckf_mod
import msckf_amd.scheduler as sched_mod
from msckf_amd import _lib, synth
from msckf_amd.msckf import MSCKF, FeatureArrays
from msckf_amd.replay import FeatureStream, replay
from conftest import golden
import feature_map_ref as fr
import feature_map_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def late_start(st, k0):
    a = int(st.frame_off[k0])
    return FeatureStream(st.imu, st.frame_t[k0:], st.frame_off[k0:] - a, st.feat_id[a:], st.feat_z[a:], st.gt)


def streams():
    g = golden("sequence_s1")
    return [FeatureStream.from_synthetic(synth.make_sequence(int(g["n_frames"]), int(g["seed"]))),
            FeatureStream.from_synthetic(synth.make_sequence(90, 7)),
            late_start(FeatureStream.from_synthetic(synth.make_sequence(140, 11)), 7),
            # 400 features per frame: the map passes 256 rows (tests/test_gpu_feature_map.py's big_stream)
            FeatureStream.from_synthetic(synth.make_sequence(30, 3, max_features=400, n_landmarks=2000))]


STREAMS = None


def get_streams():
    global STREAMS
    if STREAMS is None:
        STREAMS = streams()
    return STREAMS


def array_events(st):
    out = []
    for kind, m in st.events():
        if kind == 1:
            fs = m.vio_features
            m = FeatureArrays(m.timestamp, np.array([f.id for f in fs], np.int64),
                              np.array([(f.u0, f.v0, f.u1, f.v1) for f in fs], float).reshape(-1, 4))
        out.append((kind, m))
    return out


def run(monkeypatch, st, events=None, **kw):
    monkeypatch.setattr(_lib, "Context", fr.RecordingContext)
    flt = MSCKF(**kw)
    replay(flt, st, events=events)
    return flt


def map_as_lists(flt):
    return [(fid, list(f.observations.items()), bool(f.is_initialized),
             np.asarray(f.position, float).tolist() if f.is_initialized else None)
            for fid, f in flt.map_server.items()]


def assert_same_sent(a, b):
    assert [r[0] for r in a] == [r[0] for r in b]
    for k, (ra, rb) in enumerate(zip(a, b)):
        for x, y in zip(ra[1:], rb[1:]):
            np.testing.assert_array_equal(x, y, err_msg="request %d (%s)" % (k, ra[0]))


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_device_map_sends_what_the_host_map_sends(monkeypatch, which):
    st = get_streams()[which]
    fr.COUNTERS.clear()
    host = run(monkeypatch, st)
    assert not fr.COUNTERS
    sizes, add_lost = [], fr.RecordingContext.map_add_lost

    def sized(self, filters, msg_off, ids, z):
        out = add_lost(self, filters, msg_off, ids, z)
        sizes.extend(len(self.tab[f]["ids"]) for f in filters)
        return out
    monkeypatch.setattr(fr.RecordingContext, "map_add_lost", sized)
    dev = run(monkeypatch, st, device_map=True)
    assert len(sizes) > 10
    if which == 3:            # the stream whose map no single 256-row pass of a map kernel covers
        assert max(sizes) > 256 and np.diff(st.frame_off).min() > 256, max(sizes)
    else:
        assert max(sizes) <= 256
    assert any(r[0] == "tri" for r in host.ctx.sent) and any(r[0] == "upd" for r in host.ctx.sent)
    assert_same_sent(host.ctx.sent, dev.ctx.sent)
    assert host.gate_log == dev.gate_log and len(host.gate_log) > 100
    assert host.gamma_log == dev.gamma_log
    assert host.shape_log == dev.shape_log and host.reset_log == dev.reset_log
    assert host.cam_ids == dev.cam_ids and host.tracking_rate == dev.tracking_rate
    assert map_as_lists(host) == map_as_lists(dev) and len(host.map_server) > 10
    for b in fr.BRANCHES:     # every branch of the reference was taken
        assert fr.COUNTERS[b] > 0, (b, dict(fr.COUNTERS))
    # the row-cap break and a failed fused triangulation occur in the lost updates
    assert any(r[0] == "upd" and r[6] == MSCKF.ROW_CAP and r[4].any() for r in dev.ctx.sent)


@pytest.mark.parametrize("cap,n", fc.BIG)
def test_the_big_map_cases_span_several_chunks(cap, n):
    """A condition on the inputs of tests/test_gpu_feature_map.py's cases above 256
    rows, from the reference's own outputs: see feature_map_cases."""
    tabs, msgs, ncams = fc.add_lost_tables(n, cap)
    name, ids, z = msgs[0][0]
    assert name == "mixed" and {m[0] for m in msgs[0]} >= {"mixed", "tracked"} and len(tabs[0]["ids"]) == n
    c = fc.assert_add_lost_spans_chunks(tabs[0], ids, z, ncams[0] - 1, cap)
    assert len(c["table"]) == -(-(n + sum(m[0] for m in c["message"])) // 256)
    for name, ids, z in msgs[0][1:]:
        assert len(ids) > 256
    assert (len(tabs[2]["ids"]) < 64) == (n in (513, 1023, 2047))
    for nent, nent_hi in fc.prune_conditions(n):
        if n >= 1023:             # prune_commit's entry loop runs more than once
            assert nent > 256 and nent_hi > 0, (n, nent, nent_hi)


def test_the_overflow_case_spans_several_chunks():
    t, ids, z = fc.overflow_case(1024)
    with pytest.raises(fr.MapError) as e:
        fr.add_lost(t, ids, z, 5, 1024)
    assert e.value.rc == -3 and "1025 rows" in str(e.value)
    c = fc.add_lost_chunks(t, ids[:-1], z[:-1], 5, 1024)
    assert len(c["message"]) == 3 and all(m[0] > 0 for m in c["message"]) and len(c["table"]) == 4


def test_array_messages_equal_tuple_messages(monkeypatch):
    st = get_streams()[1]
    for kw in ({}, {"device_map": True}):
        a = run(monkeypatch, st, **kw)
        b = run(monkeypatch, st, events=array_events(st), **kw)
        assert_same_sent(a.ctx.sent, b.ctx.sent)
        assert a.gate_log == b.gate_log and a.gamma_log == b.gamma_log and a.shape_log == b.shape_log
        assert map_as_lists(a) == map_as_lists(b)
    ar = st.frame_arrays(3)
    msg = st.frame_msg(3)
    assert isinstance(ar, FeatureArrays) and ar.timestamp == msg.timestamp
    assert ar.ids.tolist() == [f.id for f in msg.vio_features]
    np.testing.assert_array_equal(ar.uv, [(f.u0, f.v0, f.u1, f.v1) for f in msg.vio_features])
    ids, uv = msckf_mod.message_arrays(msg)
    np.testing.assert_array_equal(ids, ar.ids)
    np.testing.assert_array_equal(uv, ar.uv)


def test_online_reset_clears_the_device_map(monkeypatch):
    st = get_streams()[1]
    cfg = msckf_amd.FilterConfig()
    cfg.position_std_threshold = 1e-9     # the stand-in's variances are 0: force the reset by hand below
    monkeypatch.setattr(fr.RecordingContext, "readback",
                        lambda self, filters, want_cams=True, cov=None: (
                            np.array([self.imu[f] for f in filters]), [self._cams(f) for f in filters],
                            np.full((len(filters), cov[1]), 1.0 if self.next_serial[0] == 30 else 0.0)
                            if cov else None))
    host, dev = run(monkeypatch, st, config=cfg), run(monkeypatch, st, config=cfg, device_map=True)
    assert host.reset_log == dev.reset_log and len(dev.reset_log) == 1
    assert host.gate_log == dev.gate_log and map_as_lists(host) == map_as_lists(dev)


def test_constructor_rules(monkeypatch):
    monkeypatch.setattr(_lib, "Context", fr.RecordingContext)
    cfg = msckf_amd.FilterConfig()
    cfg.optimization.translation_threshold = 0.2
    with pytest.raises(ValueError, match="translation_threshold"):
        MSCKF(cfg, device_map=True)
    MSCKF(cfg)                                               # the host map keeps check_motion
    with pytest.raises(ValueError, match="lane 1.*translation_threshold"):
        sched_mod.MultiMSCKF(2, lane_configs=[msckf_amd.FilterConfig(), cfg], device_map=True)
    flt = MSCKF(device_map=True, map_capacity=300)
    assert flt.device_map and flt.ctx.map_cap == 300 and len(flt.map_server) == 0
    assert not MSCKF().device_map and isinstance(MSCKF().map_server, dict)
    ms = sched_mod.MultiMSCKF(3, device_map=True, map_capacity=64)
    assert ms.ctx.map_cap == 64 and all(ln.device_map for ln in ms.lanes)
    assert not any(ln.device_map for ln in sched_mod.MultiMSCKF(2).lanes)
    assert isinstance(flt, MSCKF) and type(MSCKF()) is MSCKF

    class Mine(MSCKF):                                       # a user's subclass keeps its overrides
        def publish(self, time):
            return "mine"
    mine = Mine(device_map=True)
    assert isinstance(mine, Mine) and mine.publish(0.0) == "mine" and len(mine.map_server) == 0
    assert type(Mine()) is Mine and type(mine) is type(Mine(device_map=True))
    with pytest.raises(AttributeError):
        flt.map_server = {}


def test_reference_error_rules():
    t = fr.empty(8)
    with pytest.raises(fr.MapError) as e:
        fr.add_lost(t, [1, 2, 1], np.zeros((3, 4)), 0, 16)
    assert e.value.rc == -1
    with pytest.raises(fr.MapError) as e:
        fr.add_lost(t, np.arange(17), np.zeros((17, 4)), 0, 16)
    assert e.value.rc == -3


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_map_exports_and_binding():
    syms = header_symbols("msckf_map.h", "msckf_map_")
    assert syms == sorted(["msckf_map_create", "msckf_map_clear", "msckf_map_put", "msckf_map_get",
                           "msckf_map_add_lost", "msckf_map_prune_select", "msckf_map_load",
                           "msckf_map_prune_commit"])
    assert sorted(_lib.MAP_EXPORTED) == syms
    assert not set(syms) & set(_lib.EXPORTED)                # msckf_hip.h keeps its own set
    src = open(os.path.join(ROOT, "include", "msckf_map.h")).read()
    assert int(re.search(r"#define MSCKF_MAP_INFO (\d+)", src).group(1)) == _lib.MAP_INFO
    for name, val in (("LOST", _lib.MAP_LOAD_LOST), ("PRUNE_TRI", _lib.MAP_LOAD_PRUNE_TRI),
                      ("PRUNE_UPDATE", _lib.MAP_LOAD_PRUNE_UPDATE)):
        assert int(re.search(r"#define MSCKF_MAP_LOAD_%s (\d+)" % name, src).group(1)) == val
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (_, args) in _lib.MAP_SIGS.items():            # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s


@pytest.mark.parametrize("tracks", [True, False])
def test_frontend_array_messages(monkeypatch, tracks):
    """MultiImageProcessor.stereo_callbacks(msgs, arrays=True) returns the default
    messages' ids and coordinates as FeatureArrays, with the tracks on the device
    (straight from the step's arrays) and on the host (converted once); lane 1
    starts a frame late, so a first frame and a tracked frame share a step.
    Two lanes on a textured 96 x 64 scene each, three frames (the scenes of
    tests/test_tracks_ref.py)."""
    import msckf_amd.frontend as fe_mod
    import frontend_lanes_ref as lr
    import frontend_synth as fs
    import frontend_tracks_ref as tr
    monkeypatch.setattr(fe_mod, "Frontend", tr.TracksOracleFrontend)
    W, H = 96, 64
    K = np.array([80.0, 80.0, 48.0, 32.0])

    def lanes():
        cfgs, sts = [], []
        for i in range(2):
            Ti1 = np.eye(4)
            Ti1[0, 3] = -0.11 - 0.01 * i
            cfgs.append(fe_mod.FrontendConfig(
                T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_intrinsics=K, cam1_intrinsics=K,
                cam0_distortion_coeffs=np.zeros(4), cam1_distortion_coeffs=np.zeros(4),
                cam0_resolution=np.array([W, H]), cam1_resolution=np.array([W, H]), grid_row=2, grid_col=2,
                pyramid_levels=1, device_pipeline=True, device_tracks=tracks))
            sts.append(lr.stream_frames(fs.texture_fn(3 + i, W=W, H=H), W, H, 3, (1.0 + 0.25 * i, -0.5),
                                        (0.0, 0.0, 0.0), 4.0))
        return fe_mod.MultiImageProcessor(2, lane_configs=cfgs), sts
    mp, sts = lanes()
    want = lr.run_lanes(mp, sts, start=[0, 1])
    mp, sts = lanes()
    default = mp.stereo_callbacks
    seen = []

    def as_arrays(msgs):
        out = default(msgs, arrays=True)
        seen.extend(out.values())
        return {i: fe_mod.FeatureMsg(m.timestamp, [fe_mod.FeatureMeasurement(k, *u)
                                                   for k, u in zip(m.ids.tolist(), m.uv.tolist())])
                for i, m in out.items()}
    monkeypatch.setattr(mp, "stereo_callbacks", as_arrays)
    got = lr.run_lanes(mp, sts, start=[0, 1])
    assert len(seen) == 6 and all(isinstance(m, FeatureArrays) and m.ids.dtype == np.int64 and
                                  m.uv.dtype == np.float64 and m.uv.shape == (len(m.ids), 4) for m in seen)
    for a, b in zip(got, want):
        assert len(a) == len(b) == 3 and len(a[-1][0]) > 0
        for (ids, uv), (wids, wuv) in zip(a, b):
            np.testing.assert_array_equal(ids, wids)
            np.testing.assert_array_equal(uv, wuv)
