"""msckf_amd.vio end to end on the device: MultiStereoVIO with both hand-offs,
and StereoVIO, against MultiImageProcessor(device_tracks, arrays=True) wired by
hand into MultiMSCKF(device_map, device_keyframes) on fresh contexts.

Two lanes: the ``rectified`` and the ``euroc`` scene of
tests/golden/frontend_ref.npz extended to 45 frames, max_cam_state_size = 6;
lane 1 starts two frames late, so a first-frame lane and a tracking lane share a
round.  In fp64 and in fp32.  No tolerance: every vio_result field, the final
maps, the track tables and next_id are compared bit for bit."""
import numpy as np
import pytest

import msckf_amd
import msckf_amd.frontend as fe_mod
from msckf_amd.scheduler import MultiMSCKF, MultiStereoVIO, StereoVIO
from conftest import golden
from frontend_ref_scenes import SCENES, scene_config
import frontend_synth as fs
import frontend_lanes_ref as lr

pytestmark = pytest.mark.gpu
N_FRAMES, START = 45, [0, 2]
_streams, _wired = None, {}


def filter_config():
    cfg = msckf_amd.FilterConfig()
    cfg.max_cam_state_size = 6
    return cfg


def scenes():
    """([front-end config per lane], [frames per lane]), rendered once."""
    global _streams
    if _streams is None:
        g = golden("frontend_ref")
        W, H = (int(v) for v in g["size"])
        cfgs, streams = [], []
        for name in SCENES:
            f = fs.texture_fn(int(g[name + "_seed"]), W=W, H=H)
            cfgs.append(scene_config(g, name))
            streams.append(lr.stream_frames(f, W, H, N_FRAMES, g[name + "_step"], g[name + "_gyro"],
                                            float(g[name + "_disparity"])))
        _streams = (cfgs, streams)
    return _streams


def steps(streams, start):
    for step in range(max(s + len(fr) for s, fr in zip(start, streams))):
        yield step, {i: fr[step - s] for i, (s, fr) in enumerate(zip(start, streams)) if 0 <= step - s < len(fr)}


def end_state(frontend, filters, results, launches):
    n = len(filters)
    return dict(results=results, launches=launches, maps=[filters.ctx.map_get(i) for i in range(n)],
                tracks=[frontend.tracks(i) for i in range(n)],
                next_id=[ip.next_feature_id for ip in frontend.lanes])


def wired(dtype):
    """The reference run, once per dtype."""
    key = np.dtype(dtype).name
    if key in _wired:
        return _wired[key]
    cfgs, streams = scenes()
    on = [fe_mod.FrontendConfig(**{**vars(c), "device_pipeline": True, "device_tracks": True}) for c in cfgs]
    mp = fe_mod.MultiImageProcessor(2, lane_configs=on)
    ms = MultiMSCKF(2, config=filter_config(), dtype=dtype, device_map=True, device_keyframes=True)
    try:
        results = [[] for _ in streams]
        for step, frames in steps(streams, START):
            for i, (imu, _) in frames.items():
                for m in imu:
                    mp.imu_callback(i, m)
                    ms.imu_callback(i, m)
            out = ms.feature_callbacks(mp.stereo_callbacks({i: fr[1] for i, fr in frames.items()}, arrays=True))
            for i, res in out.items():
                results[i].append(res)
        _wired[key] = end_state(mp, ms, results, {"frontend": dict(mp.launches), "filter": dict(ms.launches)})
    finally:
        mp.close()
        ms.close()
    return _wired[key]


def same_result(x, y, what):
    assert (x is None) == (y is None), what
    if x is None:
        return
    assert x.timestamp == y.timestamp, what
    for p, q in ((x.pose, y.pose), (x.cam0_pose, y.cam0_pose)):
        assert np.asarray(p._vio_R__).tobytes() == np.asarray(q._vio_R__).tobytes(), what
        assert np.asarray(p._vio_t__).tobytes() == np.asarray(q._vio_t__).tobytes(), what
    assert np.asarray(x.velocity).tobytes() == np.asarray(y.velocity).tobytes(), what


def same_arrays(a, b, what):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), what


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_reference_run_updates_and_prunes(dtype):
    w = wired(dtype)
    for lane in range(2):
        n = sum(r is not None for r in w["results"][lane])
        assert n > 0 and len(w["results"][lane]) == N_FRAMES
    f = w["launches"]["filter"]
    assert f["map_update"] > 0 and f["prune"] > 0 and f["map_keyframe_select"] > 0 and f["map_add_lost"] > 0
    assert all(len(m[0]) > 0 for m in w["maps"]) and all(len(t[0]) > 0 for t in w["tracks"])


@pytest.mark.parametrize("handoff", ["host", "device"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_stereo_vio_equals_the_hand_wired_composition(dtype, handoff):
    w = wired(dtype)
    cfgs, streams = scenes()
    per_step = []
    with MultiStereoVIO(2, filter_config=filter_config(), lane_frontend_configs=cfgs, dtype=dtype,
                        handoff=handoff) as vio:
        results = [[] for _ in streams]

        def on_step(step, out):
            per_step.append(sorted(out))
            for i, res in out.items():
                results[i].append(res)
        traj = vio.run(streams, start=START, on_step=on_step)
        got = end_state(vio.frontend, vio.filters, results, vio.launches)
        vio.close()                                   # twice (with the block's) is harmless
    assert per_step[0] == [0] and per_step[2] == [0, 1] and per_step[-1] == [1] and len(per_step) == N_FRAMES + 2
    for lane in range(2):
        assert len(got["results"][lane]) == len(w["results"][lane])
        for k, (x, y) in enumerate(zip(got["results"][lane], w["results"][lane])):
            same_result(x, y, "lane %d frame %d" % (lane, k))
        assert len(traj[lane]) == sum(r is not None for r in w["results"][lane])
        same_arrays(got["maps"][lane], w["maps"][lane], "map of lane %d" % lane)
        same_arrays(got["tracks"][lane], w["tracks"][lane], "tracks of lane %d" % lane)
    assert got["next_id"] == w["next_id"]
    f, wf = got["launches"]["filter"], w["launches"]["filter"]
    if handoff == "host":
        assert got["launches"] == w["launches"]
        return
    # one hand-off call per round for all lanes, none fed from the host
    assert "map_add_lost" not in f and f["map_add_lost_tracks"] == wf["map_add_lost"] > 0
    assert {k: v for k, v in f.items() if k != "map_add_lost_tracks"} == \
        {k: v for k, v in wf.items() if k != "map_add_lost"}
    fe_l, wfe = got["launches"]["frontend"], w["launches"]["frontend"]
    assert fe_l.pop("tracks_msg_put") == 2 and fe_l == wfe        # the two first frames write their messages


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stereo_vio_equals_lane_0(dtype):
    w = wired(dtype)
    cfgs, streams = scenes()
    with StereoVIO(filter_config(), cfgs[0], dtype=dtype) as vio:
        assert vio.handoff == "device"
        got = []
        for imu, msg in streams[0]:
            for m in imu:
                vio.imu_callback(m)
            got.append(vio.stareo_callback(msg))
        for k, (x, y) in enumerate(zip(got, w["results"][0])):
            same_result(x, y, "frame %d" % k)
        same_arrays(vio.tracks(), w["tracks"][0], "tracks")
        same_arrays(vio.filter.ctx.map_get(0), w["maps"][0], "map")
    vio.close()
