"""mfe_upload_many_eq / mfe_download (include/msckf_equalize.h) on the device
against tests/equalize_ref.py.

  * Level 0 after an equalised upload is the reference's image byte for byte
    (np.array_equal on uint8, no tolerance): hist and clahe at clip 0, 2 and 40,
    on 752 x 480 (tiles divide it; the 16-byte scatter path of the plain
    upload), 150 x 110 (padded histograms, px % 16 != 0) and 33 x 17 at tiles
    8 x 8 (5 x 3-pixel tiles, the clip's floor of 1), 16 x 16 and 1 x 1; on a
    uniform random image, the contrast-6 texture (few bins), a constant and a
    two-level image and a random image with one constant tile.  The 20 images of
    a shape go up in ONE call, modes mixed.
  * Plumbing: a "none" upload downloads as its input; the pyramid is built
    after the equalisation; one call of mixed modes leaves each slot as its
    single upload does and other slots alone.
  * Every rejected argument returns -1 with a message naming it, the slot
    unchanged.
  * End to end, 3 lanes (none, hist, clahe) at 150 x 110 on contrast-6 streams:
    every lane publishes, bit for bit, what an all-"none" processor publishes
    when fed the images equalised by the reference on the host -- with the
    tracks on the host and on the device, and through MultiStereoVIO."""
import numpy as np
import pytest

import msckf_amd
import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from msckf_amd.scheduler import MultiStereoVIO
from frontend_ref_scenes import StereoMsg, ImgMsg
import frontend_synth as fs
import frontend_lanes_ref as lr
import equalize_ref as er

pytestmark = pytest.mark.gpu

MODES = [("hist", 0.0), ("clahe", 0.0), ("clahe", 2.0), ("clahe", 40.0)]
SHAPES = [(752, 480, (8, 8)), (150, 110, (8, 8)), (33, 17, (8, 8)), (33, 17, (16, 16)), (33, 17, (1, 1))]


def make_images(W, H, tiles):
    """The five images of a shape, by name."""
    rng = np.random.default_rng(W * 1000 + H + tiles[0])
    rand = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ext = er.pad101(rand, tiles)
    tw, th = ext.shape[1] // tiles[0], ext.shape[0] // tiles[1]
    i, j = min(1, tiles[0] - 1), min(1, tiles[1] - 1)
    one_tile = rng.integers(0, 256, (H, W)).astype(np.uint8)
    one_tile[j * th:(j + 1) * th, i * tw:(i + 1) * tw] = 200
    return {"random": rand,
            "texture6": fs.render(fs.texture_fn(3, W=W, H=H, contrast=6.0), W, H),
            "constant": np.full((H, W), 77, np.uint8),
            "two_level": np.where(rng.random((H, W)) < 0.3, 50, 200).astype(np.uint8),
            "constant_tile": one_tile}


@pytest.mark.parametrize("W,H,tiles", SHAPES, ids=["%dx%d_t%d" % (w, h, t[0]) for w, h, t in SHAPES])
def test_level0_is_the_reference_bit_for_bit(W, H, tiles):
    images = make_images(W, H, tiles)
    assert int(images["texture6"].max()) - int(images["texture6"].min()) <= 20
    cases = [(name, mode, clip) for name in images for mode, clip in MODES]
    fe = fe_mod.Frontend(W, H, nslot=len(cases), max_level=1, max_points=16)
    try:
        fe.upload_many(list(range(len(cases))), np.stack([images[c[0]] for c in cases]),
                       ([c[1] for c in cases], [c[2] for c in cases], tiles))
        bad = []
        for slot, (name, mode, clip) in enumerate(cases):
            ref = er.equalize(images[name], mode, clip, tiles)
            got = fe.download(slot)
            assert got.shape == ref.shape and got.dtype == np.uint8
            if not np.array_equal(got, ref):
                bad.append((name, mode, clip, int((got != ref).sum())))
        assert not bad, bad
    finally:
        fe.close()


def level_shapes(W, H, max_level):
    out = [(H, W)]
    for _ in range(max_level):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def slot_levels(fe, slot, max_level):
    return [fe.download(slot, l) for l in range(max_level + 1)]


def test_plumbing_none_pyramid_and_mixed_call():
    W, H, L, tiles = 150, 110, 3, (8, 8)
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(4)] + \
        [fs.render(fs.texture_fn(3, W=W, H=H, contrast=6.0), W, H)]
    modes, clips = ["none", "hist", "clahe", "clahe", "hist"], [0.0, 0.0, 40.0, 2.0, 0.0]
    fe = fe_mod.Frontend(W, H, nslot=12, max_level=L, max_points=16)
    try:
        # a "none" upload is its input, on every path
        fe.upload(0, imgs[0])
        plain = slot_levels(fe, 0, L)
        assert [p.shape for p in plain] == level_shapes(W, H, L) and np.array_equal(plain[0], imgs[0])
        fe.upload(1, imgs[0], ("none", 40.0, tiles))
        for a, b in zip(slot_levels(fe, 1, L), plain):
            assert np.array_equal(a, b)
        # the pyramid is built after the equalisation: device against device
        for k in range(1, 5):
            fe.upload(2, imgs[k], (modes[k], clips[k], tiles))
            eq = slot_levels(fe, 2, L)
            fe.upload(3, eq[0])
            for l, (a, b) in enumerate(zip(eq, slot_levels(fe, 3, L))):
                assert np.array_equal(a, b), (k, l)
            assert not np.array_equal(eq[0], imgs[k])
        # one call of five images: each slot as its single upload leaves it, the sixth untouched
        fe.upload(9, imgs[1])
        before = slot_levels(fe, 9, L)
        singles = []
        for k in range(5):
            fe.upload(10, imgs[k], (modes[k], clips[k], tiles))
            singles.append(slot_levels(fe, 10, L))
        fe.upload_many([4, 5, 6, 7, 8], np.stack(imgs), (modes, clips, tiles))
        for k in range(5):
            for l, (a, b) in enumerate(zip(slot_levels(fe, 4 + k, L), singles[k])):
                assert np.array_equal(a, b), (k, l)
        for a, b in zip(slot_levels(fe, 9, L), before):
            assert np.array_equal(a, b)
        with pytest.raises(_lib.MsckfError, match="level"):
            fe.download(0, L + 1)
        with pytest.raises(_lib.MsckfError, match="slot"):
            fe.download(12)
    finally:
        fe.close()


def test_rejected_arguments_leave_the_slot_unchanged():
    rng = np.random.default_rng(6)
    for (W, H), calls in (
            ((40, 24), [(([7], [40.0], (8, 8)), "mode"), ((["clahe"], [40.0], (0, 8)), "tiles_x"),
                        ((["clahe"], [40.0], (17, 8)), "tiles_x"), ((["hist"], [40.0], (8, 0)), "tiles_y"),
                        ((["hist"], [40.0], (8, 17)), "tiles_y"), ((["clahe"], [float("nan")], (8, 8)), "clip_limit"),
                        ((["none"], [0.0], (-1, 8)), "tiles_x"), (([-1], [0.0], (8, 8)), "mode")]),
            ((12, 10), [((["clahe"], [40.0], (16, 8)), "tiles_x"), ((["clahe"], [40.0], (8, 16)), "tiles_y")])):
        img, other = (rng.integers(0, 256, (H, W)).astype(np.uint8) for _ in range(2))
        fe = fe_mod.Frontend(W, H, nslot=2, max_level=1, max_points=16)
        try:
            fe.upload(0, img)
            before = slot_levels(fe, 0, 1)
            for eq, name in calls:
                with pytest.raises(_lib.MsckfError, match=r"%s.*\(rc=-1\)" % name):
                    fe.upload_many([0], other[None], eq)
                for a, b in zip(slot_levels(fe, 0, 1), before):
                    assert np.array_equal(a, b), (eq, name)
            # a NaN clip limit of an image that is not CLAHE is not read
            fe.upload_many([0], other[None], (["hist"], [float("nan")], (8, 8)))
            assert np.array_equal(fe.download(0), er.equalize_hist(other))
        finally:
            fe.close()


# ------------------------------------------------------------------ end to end --
W2, H2, N_FRAMES = 150, 110, 5
LANE_MODES = ["none", "hist", "clahe"]
_e2e = {}


def lane_config(i, **kw):
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11 - 0.01 * i
    K = np.array([80.0, 80.0, W2 / 2, H2 / 2])
    return fe_mod.FrontendConfig(
        T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_intrinsics=K, cam1_intrinsics=K,
        cam0_distortion_coeffs=np.zeros(4), cam1_distortion_coeffs=np.zeros(4),
        cam0_resolution=np.array([W2, H2]), cam1_resolution=np.array([W2, H2]), grid_row=2, grid_col=2,
        pyramid_levels=1, device_pipeline=True, **kw)


def e2e_streams():
    """(raw streams, the same with lane i's images equalised by the reference in LANE_MODES[i]), rendered once."""
    if "streams" not in _e2e:
        raw, host = [], []
        for i, mode in enumerate(LANE_MODES):
            fr = lr.stream_frames(fs.texture_fn(3, W=W2, H=H2, contrast=6.0), W2, H2, N_FRAMES,
                                  (1.0 + 0.25 * i, -0.5), (0.0, 0.0, 0.0), 4.0)
            raw.append(fr)
            eq = lambda im: er.equalize(im, mode, 40.0, (8, 8))
            host.append([(imu, StereoMsg(m.vio_timestamp__, ImgMsg(m.vio_timestamp__, eq(m.cam0_msg.image)),
                                         ImgMsg(m.vio_timestamp__, eq(m.cam1_msg.image)))) for imu, m in fr])
        _e2e["streams"] = (raw, host)
    return _e2e["streams"]


def run_frontend(device_tracks, equalised_on_device):
    raw, host = e2e_streams()
    cfgs = [lane_config(i, device_tracks=device_tracks, equalize=m if equalised_on_device else "none")
            for i, m in enumerate(LANE_MODES)]
    mp = fe_mod.MultiImageProcessor(3, lane_configs=cfgs)
    per_step = []
    try:
        got = lr.run_lanes(mp, raw if equalised_on_device else host,
                           on_step=lambda step, lanes: per_step.append(dict(mp.launches)))
    finally:
        mp.close()
    return got, per_step


@pytest.mark.parametrize("device_tracks", [False, True], ids=["host_tracks", "device_tracks"])
def test_lanes_publish_what_host_equalised_images_publish(device_tracks):
    got, launches = run_frontend(device_tracks, True)
    ref, ref_launches = run_frontend(device_tracks, False)
    for i, (lane, rlane) in enumerate(zip(got, ref)):
        assert len(lane) == len(rlane) == N_FRAMES
        for k, ((ids, uv), (rids, ruv)) in enumerate(zip(lane, rlane)):
            assert ids.tobytes() == rids.tobytes() and uv.tobytes() == ruv.tobytes(), (LANE_MODES[i], k)
    counts = [[len(ids) for ids, _ in lane] for lane in got]
    assert counts[0] == [0] * N_FRAMES                      # the fixed threshold finds nothing in 120..136
    assert all(c > 0 for lane in counts[1:] for c in lane), counts
    assert launches == ref_launches                         # per step, the device calls of an all-"none" run
    assert launches[-1]["upload"] == N_FRAMES
    if device_tracks:
        assert launches[-1]["tracks_step"] == N_FRAMES - 1
    _e2e["counts_%d" % device_tracks] = counts


def test_multi_stereo_vio_takes_the_switch_through_frontend_config():
    raw, _ = e2e_streams()
    if "counts_1" not in _e2e:
        _e2e["counts_1"] = [[len(ids) for ids, _ in lane] for lane in run_frontend(True, True)[0]]
    cfgs = [lane_config(i, equalize=m) for i, m in enumerate(LANE_MODES)]
    counts = [[] for _ in LANE_MODES]
    with MultiStereoVIO(3, filter_config=msckf_amd.FilterConfig(), lane_frontend_configs=cfgs) as vio:
        assert [ip.config.equalize for ip in vio.frontend.lanes] == LANE_MODES
        inner = vio.frontend.stereo_callbacks

        def counting(msgs, **kw):
            out = inner(msgs, **kw)
            for i, m in out.items():
                counts[i].append(m.n)
            return out
        vio.frontend.stereo_callbacks = counting
        vio.run(raw)
        assert vio.launches["frontend"]["upload"] == N_FRAMES
        assert vio.launches["frontend"]["tracks_step"] == N_FRAMES - 1
    assert counts == _e2e["counts_1"]
