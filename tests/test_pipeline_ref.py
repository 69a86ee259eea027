"""CPU checks around the device pipeline (include/msckf_pipeline.h):
  * the reference tests/frontend_pipeline_ref.py under
    ImageProcessor(device_pipeline=True) publishes, on both scenes of
    tests/golden/frontend_ref.npz, the ids of the recorded reference frames and
    their coordinates to 1e-12 -- the bar of tests/test_frontend_ref.py, against
    the reference's own ImageProcessor: the switch changes nothing observable;
  * the device calls counted on a stand-in: one stereo_match is one call with
    the switch on and six composed; one add_new_features is one fast_grid call
    plus the stereo match, composed one fast call plus six;
  * the new header against the binding table and the built library (the ABI
    check of tests/test_abi.py for msckf_pipeline.h; msckf_frontend.h keeps its
    8 symbols);
  * the reference's own selection order and mask on small constructed cases."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from conftest import golden
from frontend_ref_scenes import SCENES, scene_config, run_scene, reference_frames
import frontend_synth as fs
import frontend_pipeline_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", SCENES)
def test_device_pipeline_reference_vs_recorded_frames(name, monkeypatch):
    g = golden("frontend_ref")
    monkeypatch.setattr(fe_mod, "Frontend", pr.OracleFrontend)
    cfg = scene_config(g, name)
    cfg.device_pipeline = True
    ip = fe_mod.ImageProcessor(cfg)
    got = run_scene(ip, g, name)
    for k, ((ids, uv), (rids, ruv)) in enumerate(zip(got, reference_frames(g, name))):
        np.testing.assert_array_equal(ids, rids, err_msg="frame %d" % k)
        np.testing.assert_allclose(uv, ruv, rtol=0, atol=1e-12, err_msg="frame %d" % k)
    assert len(got) == int(g[name + "_frames"]) and len(got[-1][0]) >= 50
    # the switch was on: lk is the temporal tracking, undistort the publish, fast the first frame
    assert set(ip.fe.calls) == {"fast", "lk", "stereo_match", "fast_grid", "undistort"}
    assert ip.fe.calls.count("fast") == 1 and ip.fe.calls.count("lk") == len(got) - 1


def _one_frame_processor(monkeypatch, device_pipeline):
    """An ImageProcessor on the counting stand-in with one uploaded stereo
    pair (a textured 96 x 64 scene, cam1 seeing it 4 px to the left)."""
    monkeypatch.setattr(fe_mod, "Frontend", pr.OracleFrontend)
    W, H = 96, 64
    K = np.array([80.0, 80.0, 48.0, 32.0])
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    cfg = fe_mod.FrontendConfig(T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_intrinsics=K, cam1_intrinsics=K,
                                cam0_distortion_coeffs=np.zeros(4), cam1_distortion_coeffs=np.zeros(4),
                                cam0_resolution=np.array([W, H]), cam1_resolution=np.array([W, H]),
                                grid_row=2, grid_col=2, pyramid_levels=1, device_pipeline=device_pipeline)
    ip = fe_mod.ImageProcessor(cfg)
    f = fs.texture_fn(3, W=W, H=H)
    img, im1 = fs.render(f, W, H), fs.render(f, W, H, -4.0, 0.0)
    ip.cam0_curr_img_msg = SimpleNamespace(image=img, vio_timestamp__=0.0)
    ip.cam1_curr_img_msg = SimpleNamespace(image=im1, vio_timestamp__=0.0)
    ip.create_image_pyramids()
    return ip


def test_call_counts(monkeypatch):
    pts = [(30.0, 20.0), (50.5, 40.25), (70.0, 33.0)]
    on = _one_frame_processor(monkeypatch, True)
    on.stereo_match(pts)
    assert on.fe.calls == ["stereo_match"]
    del on.fe.calls[:]
    on.add_new_features()
    assert on.fe.calls == ["fast_grid", "stereo_match"]

    off = _one_frame_processor(monkeypatch, False)
    off.stereo_match(pts)
    assert off.fe.calls == ["undistort", "distort", "lk", "lk", "undistort", "undistort"]
    del off.fe.calls[:]
    off.add_new_features()
    assert off.fe.calls == ["fast", "undistort", "distort", "lk", "lk", "undistort", "undistort"]
    # and both ways found the same features
    key = lambda ip: [(f.id, f.cam0_point, f.cam1_point, f.response) for c in ip.curr_features for f in c]
    assert key(on) == key(off) and len(key(on)) > 0

    # one whole tracked frame (the second stareo_callback, RANSAC on), uploads included: the
    # switch-off list is the one the plain methods made before the frame logic was written once
    composed = ["undistort", "distort", "lk", "lk", "undistort", "undistort"]
    want = {False: ["upload", "upload", "lk"] + composed + ["ransac", "fast"] + composed + ["undistort", "undistort"],
            True: ["upload", "upload", "lk", "stereo_match", "ransac", "fast_grid", "stereo_match", "undistort",
                   "undistort"]}
    msgs = {}
    for switch in (False, True):
        ip = _one_frame_processor(monkeypatch, switch)
        calls = ip.fe.calls
        ip.config.ransac_enabled = True
        ip.ransac_fn = lambda sets, *a: (calls.append("ransac"), [(np.ones(len(s[0]), bool), None) for s in sets])[1]
        ip.fe.upload = lambda slot, image, up=ip.fe.upload: (calls.append("upload"), up(slot, image))[1]
        f = fs.texture_fn(3, W=96, H=64)
        for k in range(2):
            img, im1 = fs.render(f, 96, 64, 1.0 * k, 0.0), fs.render(f, 96, 64, 1.0 * k - 4.0, 0.0)
            del calls[:]
            msgs[switch, k] = ip.stareo_callback(SimpleNamespace(
                cam0_msg=SimpleNamespace(image=img, vio_timestamp__=0.05 * k),
                cam1_msg=SimpleNamespace(image=im1, vio_timestamp__=0.05 * k)))
        assert calls == want[switch], switch
        assert ip.num_features["after_ransac"] == ip.num_features["before_tracking"] > 0
    assert msgs[False, 1] == msgs[True, 1] and len(msgs[True, 1].vio_features) > 0


def test_switch_is_off_by_default():
    assert fe_mod.FrontendConfig().device_pipeline is False
    ref = SimpleNamespace(_vio_grid_row__=3)
    cfg = fe_mod.FrontendConfig.from_reference(ref)
    assert cfg.grid_row == 3 and cfg.device_pipeline is False


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_pipeline_exports_and_binding():
    """include/msckf_pipeline.h is exported by the same library and typed one
    to one by the binding (its own table, as msckf_ransac.h has)."""
    syms = header_symbols("msckf_pipeline.h", "mfe_")
    assert syms == ["mfe_fast_grid", "mfe_stereo_match"] and sorted(_lib.FRONTEND_PIPELINE_EXPORTED) == syms
    assert not set(syms) & (set(_lib.FRONTEND_EXPORTED) | set(_lib.FRONTEND_RANSAC_EXPORTED))
    src = open(os.path.join(ROOT, "include", "msckf_pipeline.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MFE_GRID_[A-Z_]+) (\d+)", src)}
    assert consts == {"MFE_GRID_MAX_K": _lib.GRID_MAX_K, "MFE_GRID_MAX_CELLS": _lib.GRID_MAX_CELLS}
    assert (pr.GRID_MAX_K, pr.GRID_MAX_CELLS) == (_lib.GRID_MAX_K, _lib.GRID_MAX_CELLS)
    assert len(_lib.FRONTEND_PIPELINE_SIGS["mfe_stereo_match"][1]) == 21
    assert len(_lib.FRONTEND_PIPELINE_SIGS["mfe_fast_grid"][1]) == 13
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s


def test_reference_mask_is_the_reference_slice():
    """The header's mask rule equals the reference's numpy slice for every
    point inside the image (negative slice starts included)."""
    W, H = 40, 30
    rng = np.random.default_rng(0)
    occ = np.concatenate([rng.uniform([0, 0], [W, H], (40, 2)),
                          [[0, 0], [2.9, 10], [10, 2.9], [3, 3], [W - 1, H - 1], [W - 4, H - 4], [W - 0.5, 5]]])
    occ = occ.astype(np.float32)
    want = np.ones((H, W), np.uint8)
    for p in occ:
        x, y = map(int, p)
        want[y - 3:y + 4, x - 3:x + 4] = 0
    np.testing.assert_array_equal(pr.occupancy_mask(W, H, occ), want)
    assert pr.occupancy_mask(W, H, np.array([[np.nan, 5.0]])).all()


def dots(W, H, spots):
    """Dark image with single bright pixels: each is a FAST corner that
    survives the non-max suppression, its response set by its brightness."""
    img = np.full((H, W), 40, np.uint8)
    for x, y, v in spots:
        img[y, x] = v
    return img


def test_reference_selection_order():
    """Two equal-response corners in one cell with room for one: the earlier
    in raster order stays; the output is grouped by cell."""
    spots = [(30, 20, 200), (10, 8, 150), (40, 8, 200), (12, 25, 200), (35, 26, 120), (20, 12, 90)]
    img = dots(48, 32, spots)
    xy_all, r_all = pr.fo.fast_detect(img, 15)
    assert len(xy_all) == len(spots) and (r_all == r_all.max()).sum() == 3      # ties exist
    xy, resp, cnt, n = pr.fast_grid(img, 15, np.zeros((0, 2)), 1, 1, 1)
    assert n == len(spots) and cnt.tolist() == [n]
    np.testing.assert_array_equal(xy, [[40, 8]])                                # first of the ties in raster order
    xy, resp, cnt, n = pr.fast_grid(img, 15, np.zeros((0, 2)), 1, 1, 4)
    np.testing.assert_array_equal(xy, [[40, 8], [30, 20], [12, 25], [10, 8]])
    xy, resp, cnt, n = pr.fast_grid(img, 15, np.zeros((0, 2)), 2, 2, 16)
    assert cnt.sum() == n == len(xy) and cnt.tolist() == [2, 1, 1, 2]            # k above every cell: all kept
    np.testing.assert_array_equal(xy, [[10, 8], [20, 12], [40, 8], [12, 25], [30, 20], [35, 26]])
    assert pr.fast_grid(img, 15, np.zeros((0, 2)), 2, 2, 16, max_kp=n - 1)[0] is None
    # an occupied point on a corner removes it
    assert pr.fast_grid(img, 15, np.array([[42.5, 10.0]]), 1, 1, 1)[0].tolist() == [[30, 20]]
