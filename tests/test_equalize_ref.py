"""CPU checks of the equalisation reference tests/equalize_ref.py (the
restatement of include/msckf_equalize.h that tests/test_gpu_equalize.py pins
the device against) and of the host side of FrontendConfig.equalize:
  * equalize_hist and clahe on cases derivable by hand;
  * clahe's padded-histogram path against the divisible one;
  * a contrast-6 scene (grey values 120..136) publishes no feature as it is and
    12, 20, 20, 20 features per frame once equalised, through the CPU stand-in;
  * the defaults leave the upload call as it was; bad fields and lanes whose
    tile grids differ are rejected by the constructors;
  * the new header against its binding table and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
import frontend_synth as fs
import frontend_lanes_ref as lr
import equalize_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_equalize_hist_by_hand():
    rng = np.random.default_rng(0)
    perm = rng.permutation(256).astype(np.uint8).reshape(16, 16)
    # every bin holds one pixel: lut[k] = sat(k * 255 / 255)
    np.testing.assert_array_equal(er.equalize_hist(perm), perm)
    const = np.full((17, 33), 77, np.uint8)
    np.testing.assert_array_equal(er.equalize_hist(const), const)
    two = np.where(rng.random((17, 33)) < 0.3, 50, 200).astype(np.uint8)
    assert 0 < (two == 50).sum() < two.size
    np.testing.assert_array_equal(er.equalize_hist(two), np.where(two == 50, 0, 255))


def test_clahe_constant_image_by_hand():
    """96 x 64, tiles 8 x 8: tile 12 x 8, area 96, clip = int(40 * 96 / 256) = 15.
    The one bin of 96 is cut to 15, 81 excess: 81 // 256 = 0 to every bin,
    residual 81, step 3, one count each to bins 0, 3, ..., 240.  Up to 77 those
    are bins 0..75: 26 counts, plus bin 77's 15 = 41; 41 * 255 / 96 = 108.9."""
    img = np.full((64, 96), 77, np.uint8)
    out = er.clahe(img, 40.0, (8, 8))
    assert out.shape == img.shape and (out == 109).all()
    assert (er.clahe(img, 0.0, (8, 8)) == 255).all()     # no clipping: the whole tile at or below 77


def test_clahe_padded_path_equals_divisible_path():
    rng = np.random.default_rng(1)
    W, H = 150, 110
    img = rng.integers(0, 256, (H, W)).astype(np.uint8)
    ext = er.pad101(img, (8, 8))
    assert ext.shape == (112, 152)
    for clip in (0.0, 2.0, 40.0):
        np.testing.assert_array_equal(er.clahe(ext, clip, (8, 8))[:H, :W], er.clahe(img, clip, (8, 8)))
    # both sides are padded as soon as one does not divide (clahe.cpp): a full extra tile column here
    assert er.pad101(np.zeros((110, 152), np.uint8), (8, 8)).shape == (112, 160)


def lane_config(W, H, **kw):
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    K = np.array([80.0, 80.0, W / 2, H / 2])
    return fe_mod.FrontendConfig(
        T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_intrinsics=K, cam1_intrinsics=K,
        cam0_distortion_coeffs=np.zeros(4), cam1_distortion_coeffs=np.zeros(4),
        cam0_resolution=np.array([W, H]), cam1_resolution=np.array([W, H]), grid_row=2, grid_col=2,
        pyramid_levels=1, device_pipeline=True, **kw)


def low_contrast_stream(W, H, n=4, contrast=6.0):
    return lr.stream_frames(fs.texture_fn(3, W=W, H=H, contrast=contrast), W, H, n, (1.0, -0.5), (0.0, 0.0, 0.0), 4.0)


def test_low_contrast_scene_publishes_only_when_equalised(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", er.EqualizingFrontend)
    W, H = 96, 64
    stream = low_contrast_stream(W, H)
    lo, hi = min(m.cam0_msg.image.min() for _, m in stream), max(m.cam0_msg.image.max() for _, m in stream)
    assert 118 <= lo and hi <= 138
    modes = ["none", "hist", "clahe"]
    mp = fe_mod.MultiImageProcessor(3, lane_configs=[lane_config(W, H, equalize=m) for m in modes])
    got = lr.run_lanes(mp, [stream] * 3)
    counts = [[len(ids) for ids, _ in lane] for lane in got]
    assert counts == [[0, 0, 0, 0], [12, 20, 20, 20], [12, 20, 20, 20]]
    assert mp.fe.upload_log == [1] * 4 and mp.launches["upload"] == 4      # one call per step, with the modes
    # the scene at its usual contrast publishes the same counts as it is
    mp = fe_mod.MultiImageProcessor(1, lane_configs=[lane_config(W, H)])
    got = lr.run_lanes(mp, [low_contrast_stream(W, H, contrast=110.0)])
    assert [len(ids) for ids, _ in got[0]] == [12, 20, 20, 20]
    # and a single ImageProcessor goes through Frontend.upload with the same argument
    ip = fe_mod.ImageProcessor(lane_config(W, H, equalize="clahe"))
    for imu, msg in stream[:2]:
        for m in imu:
            ip.imu_callback(m)
        out = ip.stareo_callback(msg)
    assert len(out.vio_features) == 20 and ip.fe.upload_log == []


def test_defaults_leave_the_upload_call_as_it_was(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", er.EqualizingFrontend)
    cfg = fe_mod.FrontendConfig()
    assert (cfg.equalize, cfg.clahe_clip_limit, tuple(cfg.clahe_tiles)) == ("none", 40.0, (8, 8))
    W, H = 96, 64
    mp = fe_mod.MultiImageProcessor(2, lane_configs=[lane_config(W, H), lane_config(W, H)])
    lr.run_lanes(mp, [low_contrast_stream(W, H, 3, 110.0)] * 2)
    assert mp.fe.upload_log == [0, 0, 0]       # upload_many(slots, images): its present two arguments
    assert all(next(ip._upload_steps())[0] == "upload" and len(next(ip._upload_steps())) == 2 for ip in mp.lanes)


def test_bad_equalisation_fields_are_rejected(monkeypatch):
    monkeypatch.setattr(fe_mod, "Frontend", er.EqualizingFrontend)
    W, H = 96, 64
    bad = [dict(equalize="CLAHE"), dict(equalize=None), dict(equalize=True), dict(clahe_tiles=(0, 8)),
           dict(clahe_tiles=(8, 17)), dict(clahe_tiles=8), dict(clahe_tiles=(8, 8, 8)), dict(clahe_tiles=(2.5, 8)),
           dict(clahe_clip_limit=float("nan")), dict(equalize="clahe", clahe_clip_limit=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError, match="equalize|clahe_tiles|clahe_clip_limit"):
            fe_mod.ImageProcessor(lane_config(W, H, **kw))
        with pytest.raises(ValueError, match="equalize|clahe_tiles|clahe_clip_limit"):
            fe_mod.MultiImageProcessor(2, lane_configs=[lane_config(W, H), lane_config(W, H, **kw)])
    with pytest.raises(ValueError, match="clahe_tiles"):      # more tiles than pixels on a side
        fe_mod.ImageProcessor(lane_config(12, 10, clahe_tiles=(16, 8)))
    with pytest.raises(ValueError, match="lane 1.*clahe_tiles"):
        fe_mod.MultiImageProcessor(2, lane_configs=[lane_config(W, H, equalize="clahe"),
                                                    lane_config(W, H, equalize="clahe", clahe_tiles=(4, 4))])
    mp = fe_mod.MultiImageProcessor(2, lane_configs=[lane_config(W, H, equalize="clahe", clahe_tiles=[4, 4]),
                                                    lane_config(W, H, equalize="hist", clahe_tiles=(4, 4),
                                                                clahe_clip_limit=2.0)])
    assert mp.lanes[0]._equalize == ("clahe", 40.0, (4, 4)) and mp.lanes[1]._equalize == ("hist", 2.0, (4, 4))


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_equalize_exports_and_binding():
    """include/msckf_equalize.h is exported by the same library and typed one
    to one by the binding (its own table)."""
    syms = header_symbols("msckf_equalize.h", "mfe_")
    assert syms == ["mfe_download", "mfe_download_deriv", "mfe_upload_many_eq"]
    assert sorted(_lib.EQUALIZE_EXPORTED) == syms
    assert not set(syms) & (set(_lib.FRONTEND_EXPORTED) | set(_lib.FRONTEND_LANES_EXPORTED) |
                            set(_lib.FRONTEND_PIPELINE_EXPORTED) | set(_lib.TRACKS_EXPORTED))
    src = open(os.path.join(ROOT, "include", "msckf_equalize.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MFE_EQ_[A-Z_]+) (\d+)", src)}
    assert consts == {"MFE_EQ_NONE": _lib.EQ_NONE, "MFE_EQ_HIST": _lib.EQ_HIST, "MFE_EQ_CLAHE": _lib.EQ_CLAHE,
                      "MFE_EQ_MAX_TILES": _lib.EQ_MAX_TILES}
    assert fe_mod.EQ_MODES == {"none": 0, "hist": 1, "clahe": 2} and er.MODES == {v: k for k, v in fe_mod.EQ_MODES.items()}
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (_, args) in _lib.EQUALIZE_SIGS.items():       # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
