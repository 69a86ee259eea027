"""CPU checks around the two-point RANSAC (include/msckf_ransac.h):
  * the numpy reference (tests/ransac_ref.py) recovers planted outliers on
    generated data, for both camera models, and reaches its pure-rotation,
    n_raw < 3 and no-qualifying-hypothesis branches;
  * the lowest-h tie rule on a constructed tie;
  * the new header against the binding table and the built library (the ABI
    check of tests/test_abi.py for msckf_ransac.h);
  * the feature is opt-in: FrontendConfig().ransac_enabled is False, and the
    ImageProcessor bookkeeping around a replaced ransac_fn."""
import ctypes
import os
import re

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def draws_for(n_sets, n_hyp, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(n_sets, n_hyp, 2), dtype=np.uint32)


@pytest.mark.parametrize("model", [0, 1])
def test_reference_recovers_planted_outliers(model):
    g = rr.synth_correspondences(120, seed=3 + model, model=model, outlier_share=0.25, far=4)
    mk, info, mg, _ = rr.ransac_set(*g["set"], 3.0, 17, draws_for(1, 17, 1)[0])
    assert info[0] == 0 and info[1] == 116          # the 4 far matches fall to the pre-filter
    np.testing.assert_array_equal(mk, ~(g["outlier"] | g["far"]))
    assert info[6] == mk.sum() and 0 <= info[5] < 17
    assert info[10] < 1.0 * info[3]                  # mean refit residual below one pixel
    assert mg["threshold"] > 0 and np.isfinite(mg["cond"])


def test_reference_pure_rotation_branch():
    """No translation: after the rotation compensation the matches coincide up
    to the noise, mean_dist < unit (2 gross outliers in 80 do not lift the
    mean above a pixel), and only the outliers go."""
    g = rr.synth_correspondences(80, seed=5, t=(0.0, 0.0, 0.0), rvec=(0.002, -0.003, 0.001), noise=0.1,
                                 outlier_share=0.025)
    mk, info, _, _ = rr.ransac_set(*g["set"], 3.0, 7, draws_for(1, 7, 0)[0])
    assert info[0] == 1 and info[5] == -1 and np.isnan(info[7:11]).all()
    np.testing.assert_array_equal(mk, ~g["outlier"])
    assert info[6] == mk.sum()


@pytest.mark.parametrize("n", [0, 1, 2])
def test_reference_too_few_points(n):
    g = rr.synth_correspondences(n, seed=1, outlier_share=0.0)
    mk, info, _, _ = rr.ransac_set(*g["set"], 3.0, 7, draws_for(1, 7, 0)[0])
    assert info[0] == 2 and info[1] == n and not mk.any() and len(mk) == n
    if n == 0:
        np.testing.assert_array_equal(info, rr.empty_info())


def test_reference_no_qualifying_hypothesis():
    """Matches without a common motion: no two-point model gathers 20 %."""
    rng = np.random.default_rng(7)
    prev = rng.uniform([100, 80], [650, 400], (60, 2))
    curr = prev + rng.uniform(8, 30, (60, 1)) * (lambda a: np.stack([np.cos(a), np.sin(a)], 1))(rng.uniform(0, 7, 60))
    mk, info, _, detail = rr.ransac_set(prev, curr, np.eye(3), rr.EUROC_K, 0, rr.RADTAN, 0.5, 7, draws_for(1, 7, 2)[0])
    assert info[0] == 3 and info[5] == -1 and info[6] == 0 and not mk.any()
    assert max(detail["count"]) < 0.2 * 60


def test_reference_lowest_h_wins_tie():
    s, draws = rr.tie_case()
    mk, info, mg, detail = rr.ransac_set(*s, 0.5, 3, draws[0])
    assert detail["count"] == [4, 4, 4] and info[0] == 0
    assert info[5] == 0 and info[6] == 4
    np.testing.assert_array_equal(mk, np.arange(8) < 4)
    # the other order of the same draws: still the first of the tied hypotheses
    mk2, info2, _, _ = rr.ransac_set(*s, 0.5, 3, draws[0][[1, 0, 2]])
    assert info2[5] == 0
    np.testing.assert_array_equal(mk2, np.arange(8) >= 4)
    assert mg["threshold"] >= 1e-6 and mg["cond"] <= 1e4


# ------------------------------------------------------------------ ABI ----
def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_ransac_exports_and_binding():
    """include/msckf_ransac.h is exported by the same library and typed one to
    one by the binding (its own table: msckf_frontend.h keeps its 8 symbols)."""
    syms = header_symbols("msckf_ransac.h", "mfe_")
    assert syms == ["mfe_two_point_ransac"] and sorted(_lib.FRONTEND_RANSAC_EXPORTED) == syms
    assert not set(syms) & set(_lib.FRONTEND_EXPORTED)
    src = open(os.path.join(ROOT, "include", "msckf_ransac.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (MFE_RANSAC_[A-Z_]+) (\d+)", src)}
    assert consts == {"MFE_RANSAC_INFO_LEN": _lib.RANSAC_INFO_LEN,
                      "MFE_RANSAC_MAX_SET_POINTS": _lib.RANSAC_MAX_SET_POINTS,
                      "MFE_RANSAC_MAX_HYP": _lib.RANSAC_MAX_HYP}
    assert consts["MFE_RANSAC_INFO_LEN"] == rr.INFO_LEN == 12
    assert consts["MFE_RANSAC_MAX_SET_POINTS"] >= 4096 and consts["MFE_RANSAC_MAX_HYP"] >= 64
    assert len(_lib.FRONTEND_RANSAC_SIGS["mfe_two_point_ransac"][1]) == 14
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s
    assert _lib.load_library().mfe_two_point_ransac.restype is ctypes.c_int


# ------------------------------------------------------------- opt-in ----
def test_ransac_is_opt_in():
    cfg = fe_mod.FrontendConfig()
    assert cfg.ransac_enabled is False
    assert cfg.ransac_success_probability == 0.99 and cfg.ransac_seed == 0 and cfg.ransac_threshold == 3
    assert fe_mod.ransac_hypotheses(0.99) == 7


def test_image_processor_ransac_bookkeeping(monkeypatch):
    """ImageProcessor.two_point_ransac: one call with the cam0 and the cam1
    set, each with its own camera, and a feature kept only if both sets keep
    it (device context replaced by a stub: host logic only)."""
    class NoDevice:
        def __init__(self, *a, **k):
            pass
    monkeypatch.setattr(fe_mod, "Frontend", NoDevice)
    calls = []

    def fake(sets, inlier_error, n_hyp, draws):
        calls.append((sets, inlier_error, n_hyp, draws))
        info = fe_mod.RansacInfo.from_row(rr.empty_info())
        return [(np.array([1, 1, 0, 0], bool), info), (np.array([1, 0, 1, 0], bool), info)]
    cfg = fe_mod.FrontendConfig(ransac_enabled=True, cam1_distortion_model="equidistant", ransac_threshold=2.5)
    ip = fe_mod.ImageProcessor(cfg, ransac_fn=fake)
    p = np.arange(8.0).reshape(4, 2)
    R0, R1 = np.eye(3), np.diag([1.0, -1.0, -1.0])
    keep = ip.two_point_ransac(p, p + 1, p + 2, p + 3, R0, R1, "draws")
    np.testing.assert_array_equal(keep, [True, False, False, False])
    (s0, s1), err, n_hyp, draws = calls[0]
    assert len(calls) == 1 and err == 2.5 and n_hyp == 7 and draws == "draws"
    np.testing.assert_array_equal(s0[0], p)
    np.testing.assert_array_equal(s1[1], p + 3)
    assert s0[2] is R0 and s1[2] is R1 and s0[4] == fe_mod.RADTAN and s1[4] == fe_mod.EQUIDISTANT
    np.testing.assert_array_equal(s1[3], cfg.cam1_intrinsics)
    np.testing.assert_array_equal(s0[5], cfg.cam0_distortion_coeffs)
