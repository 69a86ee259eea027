"""The numpy restatement of include/msckf_standstill.h (tests/standstill_ref.py)
checked on the CPU: the decision table, the quantile's index, the config, the
binding, and the cue's effect in a closed loop on the numpy oracle.
"""
import itertools

import numpy as np
import pytest

from msckf_amd import FilterConfig, VisionCue, ZuptConfig, chi2_threshold, synth
import standstill_ref as S
import zupt_ref as Z
from test_zupt_ref import N_MOVING, N_REST, STREAM

# The synthetic messages carry pix_sigma = 0.5 px of noise per coordinate, so between two
# frames at rest a feature moves by the difference of two draws: variance 0.5 px^2 per axis,
# d2 / 0.5 ~ chi^2(2), median 0.5 * 2 ln 2 = 0.69 px^2.  max_px = 2 px (4 px^2) is 2.8
# standard deviations of one axis, almost six times the median of ~100 tracks; min_tracks
# is VisionCue's default reasoning at the stream's ~150 features per frame.
CUE = dict(max_px=2.0, min_tracks=20)
FOCAL = 458.654


def test_decision_table():
    """{pd, not pd} x {gamma under / over} x {speed under / over} x {STILL,
    MOVING, UNKNOWN} x {VETO, EITHER} x {IMU, REJECT}, each cell against the
    header's two sentences written out by hand."""
    prm = ZuptConfig(chi2=5.0, max_speed=0.1)
    n = 0
    for pd, g_ok, s_ok, status, mode, unknown in itertools.product(
            (True, False), (True, False), (True, False), (S.STILL, S.MOVING, S.UNKNOWN), ("veto", "either"),
            ("imu", "reject")):
        cue = VisionCue(mode=mode, unknown=unknown, **CUE)
        gamma = (1.0 if g_ok else 9.0) if pd else np.nan
        speed = 0.05 if s_ok else 0.5
        got = S.decide(pd, gamma, speed, status, prm, cue)
        imu_ok = pd and g_ok and s_ok
        if status == S.UNKNOWN:
            want = imu_ok and unknown == "imu"          # both modes: today's gate, or nothing
        elif mode == "veto":
            want = imu_ok and status == S.STILL
        else:
            want = (pd and status == S.STILL) or imu_ok
        assert got == want, (pd, g_ok, s_ok, status, mode, unknown)
        assert not (got and not pd)                     # nothing is ever applied without a factor of S
        n += 1
    assert n == 96


def test_status():
    cue = VisionCue(max_px=1.5, min_tracks=3)
    assert S.cue_status(-1, np.float32(0.0), cue) == S.UNKNOWN          # no record
    assert S.cue_status(2, np.float32(0.0), cue) == S.UNKNOWN           # too few tracks
    assert S.cue_status(0, np.float32(np.nan), cue) == S.UNKNOWN        # the empty lane
    assert S.cue_status(3, np.float32(2.25), cue) == S.STILL            # d2 = max_px^2 is still
    assert S.cue_status(3, np.nextafter(np.float32(2.25), np.float32(3)), cue) == S.MOVING
    assert S.cue_status(3, np.float32(np.nan), cue) == S.MOVING


@pytest.mark.parametrize("n,q,k", [(1, 0, 0), (1, 0.5, 0), (1, 1, 0), (2, 0, 0), (2, 0.5, 0), (2, 1, 1),
                                   (3, 0, 0), (3, 0.5, 1), (3, 1, 2)])
def test_quantile_index(n, q, k):
    assert S.motion_k(n, q) == k
    d = np.arange(n, dtype=np.float32)[::-1].copy()
    prev = np.zeros((n, 2), np.float32)
    curr = np.stack([d, np.zeros(n, np.float32)], axis=1)
    got_n, got = S.motion_stat(prev, curr, q)
    assert got_n == n and got == np.float32(k) ** 2 and got.dtype == np.float32


def test_statistic_rounds_each_operation_once():
    """float32 throughout: a value where the fused or the double evaluation differs."""
    prev = np.array([[0.1, 0.2]], np.float32)
    curr = np.array([[1000.7, 3000.3]], np.float32)
    dx, dy = curr[0, 0] - prev[0, 0], curr[0, 1] - prev[0, 1]
    want = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
    assert S.motion_stat(prev, curr, 0.5) == (1, want)
    assert float(want) != float(dx) ** 2 + float(dy) ** 2
    n, v = S.motion_stat(np.zeros((0, 2)), np.zeros((0, 2)), 0.5)
    assert n == 0 and np.isnan(v)


def test_config_checks():
    assert ZuptConfig().vision is None
    c = VisionCue()
    assert c.quantile == 0.5 and c.mode == "veto" and c.unknown == "imu" and c.max_px > 0 and c.min_tracks >= 1
    p = VisionCue(max_px=1.5, min_tracks=7, mode="either", unknown="reject").params()
    assert (p.max_px, p.min_tracks, p.mode, p.unknown) == (1.5, 7, 1, 1)
    for bad in (dict(max_px=-1.0), dict(max_px=float("nan")), dict(quantile=1.5), dict(quantile=float("nan")),
                dict(min_tracks=0), dict(mode="both"), dict(unknown="skip")):
        with pytest.raises(ValueError):
            VisionCue(**bad)
    with pytest.raises(TypeError):
        ZuptConfig(vision="veto")


def test_abi_symbols_and_struct():
    """include/msckf_standstill.h's entry points are exported by the library and
    typed one to one by the binding, in a list of their own; msckf_zupt.h's list
    stays as it is."""
    import ctypes
    import os
    import re
    from msckf_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "msckf_standstill.h")).read(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+((?:mfe|msckf)_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S))
    assert sorted(decls) == sorted(_lib.STANDSTILL_EXPORTED) and len(decls) == 5
    assert not set(decls) & (set(_lib.ZUPT_EXPORTED) | set(_lib.EXPORTED) | set(_lib.TRACKS_EXPORTED) |
                             set(_lib.HANDOFF_EXPORTED))
    lib = _lib.load_library()
    for name, params in decls.items():
        assert getattr(lib, name).restype is ctypes.c_int
        assert len(_lib.STANDSTILL_SIGS[name][1]) == params.count(",") + 1, name
    assert ctypes.sizeof(_lib.MsckfZuptCueT) == 24   # a double and three int32, padded to 8
    for name, val in re.findall(r"#define MSCKF_CUE_(MOVING|STILL|UNKNOWN)\s+(\d+)", src):
        assert getattr(_lib, "CUE_" + name) == int(val) == getattr(S, name)
    for name, val in re.findall(r"#define MSCKF_CUE_MODE_([A-Z]+)\s+(\d+)", src):
        assert _lib.CUE_MODES[name.lower()] == int(val)
    for name, val in re.findall(r"#define MSCKF_CUE_UNKNOWN_([A-Z]+)\s+(\d+)", src):
        assert _lib.CUE_UNKNOWNS[name.lower()] == int(val)


# ------------------------------------------------------------ closed loops --
# A stream at rest whose filter starts with a velocity estimate 0.3 m/s off: three times
# ZuptConfig's max_speed.  1 s of gravity initialisation, then 40 published frames at rest.
REST = dict(n_frames=0, static_s=3.0, seed=0)
V_OFF = 0.3


@pytest.fixture(scope="module")
def rest_runs():
    seq = synth.make_sequence(**REST)
    cfg = FilterConfig(velocity=np.array([V_OFF, 0.0, 0.0]))
    out = {}
    for name, zc, cue in (("plain", None, None), ("imu", ZuptConfig(), None),
                          ("either", ZuptConfig(), VisionCue(mode="either", **CUE)),
                          ("veto", ZuptConfig(), VisionCue(mode="veto", **CUE))):
        orc = S.OracleStandstill(cfg, chi2_threshold, zc, cue, focal=FOCAL)
        out[name] = (orc, Z.run_oracle(orc, seq))
    return out


def test_rest_with_a_wrong_velocity(rest_runs):
    """The filter's velocity starts 0.3 m/s off on a platform at rest, above
    max_speed = 0.1.  Measured with the oracle over the 40 published frames:

        run       applied    |p_end - p_start|
        plain     -          0.8128 m
        IMU-only  0 of 40    0.8128 m
        VETO      0 of 40    0.8128 m
        EITHER    40 of 40   0.0009 m

    The plain run's speed estimate stays above max_speed for the whole stream
    (the scenario's condition, checked on the plain run), so the IMU-only
    update never engages and VETO, which can only forbid, equals it.  EITHER
    applies at every frame at rest, the first published one included: the
    stream's messages during the second of gravity initialisation give that
    frame its previous message."""
    plain = rest_runs["plain"][1]
    n = len(plain)
    assert n == 40
    speed = np.linalg.norm(plain[:, 4:7], axis=1)
    assert speed[:10].min() > ZuptConfig().max_speed, speed[:10]        # the scenario, on the plain run
    logs = {k: rest_runs[k][0].zupt_log for k in ("imu", "either", "veto")}
    assert all(len(lg) == n for lg in logs.values())
    assert not any(e[1] for e in logs["imu"][:10])
    # the cue the stream's geometry gives: STILL at every published frame
    assert all(e[3] == S.STILL and e[4] >= CUE["min_tracks"] for e in logs["either"])
    assert all(e[1] for e in logs["either"])                            # EITHER applies at every frame at rest
    assert [e[1] for e in logs["veto"]] == [e[1] for e in logs["imu"]]
    np.testing.assert_array_equal(rest_runs["veto"][1], rest_runs["imu"][1])
    # the start: the filter's initial position, the origin, which the platform never leaves
    err = {k: float(np.linalg.norm(rest_runs[k][1][-1, 1:4])) for k in rest_runs}
    print("end errors", err, "applied", {k: sum(e[1] for e in lg) for k, lg in logs.items()})
    assert err["either"] < err["imu"]


def test_veto_is_the_imu_log_on_the_rest_and_motion_stream():
    """tests/test_zupt_ref.py's stream (31 frames at rest, 19 moving): no moving
    frame passes the IMU gate there, so VETO with the geometric cue has nothing
    to forbid and must give the IMU-only log frame for frame -- at rest the cue
    is STILL.  The synthetic
    IMU shows no false positive, so VETO's value is not demonstrated here."""
    seq = synth.make_sequence(**STREAM)
    imu = S.OracleStandstill(FilterConfig(), chi2_threshold, ZuptConfig(), None, focal=FOCAL)
    veto = S.OracleStandstill(FilterConfig(), chi2_threshold, ZuptConfig(), VisionCue(mode="veto", **CUE), focal=FOCAL)
    rec_imu, rec_veto = Z.run_oracle(imu, seq), Z.run_oracle(veto, seq)
    assert len(rec_imu) == N_REST + N_MOVING
    assert [e[:3] for e in veto.zupt_log] == [e[:3] for e in imu.zupt_log]
    np.testing.assert_array_equal(rec_veto, rec_imu)
    assert all(e[3] == S.STILL for e in veto.zupt_log[:N_REST])
    ref = Z.OracleZupt(FilterConfig(), chi2_threshold, ZuptConfig())     # and IMU-only is zupt_ref's filter
    np.testing.assert_array_equal(Z.run_oracle(ref, seq), rec_imu)
