"""CPU checks of the keyframe choice on the device (include/msckf_keyframes.h):
  * its numpy restatement tests/keyframe_ref.py equals the host's
    MSCKF._find_redundant_cam_states (pinned to the reference by
    tests/test_host_logic.py) on every generated case, as generated and with the
    poses rounded through float32;
  * the case set itself holds what the device test relies on: every outcome,
    every to_quaternion branch, both sides of the rate threshold, 4 cam states
    and candidates in the second mask word, quaternions off unit norm, and the
    margins that make the decisions exact;
  * the header against its binding table and the built library;
  * the constructor rules of device_keyframes."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import msckf_amd.scheduler as sched_mod
from conftest import golden
from msckf_amd import _lib, synth
from msckf_amd.geometry import to_quaternion, to_rotation
from msckf_amd.msckf import MSCKF
from msckf_amd.replay import FeatureStream, replay
import feature_map_ref as fr
import keyframe_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_slots(cams, rate):
    """MSCKF._find_redundant_cam_states on a bare instance, as slots."""
    flt = MSCKF.__new__(MSCKF)
    flt.cam_ids = list(range(100, 100 + 3 * len(cams), 3))
    flt.tracking_rate = rate
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # no case may reach arccos outside [-1, 1]
        rm = flt._find_redundant_cam_states(np.asarray(cams, float))
    return [flt.cam_ids.index(c) for c in rm]


@pytest.mark.parametrize("f32", [False, True])
def test_restatement_equals_the_host_method(f32):
    n_checked = 0
    for case in kr.cases():
        c = kr.rounded(case) if f32 else case
        got = kr.choice(c["cams"], c["rate"])
        assert got.slots.tolist() == host_slots(c["cams"], c["rate"]), case["name"]
        assert got.slots[0] < got.slots[1]
        n_checked += 1
    assert n_checked == len(kr.cases()) >= 4 * len(kr._SPECS)


def test_restatement_pieces_equal_geometry():
    """The pieces against geometry.py.  Both sides evaluate the same formulas in another order: an entry (at most
    2 in magnitude) comes out of fewer than 16 roundings of 2**-53 relative each."""
    tol = 16 * np.finfo(float).eps
    for case in kr.cases()[::5]:
        for q in case["cams"][-4:, 0:4]:
            np.testing.assert_allclose(kr.rotation(q), to_rotation(q), rtol=0, atol=tol)
        M = kr.rotation(case["cams"][-3, 0:4]) @ kr.rotation(case["cams"][-4, 0:4]).T
        u, _ = kr.quaternion(M)
        np.testing.assert_allclose(u / np.linalg.norm(u), to_quaternion(M), rtol=0, atol=tol)


def test_case_set_properties():
    cases = kr.cases()
    for rnd in (False, True):
        cs = [kr.rounded(c) if rnd else c for c in cases]
        ch = [kr.choice(c["cams"], c["rate"]) for c in cs]
        # margins: a condition on the inputs, not a tolerance
        for c, r in zip(cs, ch):
            assert (np.abs(r.ang - kr.ROT_THR) >= kr.MARGIN).all(), c["name"]
            assert (np.abs(r.dist - kr.TRANS_THR) >= kr.MARGIN).all(), c["name"]
        # outcomes, at every size
        for n in kr.SIZES:
            assert {r.outcome for c, r in zip(cs, ch) if c["n"] == n} == set(kr.OUTCOMES), n
        # the slots of each outcome are what its name says
        for c, r in zip(cs, ch):
            n = c["n"]
            want = {"both_newest": [n - 3, n - 2], "oldest_second": [0, n - 2], "oldest_first": [0, n - 3],
                    "two_oldest": [0, 1]}[r.outcome]
            assert r.slots.tolist() == want, c["name"]
        # all four to_quaternion branches
        assert {b for r in ch for b in r.branch} == {0, 1, 2, 3}
        # the rate threshold: exactly 0.5 is not above it, the next double is
        half = [(c, r) for c, r in zip(cs, ch) if c["rate"] == 0.5]
        above = [(c, r) for c, r in zip(cs, ch) if c["rate"] == np.nextafter(0.5, 1.0)]
        assert half and above
        for c, r in half:
            assert r.outcome == "two_oldest" and (r.ang < kr.ROT_THR).all() and (r.dist < kr.TRANS_THR).all()
        for c, r in above:
            assert r.outcome == "both_newest"
        assert any(np.isnan(c["rate"]) and r.outcome == "two_oldest" for c, r in zip(cs, ch))
        # ang and dist decide on their own, close to their thresholds
        assert any(0 < kr.ROT_THR - r.ang.max() < 1e-4 and r.outcome == "both_newest" for r in ch)
        assert any(0 < r.ang[0] - kr.ROT_THR < 1e-4 and r.outcome == "oldest_second" for r in ch)
        assert any(0 < kr.TRANS_THR - r.dist.max() < 1e-4 and r.outcome == "both_newest" for r in ch)
        assert any(0 < r.dist[1] - kr.TRANS_THR < 1e-4 and r.outcome == "oldest_first" for r in ch)
    # window sizes: the smallest, and candidates whose slots lie in the second mask word
    assert {c["n"] for c in cases} == set(kr.SIZES) and min(kr.SIZES) == 4
    assert any(c["n"] - 3 >= 64 for c in cases)
    # quaternions off unit norm, by a common and by a per-record factor, one of them negative
    norms = [np.linalg.norm(c["cams"][:, 0:4], axis=1) for c in cases]
    assert any(np.abs(nm - 1).max() > 0.1 and np.ptp(nm) < 1e-12 for nm in norms)
    assert any(np.ptp(nm) > 0.1 for nm in norms)
    assert any(np.abs(nm - 1).max() < 1e-12 for nm in norms)
    # the float32 set is another set: its poses differ, its decisions do not
    assert any((kr.rounded(c)["cams"] != c["cams"]).any() for c in cases)
    for c in cases:
        assert kr.choice(kr.rounded(c)["cams"], c["rate"]).outcome == kr.choice(c["cams"], c["rate"]).outcome
    # groups: one case per size, in SIZES' order
    for g in kr.groups():
        assert [c["n"] for c in g] == list(kr.SIZES)


def test_fewer_than_four_cam_states():
    with pytest.raises(ValueError):
        kr.choice(np.zeros((3, 11)), 0.9)


def header_symbols(header, prefix):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z_]+)\s*\(" % prefix, src)))


def test_keyframe_exports_and_binding():
    syms = header_symbols("msckf_keyframes.h", "msckf_")
    assert syms == ["msckf_keyframe_select"]
    assert sorted(_lib.KEYFRAME_EXPORTED) == syms
    assert not set(syms) & (set(_lib.EXPORTED) | set(_lib.MAP_EXPORTED))   # the other headers keep their sets
    assert (_lib.KEYFRAME_ROT_THR, _lib.KEYFRAME_TRANS_THR, _lib.KEYFRAME_RATE_THR) == (0.2618, 0.4, 0.5)
    assert (kr.ROT_THR, kr.TRANS_THR, kr.RATE_THR) == (0.2618, 0.4, 0.5)
    src = open(os.path.join(ROOT, "include", "msckf_keyframes.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, (_, args) in _lib.KEYFRAME_SIGS.items():       # as many typed arguments as declared
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        assert len(args) == params.count(",") + 1, name
    assert callable(_lib.Context.keyframe_select)
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmsckf_hip.so not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), s


def test_device_keyframes_needs_device_map(monkeypatch):
    monkeypatch.setattr(_lib, "Context", fr.RecordingContext)
    with pytest.raises(ValueError, match="device_map"):
        MSCKF(device_keyframes=True)
    with pytest.raises(ValueError, match="device_map"):
        sched_mod.MultiMSCKF(2, device_keyframes=True)
    flt = MSCKF(device_map=True, device_keyframes=True)
    assert flt.device_map and flt.device_keyframes
    assert not MSCKF(device_map=True).device_keyframes and not MSCKF().device_keyframes
    assert "map_keyframe_select" in sched_mod._ORDER
    assert sched_mod._ORDER["map_keyframe_select"] == sched_mod._ORDER["map_prune_select"]


class KeyframeContext(fr.RecordingContext):
    """The stand-in with msckf_keyframe_select: the restated choice on its cam
    poses, then its prune select."""
    outcomes = None

    def keyframe_select(self, filters, rates):
        out = []
        for f, rate in zip(filters, rates):
            ch = kr.choice(self._cams(f), rate)
            if self.outcomes is not None:
                self.outcomes.append(ch.outcome)
            (iid, info), = self.map_prune_select([f], [0, 2], ch.slots)
            out.append((ch.slots, iid, info))
        return out


@pytest.mark.parametrize("which", [0, 1])
def test_filter_with_device_keyframes_equals_host_choice(monkeypatch, which):
    """MSCKF(device_map=True, device_keyframes=True) sends down the same batches
    and prune slots as MSCKF(device_map=True) and ends with the same logs, map
    and cam ids; the frame asks for one ``states`` read fewer on a prune frame."""
    g = golden("sequence_s1")
    st = [FeatureStream.from_synthetic(synth.make_sequence(int(g["n_frames"]), int(g["seed"]))),
          FeatureStream.from_synthetic(synth.make_sequence(90, 7))][which]
    monkeypatch.setattr(_lib, "Context", KeyframeContext)
    runs, outcomes = [], []
    for kw in ({"device_keyframes": True}, {}):
        flt = MSCKF(device_map=True, **kw)
        flt.ctx.outcomes = outcomes if kw else None
        kinds = []
        serve = flt._serve
        monkeypatch.setattr(flt, "_serve", lambda req, serve=serve, kinds=kinds: (kinds.append(req[0]), serve(req))[1])
        replay(flt, st)
        runs.append((flt, kinds))
    (a, ka), (b, kb) = runs
    assert [r[0] for r in a.ctx.sent] == [r[0] for r in b.ctx.sent]
    for x, y in zip(a.ctx.sent, b.ctx.sent):
        for u, v in zip(x[1:], y[1:]):
            np.testing.assert_array_equal(u, v)
    assert a.gate_log == b.gate_log and len(a.gate_log) > 100
    assert a.gamma_log == b.gamma_log and a.shape_log == b.shape_log
    assert a.cam_ids == b.cam_ids
    for x, y in zip(a.ctx.map_get(0), b.ctx.map_get(0)):
        np.testing.assert_array_equal(x, y)
    n_sel = ka.count("map_keyframe_select")
    assert n_sel > 10 and "map_prune_select" not in ka and "map_keyframe_select" not in kb
    assert kb.count("map_prune_select") == n_sel == ka.count("map_prune_commit")
    assert ka.count("states") == kb.count("states") - n_sel
    assert len(set(outcomes)) >= 2, set(outcomes)
