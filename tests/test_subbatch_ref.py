"""CPU checks of the lane split (csrc/msckf_subbatch.h, built here with the host
compiler alone): the class lists load_features builds -- the gating lists of
msckf_gate_routes.h and the five segment classes, each ascending in feature
index -- are cut where lane 1's features begin, and each lane is handed its
part.  For random and edge batches the lanes' sub-lists must partition every
class list, stay ascending, and hold only features of the lane's own filters."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "visual-inertial-odometry-msckf-stereo_amd", "csrc")

# stdin: B, then B feature counts, then the track length M of every feature.
# stdout: "lanes <n>", "cut <first filter of lane 1>", then one line per (kind, list, lane):
# "<g|s> <list> <lane> <lane's first filter> <filter count> : <features ...>", and "full <g|s> <list> : <features ...>".
_DRIVER = r"""
#include <cstdio>
#include <vector>
#include "msckf_gate_routes.h"
#include "msckf_subbatch.h"
using namespace msckf;
static const int SEG[5] = {8, 16, 32, 64, 128};
static void dump(char kind, const std::vector<int>& flat, const std::vector<int>& off, int B, int nl, int f_cut) {
    const int n = (int)off.size() - 1;
    std::vector<int> cut(n), beg(n), end(n);
    subbatch_cut_lists(flat.data(), off.data(), n, f_cut, cut.data());
    for (int l = 0; l < n; ++l) {
        std::printf("full %c %d :", kind, l);
        for (int i = off[l]; i < off[l + 1]; ++i) std::printf(" %d", flat[i]);
        std::printf("\n");
    }
    for (int lane = 0; lane < nl; ++lane) {
        subbatch_lane_lists(off.data(), cut.data(), n, lane, nl, beg.data(), end.data());
        const int b0 = subbatch_first_filter(B, lane, nl), b1 = subbatch_first_filter(B, lane + 1, nl);
        for (int l = 0; l < n; ++l) {
            std::printf("%c %d %d %d %d :", kind, l, lane, b0, b1 - b0);
            for (int i = beg[l]; i < end[l]; ++i) std::printf(" %d", flat[i]);
            std::printf("\n");
        }
    }
}
int main() {
    int B = 0, forced = 0;
    if (std::scanf("%d %d", &B, &forced) != 2) return 1;
    std::vector<int> feat_off(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        int n = 0;
        if (std::scanf("%d", &n) != 1) return 1;
        feat_off[b + 1] = feat_off[b] + n;
    }
    const int nf = feat_off[B];
    std::vector<int> M(nf);
    for (int f = 0; f < nf; ++f)
        if (std::scanf("%d", &M[f]) != 1) return 1;
    // the lists as load_features builds them
    std::vector<int> gflat, goff(GATE_NLIST + 1), sflat, soff(6);
    for (int l = 0; l < GATE_NLIST; ++l) {
        goff[l] = (int)gflat.size();
        for (int f = 0; f < nf; ++f)
            if (gate_list_of(M[f]) == l) gflat.push_back(f);
    }
    goff[GATE_NLIST] = (int)gflat.size();
    for (int k = 0; k < 5; ++k) {
        soff[k] = (int)sflat.size();
        for (int f = 0; f < nf; ++f)
            if (M[f] <= SEG[k] && (k == 0 || M[f] > SEG[k - 1])) sflat.push_back(f);
    }
    soff[5] = (int)sflat.size();
    const int nl = subbatch_lanes(B, forced);
    std::printf("lanes %d\n", nl);
    std::printf("cut %d\n", subbatch_first_filter(B, 1, nl));
    const int f_cut = feat_off[subbatch_first_filter(B, 1, 2)];   // as load_features: the cut of a two-lane run
    dump('g', gflat, goff, B, nl, f_cut);
    dump('s', sflat, soff, B, nl, f_cut);
    return 0;
}
"""


def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for cxx in ("c++", "g++", os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "bin", "amdclang++")):
        path = shutil.which(cxx)
        if path:
            return path
    return None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler (c++, g++ or the ROCm clang++) to build msckf_subbatch.h with"
    d = tmp_path_factory.mktemp("subbatch")
    src, exe = d / "subbatch.cpp", d / "subbatch"
    src.write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _run(exe, counts, M, forced=2):
    counts, M = list(map(int, counts)), list(map(int, M))
    assert sum(counts) == len(M)
    text = " ".join(map(str, [len(counts), forced] + counts + M))
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    lanes, cut = int(out[0].split()[1]), int(out[1].split()[1])
    full, parts = {}, {}
    for ln in out[2:]:
        head, _, tail = ln.partition(":")
        feats = [int(x) for x in tail.split()]
        h = head.split()
        if h[0] == "full":
            full[(h[1], int(h[2]))] = feats
        else:
            parts[(h[0], int(h[1]), int(h[2]))] = (int(h[3]), int(h[4]), feats)
    return lanes, cut, full, parts


def _gate_list(M):
    return (-(-(3 * M + 4) // 16) - 1) if M <= 82 else 16


def _seg_class(M):
    return next(k for k, s in enumerate((8, 16, 32, 64, 128)) if M <= s)


def _check(exe, counts, M, forced=2):
    lanes, cut, full, parts = _run(exe, counts, M, forced)
    B = len(counts)
    feat_off = np.concatenate([[0], np.cumsum(counts)])
    filt = np.repeat(np.arange(B), counts)
    assert lanes == (2 if B >= 2 and forced == 2 else 1)
    assert cut == (B // 2 if lanes == 2 else B)          # lane 0 = [0, B / 2)
    # the lists themselves: every feature once per kind, in the list of its track length
    for kind, nlist, which in (("g", 17, _gate_list), ("s", 5, _seg_class)):
        seen = []
        for l in range(nlist):
            assert full[(kind, l)] == [f for f in range(len(M)) if which(M[f]) == l]
            seen += full[(kind, l)]
            cat = []
            for lane in range(lanes):
                b0, nb, feats = parts[(kind, l, lane)]
                assert (b0, nb) == ((0, cut) if lane == 0 else (cut, B - cut)) if lanes == 2 else (b0, nb) == (0, B)
                assert feats == sorted(feats) and len(set(feats)) == len(feats)            # ascending
                assert all(b0 <= filt[f] < b0 + nb for f in feats), (kind, l, lane)         # the lane's own filters
                assert all(feat_off[b0] <= f < feat_off[b0 + nb] for f in feats)
                cat += feats
            assert cat == full[(kind, l)], (kind, l)                                        # a partition, in order
        assert sorted(seen) == list(range(len(M)))
    return lanes, parts


def test_random_batches(driver):
    rng = np.random.default_rng(7)
    for _ in range(40):
        B = int(rng.integers(2, 12))
        counts = rng.integers(0, 9, size=B)
        hi = int(rng.choice([8, 30, 128]))
        M = rng.integers(1, hi + 1, size=int(counts.sum()))
        _check(driver, counts, M)


def test_filter_without_features(driver):
    rng = np.random.default_rng(1)
    for empty in range(5):
        counts = [6] * 5
        counts[empty] = 0
        _check(driver, counts, rng.integers(2, 9, size=24))


def test_class_absent_from_one_half(driver):
    # the long tracks (M = 100: last gating list, last segment class) are all in lane 0, the 2-observation ones in lane 1
    counts, M = [3, 3, 3, 3], [100, 5, 100, 20, 100, 5] + [2, 5, 20, 2, 5, 20]
    lanes, parts = _check(driver, counts, M)
    assert parts[("g", 16, 0)][2] == [0, 2, 4] and parts[("g", 16, 1)][2] == []
    assert parts[("s", 4, 0)][2] == [0, 2, 4] and parts[("s", 4, 1)][2] == []
    assert parts[("g", 0, 0)][2] == [] and parts[("g", 0, 1)][2] == [6, 9]


def test_all_features_in_one_half(driver):
    rng = np.random.default_rng(2)
    M = rng.integers(2, 40, size=12)
    for counts in ([5, 7, 0, 0], [0, 0, 4, 8], [12, 0], [0, 12]):
        lanes, parts = _check(driver, counts, M)
        empty_lane = 1 if counts[-1] == 0 else 0
        assert all(p[2] == [] for k, p in parts.items() if k[2] == empty_lane)


def test_odd_batch(driver):
    rng = np.random.default_rng(3)
    for B in (3, 5, 7, 2049):
        counts = rng.integers(0, 4, size=B)
        M = rng.integers(2, 31, size=int(counts.sum()))
        lanes, parts = _check(driver, counts, M)
        assert parts[("g", 0, 0)][:2] == (0, B // 2) and parts[("g", 0, 1)][:2] == (B // 2, B - B // 2)


def test_lane_count(driver):
    """Two lanes from 1024 filters on (two resident sets of 512, msckf_subbatch.h);
    MSCKF_SUBBATCH forces either mode for any batch of two or more; one filter never splits."""
    for B, forced, want in ((1, 0, 1), (1, 2, 1), (2, 0, 1), (2, 2, 2), (1023, 0, 1), (1024, 0, 2), (2048, 0, 2),
                            (2048, 1, 1), (5, 2, 2)):
        lanes, _, _, _ = _run(driver, [0] * B, [], forced)
        assert lanes == want, (B, forced)
    _check(driver, [2, 0, 3], [4, 9, 2, 2, 30], forced=1)
