"""CPU checks of k_kal_mchol's compile-time slot map (csrc/msckf_mchol_slots.h,
built here with the host compiler alone; its static_asserts -- every lower block
held exactly once, a wave's block column never decreasing with the slot -- hold
or the build fails) and a numpy model of the schedule the kernel runs on it:

    block column KB = 0, 1, ...: four pivot steps sc = 0 .. 3, leaving at the
    first step >= nsteps = Cp / 4 (possibly in the middle of a block column);
    per step and wave: the slots [first_slot(KB), first_slot(KB + 1)) -- block
    column KB itself -- take the step's rank-4 update while sc < 3, the slots from
    first_slot(KB + 1) on take it always.

The model follows the (wave, slot) -> block map printed by the header, applies
exact rank-4 updates to a random SPD matrix and must reproduce numpy's Cholesky
factor over the pivots and the Schur complement behind them (stage A's index
space [cams (Cp) | IMU (24)] and stage C1's full factorisation), visiting every
(block, step) pair that needs the update exactly once and no other.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "visual-inertial-odometry-msckf-stereo_amd", "csrc")
NW = 4

# stdout: "slot <NBR> <wave> <j> <brow> <bcol>" for every slot, "first <NBR> <wave> <KB> <j>" for KB = 0 .. NBR,
# "used <NBR> <wave> <n>"
_DRIVER = r"""
#include <cstdio>
#include "msckf_mchol_slots.h"
using namespace msckf;
template <int NBR>
static void dump() {
    constexpr int NW = 4;
    for (int w = 0; w < NW; ++w) {
        for (int j = 0; j < mk_nslots(NBR, NW); ++j)
            std::printf("slot %d %d %d %d %d\n", NBR, w, j, mk_brow(NBR, NW, w, j), mk_bcol(NBR, NW, w, j));
        for (int kb = 0; kb <= NBR; ++kb) std::printf("first %d %d %d %d\n", NBR, w, kb, mk_first_slot(NBR, NW, w, kb));
        std::printf("used %d %d %d\n", NBR, w, mk_used_slots(NBR, NW, w));
    }
}
int main() {
    dump<8>();
    dump<12>();
    dump<13>();
    dump<14>();
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
def slot_map(tmp_path_factory):
    """{NBR: (slots[w] = [(brow, bcol), ...], first[w][KB], used[w])} as the header computes them."""
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler (c++, g++ or the ROCm clang++) to build msckf_mchol_slots.h with"
    d = tmp_path_factory.mktemp("mchol_slots")
    src, exe = d / "slots.cpp", d / "slots"
    src.write_text(_DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    maps = {}
    for ln in out:
        t = ln.split()
        if not t:
            continue
        v = [int(x) for x in t[1:]]
        m = maps.setdefault(v[0], ([[] for _ in range(NW)], [{} for _ in range(NW)], [0] * NW))
        if t[0] == "slot":
            assert v[2] == len(m[0][v[1]])
            m[0][v[1]].append((v[3], v[4]))
        elif t[0] == "first":
            m[1][v[1]][v[2]] = v[3]
        else:
            m[2][v[1]] = v[2]
    return maps


def test_header_map(slot_map):
    """The dealing: slot j of wave w holds block w + 4 j of the column-major lower
    order; 23 / 20 accumulators per wave in the bench's kernels (NBR 13 / 12)."""
    for NBR in (8, 12, 13, 14):
        slots, first, used = slot_map[NBR]
        order = [(r, c) for c in range(NBR) for r in range(c, NBR)]
        SL = -(-len(order) // NW)
        assert SL == {8: 9, 12: 20, 13: 23, 14: 27}[NBR]
        for w in range(NW):
            assert len(slots[w]) == SL
            for j, (r, c) in enumerate(slots[w]):
                t = w + NW * j
                assert (r, c) == (order[t] if t < len(order) else (-1, NBR))
            assert used[w] == sum(1 for r, _ in slots[w] if r >= 0)
            cols = [c for _, c in slots[w]]
            assert cols == sorted(cols)
            for kb in range(NBR + 1):
                assert first[w][kb] == sum(1 for c in cols if c < kb)


def _model(slot_map, NBR, M, nsteps):
    """The kernel's schedule on the padded 16 NBR matrix M (lower part used): returns the
    Cholesky columns of the 4 nsteps pivots and the matrix left in the blocks."""
    slots, first, used = slot_map[NBR]
    n = 16 * NBR
    assert M.shape == (n, n)
    blk = {}   # (wave, slot) -> 16 x 16 block
    for w in range(NW):
        for j in range(used[w]):
            r, c = slots[w][j]
            blk[(w, j)] = M[16 * r:16 * r + 16, 16 * c:16 * c + 16].copy()
    L = np.zeros((n, 4 * nsteps))
    visits = {}
    done = False
    for KB in range(NBR):
        for sc in range(4):
            s = 4 * KB + sc
            if s >= nsteps:
                done = True
                break
            p0 = 4 * s
            X = np.zeros((n, 4))   # the panel: the step's four columns, dumped by their owners
            for w in range(NW):
                for j in range(first[w][KB], first[w][KB + 1]):
                    r, c = slots[w][j]
                    assert c == KB
                    X[16 * r:16 * r + 16] = blk[(w, j)][:, 4 * sc:4 * sc + 4]
            Ad = np.tril(X[p0:p0 + 4]) + np.tril(X[p0:p0 + 4], -1).T
            Ld = np.linalg.cholesky(Ad)
            Y = np.linalg.solve(Ld, X[p0:].T).T
            Y[:4] = Ld                                     # the diagonal block: zeros above the diagonal
            L[p0:, p0:p0 + 4] = Y
            Ainv = np.linalg.inv(Ad)
            for w in range(NW):
                j0, j1 = first[w][KB], first[w][KB + 1]
                act = (list(range(j0, j1)) if sc < 3 else []) + list(range(j1, used[w]))
                for j in act:
                    r, c = slots[w][j]
                    blk[(w, j)] -= X[16 * r:16 * r + 16] @ Ainv @ X[16 * c:16 * c + 16].T
                    visits[(r, c, s)] = visits.get((r, c, s), 0) + 1
        if done:
            break
    # every (block, step) that needs the update, once: blocks right of the pivots' block column, and
    # those of the column itself while one of its steps is still to come
    want = {(r, c, s) for c in range(NBR) for r in range(c, NBR) for s in range(nsteps)
            if c > s // 4 or (c == s // 4 and s % 4 < 3)}
    assert set(visits) == want and all(v == 1 for v in visits.values())
    R = np.zeros((n, n))
    for w in range(NW):
        for j in range(used[w]):
            r, c = slots[w][j]
            R[16 * r:16 * r + 16, 16 * c:16 * c + 16] = blk[(w, j)]
    return L, R


def _spd(n, rng):
    A = rng.standard_normal((n, n + 8))
    return A @ A.T / n + 0.5 * np.eye(n)


def _nbr_a(C):
    Cp = (C + 3) & ~3
    need = (Cp + 24 + 15) // 16
    return next(k for k in (8, 12, 13, 14) if need <= k)


def _nbr_c(C):
    need = (C + 15) // 16
    return next(k for k in (8, 12, 13, 14) if need <= k)


# C = 6 ncams; Cp / 4 = 3, 5, 8, 32, 33, 44, 45, 48 steps: the loop leaves at sc = 3, 1, 0 (a column boundary),
# 0, 1, 0, 1 and 0; the IMU rows start at offsets 12, 4, 0, 0, 4, 0, 4 and 0 of their block
SIZES = [12, 18, 30, 126, 132, 174, 180, 192]
CASES = [(C, None) for C in SIZES] + [(12, 13), (30, 13), (126, 14), (132, 13), (18, 12), (174, 14)]


@pytest.mark.parametrize("C,NBR", CASES)
def test_schedule_stage_a_form(slot_map, C, NBR):
    """[P_cc P_ci; P_ic P_ii] in index space [cams (Cp) | IMU (24)], identity padding: the partial
    factor over the Cp cam pivots and the Schur complement S_ii, against numpy, 1e-12 relative."""
    NBR = NBR or _nbr_a(C)
    Cp = (C + 3) & ~3
    n = 16 * NBR
    assert Cp + 24 <= n
    rng = np.random.default_rng(1000 + C)
    S = _spd(C + 21, rng)                 # [cams (C) | IMU (21)]
    M = np.eye(n)
    idx = np.r_[0:C, Cp:Cp + 21]
    M[np.ix_(idx, idx)] = S
    L, R = _model(slot_map, NBR, M, Cp // 4)
    ref = np.linalg.cholesky(M[:Cp, :Cp])
    V = np.linalg.solve(ref, M[:Cp, Cp:Cp + 24]).T        # P_ic Lc^-T
    Sii = M[Cp:Cp + 24, Cp:Cp + 24] - V @ V.T
    assert np.linalg.norm(L[:Cp] - ref) <= 1e-12 * np.linalg.norm(ref)
    assert np.linalg.norm(L[Cp:Cp + 24] - V) <= 1e-12 * np.linalg.norm(V)
    got = np.tril(R[Cp:Cp + 24, Cp:Cp + 24])
    assert np.linalg.norm(got - np.tril(Sii)) <= 1e-12 * np.linalg.norm(Sii)


@pytest.mark.parametrize("C,NBR", CASES)
def test_schedule_stage_c1_form(slot_map, C, NBR):
    """T (C x C), identity padding up to 16 NBR: the whole factor, against numpy, 1e-12 relative."""
    NBR = NBR or _nbr_c(C)
    Cp = (C + 3) & ~3
    n = 16 * NBR
    assert Cp <= n
    rng = np.random.default_rng(2000 + C)
    M = np.eye(n)
    M[:C, :C] = _spd(C, rng)
    L, _ = _model(slot_map, NBR, M, Cp // 4)
    ref = np.linalg.cholesky(M[:Cp, :Cp])
    assert np.linalg.norm(L[:Cp] - ref) <= 1e-12 * np.linalg.norm(ref)
