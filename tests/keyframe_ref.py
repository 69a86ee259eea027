"""The keyframe choice of include/msckf_keyframes.h restated in numpy on arrays,
and the fixed cases of tests/test_keyframe_ref.py (CPU, against the host's
MSCKF._find_redundant_cam_states) and tests/test_gpu_keyframes.py (the device).

``choice(cams [n][11], rate)`` -> Choice(slots [2] ascending, ang [2], dist [2],
branch [2] of to_quaternion, outcome).  ``case_groups()``: groups of four cases
with 4, 5, 22 and 70 cam states -- one per filter of a four-filter context.
Every case keeps ang and dist at least MARGIN from their thresholds, also after
its poses went through float32 (``rounded``): the host, this file and the device
evaluate the same fp64 formulas on the same stored values, their roundings move
ang by about 1e-14, so the decisions agree exactly.
"""
import collections

import numpy as np

ROT_THR, TRANS_THR, RATE_THR = 0.2618, 0.4, 0.5   # msckf.py:711
MARGIN = 1e-6
SIZES = (4, 5, 22, 70)
OUTCOMES = ("both_newest", "oldest_second", "oldest_first", "two_oldest")

Choice = collections.namedtuple("Choice", ["slots", "ang", "dist", "branch", "outcome"])


def rotation(q):
    """to_rotation of q / |q| (JPL, [x y z w])."""
    q = np.asarray(q, float)
    x, y, z, w = q / np.sqrt((q * q).sum())
    d = 2 * w * w - 1
    return np.array([[d + 2 * x * x, 2 * w * z + 2 * x * y, -2 * w * y + 2 * x * z],
                     [-2 * w * z + 2 * y * x, d + 2 * y * y, 2 * w * x + 2 * y * z],
                     [2 * w * y + 2 * z * x, -2 * w * x + 2 * z * y, d + 2 * z * z]])


def quaternion(M):
    """(to_quaternion(M) before its normalisation, the branch 0..3 taken)."""
    if M[2, 2] < 0:
        if M[0, 0] > M[1, 1]:
            return np.array([1 + M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2],
                             M[1, 2] - M[2, 1]]), 0
        return np.array([M[0, 1] + M[1, 0], 1 - M[0, 0] + M[1, 1] - M[2, 2], M[2, 1] + M[1, 2],
                         M[2, 0] - M[0, 2]]), 1
    if M[0, 0] < -M[1, 1]:
        return np.array([M[0, 2] + M[2, 0], M[2, 1] + M[1, 2], 1 - M[0, 0] - M[1, 1] + M[2, 2],
                         M[0, 1] - M[1, 0]]), 2
    return np.array([M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0],
                     1 + M[0, 0] + M[1, 1] + M[2, 2]]), 3


def choice(cams, rate, rot_thr=ROT_THR, trans_thr=TRANS_THR, rate_thr=RATE_THR):
    cams = np.asarray(cams, np.float64)
    n = len(cams)
    if n < 4:
        raise ValueError("%d cam states: the keyframe choice needs 4" % n)
    key = n - 4
    Rk, pk = rotation(cams[key, 0:4]), cams[key, 4:7]
    slots, ang, dist, branch, took = [], np.zeros(2), np.zeros(2), [0, 0], []
    first = 0
    for j in range(2):
        c = n - 3 + j
        u, branch[j] = quaternion(rotation(cams[c, 0:4]) @ Rk.T)
        with np.errstate(invalid="ignore"):
            ang[j] = 2 * np.arccos(u[3] / np.sqrt((u * u).sum()))
        d = cams[c, 4:7] - pk
        dist[j] = np.sqrt((d * d).sum())
        if ang[j] < rot_thr and dist[j] < trans_thr and rate > rate_thr:   # a NaN comparison is false
            slots.append(c)
            took.append(True)
        else:
            slots.append(first)
            first += 1
            took.append(False)
    outcome = OUTCOMES[{(True, True): 0, (False, True): 1, (True, False): 2, (False, False): 3}[tuple(took)]]
    return Choice(np.array(sorted(slots), np.int32), ang, dist, tuple(branch), outcome)


def margins_ok(cams, rate):
    c = choice(cams, rate)
    return bool((np.abs(c.ang - ROT_THR) >= MARGIN).all() and (np.abs(c.dist - TRANS_THR) >= MARGIN).all())


def rounded(case):
    """The case with its poses rounded through float32: what an fp32 context stores."""
    out = dict(case)
    out["cams"] = case["cams"].astype(np.float32).astype(np.float64)
    return out


# -------------------------------------------------------------------- cases --
def _unit(rng):
    v = rng.standard_normal(4)
    return v / np.linalg.norm(v)


def _quat_of(R):
    u, _ = quaternion(R)
    return u / np.linalg.norm(u)


def make_case(rng, n, name, a, d, rate, axes=(None, None), scale=1.0):
    """n cam records: random poses, the two candidates at rotation angle a[j]
    about axes[j] (None: random) and distance d[j] from the key pose; every
    quaternion multiplied by ``scale`` (an array scales each record's)."""
    cams = np.zeros((n, 11))
    for i in range(n):
        cams[i, 0:4] = _unit(rng)
        cams[i, 4:7] = rng.uniform(-1.5, 1.5, 3)
        cams[i, 7:11] = cams[i, 0:4]
    key = n - 4
    Rk = rotation(cams[key, 0:4])
    for j in range(2):
        ax = np.asarray(axes[j], float) if axes[j] is not None else rng.standard_normal(3)
        ax = ax / np.linalg.norm(ax)
        Rrel = rotation(np.array([*(ax * np.sin(a[j] / 2)), np.cos(a[j] / 2)]))
        cams[n - 3 + j, 0:4] = _quat_of(Rrel @ Rk)
        t = rng.standard_normal(3)
        cams[n - 3 + j, 4:7] = cams[key, 4:7] + d[j] * t / np.linalg.norm(t)
    cams[:, 0:4] *= np.reshape(scale, (-1, 1)) if np.ndim(scale) else scale
    case = dict(name=name, n=n, cams=cams, rate=float(rate))
    assert margins_ok(cams, rate) and margins_ok(rounded(case)["cams"], rate), name
    return case


_E = 2e-5   # how close the near-threshold cases come (float32 poses move ang and dist by about 1e-7)
_PI = np.pi - 0.01
# (name, a[2], d[2], rate, axes[2], scale) -- each built at every size of SIZES in turn
_SPECS = [
    ("both_newest", (0.10, 0.15), (0.10, 0.20), 0.9, (None, None), 1.0),
    ("oldest_second", (0.40, 0.15), (0.10, 0.20), 0.9, (None, None), 1.0),
    ("oldest_first", (0.10, 0.15), (0.10, 0.60), 0.9, (None, None), 1.0),
    ("two_oldest", (0.30, 0.10), (0.10, 0.45), 0.9, (None, None), 1.0),
    ("near_pi_x", (_PI, 0.10), (0.10, 0.10), 0.9, ((1, 0, 0), None), 1.0),
    ("near_pi_y", (0.10, _PI), (0.10, 0.10), 0.9, (None, (0, 1, 0)), 1.0),
    ("near_pi_z", (_PI, _PI), (0.10, 0.10), 0.9, ((0, 0, 1), (0, 0, 1)), 1.0),
    ("near_pi_xy", (_PI, _PI), (0.10, 0.10), 0.9, ((1, 0, 0), (0, 1, 0)), 1.0),
    ("rate_exactly_half", (0.10, 0.15), (0.10, 0.20), 0.5, (None, None), 1.0),
    ("rate_just_above_half", (0.10, 0.15), (0.10, 0.20), float(np.nextafter(0.5, 1.0)), (None, None), 1.0),
    ("rate_low", (0.10, 0.15), (0.10, 0.20), 0.2, (None, None), 1.0),
    ("rate_nan", (0.10, 0.15), (0.10, 0.20), float("nan"), (None, None), 1.0),
    ("ang_just_below", (ROT_THR - _E, ROT_THR - _E), (0.10, 0.20), 0.9, (None, None), 1.0),
    ("ang_just_above", (ROT_THR + _E, 0.10), (0.10, 0.20), 0.9, (None, None), 1.0),
    ("dist_just_below", (0.10, 0.15), (TRANS_THR - _E, TRANS_THR - _E), 0.9, (None, None), 1.0),
    ("dist_just_above", (0.10, 0.15), (0.10, TRANS_THR + _E), 0.9, (None, None), 1.0),
    ("scaled_2", (0.10, 0.40), (0.10, 0.20), 0.9, (None, None), 2.0),
    ("scaled_down", (0.10, 0.15), (0.10, 0.20), 0.9, (None, None), 0.37),
    ("scaled_negative", (0.40, 0.15), (0.10, 0.20), 0.9, (None, None), -1.7),
    ("scaled_slightly", (0.10, 0.15), (0.60, 0.20), 0.9, (None, None), 1.0 + 1e-3),
    ("identical_poses_apart", (0.0, 0.0), (0.10, 0.20), 0.9, (None, None), 1.0),
    ("same_place", (0.10, 0.15), (0.0, 0.0), 0.9, (None, None), 1.0),
]
N_RANDOM = 12   # random draws of angle, distance and rate on top, per size


def case_groups():
    """Groups of four cases, one per size of SIZES in that order."""
    rng = np.random.default_rng(20240611)
    groups = []
    for k in range(len(_SPECS)):   # spec k + i at size i: every spec meets every size once
        grp = []
        for i, n in enumerate(SIZES):
            nm, aa, dd, rr, ax, sc = _SPECS[(k + i) % len(_SPECS)]
            if sc != 1.0 and i % 2:   # at every other size a scale per record
                sc = sc * rng.uniform(0.5, 1.5, n)
            grp.append(make_case(rng, n, "%s_n%d" % (nm, n), aa, dd, rr, ax, sc))
        groups.append(grp)
    for k in range(N_RANDOM):
        grp = []
        for n in SIZES:
            while True:
                a, d = rng.uniform(0.0, 0.5, 2), rng.uniform(0.0, 0.8, 2)
                try:
                    grp.append(make_case(rng, n, "random%d_n%d" % (k, n), a, d, rng.uniform(0.3, 1.0),
                                         scale=rng.uniform(0.5, 2.0, n) if k % 2 else 1.0))
                    break
                except AssertionError:   # a draw inside the margin: the next one
                    continue
        groups.append(grp)
    return groups


_GROUPS = []


def groups():
    if not _GROUPS:
        _GROUPS.extend(case_groups())
    return _GROUPS


def cases():
    return [c for g in groups() for c in g]
