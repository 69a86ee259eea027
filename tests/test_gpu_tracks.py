"""The device-side feature tracks of include/msckf_tracks.h (mfe_tracks_create,
_put, _get, _step) and MultiImageProcessor with ``device_tracks`` on the device.

Step equals composition: tests/frontend_tracks_ref.py restates the header's
steps 1-9 around the set calls; fed the real ``Frontend`` every stage is a
device call pinned by tests/test_gpu_lanes.py and tests/test_gpu_ransac.py, so
mfe_tracks_step must equal it exactly -- n, ids, lifetimes, cam0, cam1 (through
tracks_get), the bytes of uv, the counters, n_total and next_id.  No tolerance
is involved anywhere in this file.

CASES: 150 x 110 images (no multiple of 16 or 64), ``cap`` the smallest the grid
allows; 1, 2 and 3 lanes per call; tables of 0, 1, 63, 64, 65 and 100 rows;
grids 1 x 1 and 4 x 5; (grid_min, grid_max) of (1, 1), (3, 5) and (2, 16);
radtan and equidistant lanes in one call; RANSAC in some lanes; two consecutive
steps each.  The scenes (lane_frames, lane_table) hold a flat patch in cam0
(LK failures), a flat band on the right (cells without candidates), a blanked
corner in cam1 (stereo failures, cells with fewer new features), rows at the
top edge (the bounds test), rows with a displaced cam1 point (RANSAC) and
lifetimes of 1..4 (ties in the prune); test_the_cases_cover_every_branch asserts
from the reference's own counters that each branch occurs.

BIG: the kernels' compactions and the per-cell gather walk 256 rows at a time,
so three more CASES hold tables of 257, 600 and 700 rows (376 x 240 images for
the latter two, ``cap`` no multiple of 256): the survivors of steps 2, 3 and 4
each above 512 in a 4 x 5 grid, next to a lane of 40 rows and an empty one, and
one cell of more than 512 rows in a 1 x 1 grid pruned to 16.
test_the_big_cases_pass_one_chunk asserts that from the reference's lists.

End to end: the lanes of tests/test_gpu_lanes.py's three-lane test publish, with
device_tracks, what single ImageProcessors publish, bit for bit.  The lanes of
one mfe_tracks_step share grid_min_feature_num (the constructor rejects a
mix), so the third stream runs twice: started late at grid_min 3 next to the two
golden scenes, and alone in a one-lane MultiImageProcessor at grid_min 2."""
from collections import Counter

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from conftest import golden
from frontend_ref_scenes import SCENES, scene_config
import frontend_synth as fs
import frontend_lanes_ref as lr
import frontend_tracks_ref as tr

pytestmark = pytest.mark.gpu
W, H = 150, 110
LK = dict(win=15, max_level=2, max_iter=30, eps=0.01)
MOTION, DISPARITY, THRESHOLD, INLIER_ERROR, N_HYP = (2.0, -1.5), 5.0, 15, 3.0, 7
# name: (grid_row, grid_col, grid_min, grid_max), [(rows, camera kind, RANSAC, texture seed) per lane]
CASES = {
    "4x5_3_5": ((4, 5, 3, 5), [(100, 0, True, 21), (63, 2, False, 22), (0, 1, False, 23)]),
    "4x5_2_16": ((4, 5, 2, 16), [(64, 1, True, 24), (65, 0, True, 25)]),
    "4x5_1_1": ((4, 5, 1, 1), [(20, 2, False, 26)]),
    "1x1_1_1": ((1, 1, 1, 1), [(1, 0, False, 27), (0, 2, False, 28), (1, 1, True, 29)]),
    "1x1_2_16": ((1, 1, 2, 16), [(16, 0, True, 30)]),
    "1x1_3_5": ((1, 1, 3, 5), [(5, 1, False, 31), (2, 2, True, 32)]),
    # beyond one 256-row chunk of k_trk_compact / k_trk_assemble (see BIG below)
    "4x5_3_5_257": ((4, 5, 3, 5), [(257, 0, True, 33)]),
    "4x5_3_5_700": ((4, 5, 3, 5), [(700, 0, True, 34), (40, 1, False, 35), (0, 2, False, 36)]),
    "1x1_2_16_600": ((1, 1, 2, 16), [(600, 0, False, 37)]),
}
# The cases whose tables pass 256 rows: (W, H) where the 150 x 110 scene has too few corners, and a
# ``cap`` a little above rows + cells grid_min that is no multiple of 256.  None of them uses H > 256:
# the row scan's case of several rows per thread is tests/test_gpu_pipeline.py's and test_gpu_lanes.py's.
BIG = {"4x5_3_5_257": ((W, H), 320), "4x5_3_5_700": ((376, 240), 765), "1x1_2_16_600": ((376, 240), 605)}
_cache = {}


def camera(kind):
    """(cam0, cam1, R_guess, E, stereo_threshold): a rectified radtan pair, a
    distorted radtan pair under the EuRoC extrinsics, an equidistant pair (the
    cameras of tests/test_gpu_lanes.py)."""
    g = golden("frontend_ref")

    def ext(T_imu_cam0, T_imu_cam1):                      # R_cam0_cam1 and E as ImageProcessor forms them
        T0, T1 = fe_mod._inv_T(T_imu_cam0), fe_mod._inv_T(T_imu_cam1)
        R = T1[:3, :3].T @ T0[:3, :3]
        return R, fe_mod._skew(T1[:3, :3].T @ (T0[:3, 3] - T1[:3, 3])) @ R
    K0, K1 = np.array([90.0, 90.0, 75.0, 55.0]), np.array([91.0, 89.5, 74.0, 56.0])
    if kind == 0:
        R, E = ext(g["rectified_T_imu_cam0"], g["rectified_T_imu_cam1"])
        return (K0, 0, np.zeros(4)), (K0, 0, np.zeros(4)), R, E, 5.0
    R, E = ext(g["euroc_T_imu_cam0"], g["euroc_T_imu_cam1"])
    if kind == 1:
        return (K0, 0, g["euroc_distortion"]), (K1, 0, g["euroc_distortion1"]), R, E, 5.0
    k = np.array([0.01, -0.005, 0.001, -0.0002])
    return (K0, 1, k), (K1, 1, k), np.eye(3), E, 5.0      # equidistant: the reference never rectifies the guess


def lane_frames(seed, W=W, H=H):
    """Three stereo frames of a texture moving by MOTION per frame."""
    f = fs.texture_fn(seed, W=W, H=H)
    out = []
    for k in range(3):
        dx, dy = MOTION[0] * k, MOTION[1] * k
        im0, im1 = fs.render(f, W, H, dx, dy).copy(), fs.render(f, W, H, dx - DISPARITY, dy).copy()
        im0[:, 4 * W // 5:], im1[:, 4 * W // 5 - 5:] = 90, 90     # the last grid column holds no corner
        im0[40:70, 60:90] = 128                      # rows here fail LK
        im1[:34, :55] = 70                           # candidates here fail the stereo match
        out.append((im0, im1))
    return out


def lane_table(ops, lane, n, kind, seed):
    """n rows for the lane whose slots hold frame 0 in (c0, c1): detected corners
    with their stereo matches, a row in the flat patch, rows at the top edge
    and next to a cell boundary; every 6th row's cam1 displaced.  A table of more
    rows than the frame has corners repeats corners, each row with its own offset."""
    if n == 0:
        return tr.empty_table(1000 * (lane + 1))
    cam0, cam1, R, E, thr = camera(kind)
    xy, _ = ops.fast(3 * lane + 1, THRESHOLD)
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(xy))[:n]
    if len(pick) < n:
        pick = np.concatenate([pick, rng.integers(0, len(xy), n - len(pick))])
    p = xy[pick].astype(np.float32) + rng.uniform(0, 0.9, (n, 2)).astype(np.float32)
    extra = np.array([[75.25, 55.5], [70.5, 0.75], [31.0, 1.25], [28.75, 50.5], [100.5, 0.5], [58.5, 27.0]], np.float32)
    m = min((n + 1) // 2, len(extra))
    p[:m] = extra[:m]
    c1 = np.asarray(ops.stereo_match_sets([(3 * lane + 1, 3 * lane + 2, p.astype(float), cam0, cam1, R, E, thr)],
                                          **LK)[0][0], np.float32).copy()
    c1[5::6] += np.float32([9.0, -6.0])
    return tr.make_table(100 * lane + 3 * np.arange(n), (7 * np.arange(n)) % 4 + 1, p, c1, 1000 * (lane + 1))


def lane_args(lane, kind, ransac, step, seed):
    """The lane's TracksLane at step 0 or 1: the slots rotate as ImageProcessor's do."""
    cam0, cam1, R, E, thr = camera(kind)
    K = np.array([[cam0[0][0], 0.0, cam0[0][2]], [0.0, cam0[0][1], cam0[0][3]], [0.0, 0.0, 1.0]])
    R0 = fe_mod._rodrigues(np.array([0.002, -0.003, 0.004]) * (1 + lane + step)).T
    R1 = fe_mod._rodrigues(np.array([0.002, -0.003, 0.0035]) * (1 + lane + step)).T
    rs = None
    if ransac:
        rs = (R0, R1, np.random.default_rng(seed + step).integers(0, 1 << 32, size=(2, N_HYP, 2), dtype=np.uint32))
    prev, c0 = (3 * lane + 1, 3 * lane) if step == 0 else (3 * lane, 3 * lane + 1)
    return fe_mod.TracksLane(lane, prev, c0, 3 * lane + 2, K @ R0 @ np.linalg.inv(K), cam0, cam1, R, E, thr, rs)


def run_case(ops, name, on_tables=None):
    """Two consecutive reference steps of the case on ``ops`` (a Frontend or its
    CPU stand-in).  ``on_tables(step, tables, lanes, args)`` runs before each
    reference step, the images in place.  Returns [(results, tables after)], the
    cover counters and the two steps' traces."""
    (rows, cols, gmin, gmax), lanes = CASES[name]
    grid = tr.Grid(rows, cols, gmin, gmax)
    Wc, Hc = BIG.get(name, ((W, H), 0))[0]
    frames = [lane_frames(seed, Wc, Hc) for _, _, _, seed in lanes]
    S = len(lanes)
    ops.upload_many([3 * l + 1 + j for l in range(S) for j in range(2)],
                    np.stack([frames[l][0][j] for l in range(S) for j in range(2)]))
    tables = {l: lane_table(ops, l, n, kind, seed) for l, (n, kind, _, seed) in enumerate(lanes)}
    out, cover, traces = [], Counter(), []
    for step in range(2):
        # frame step + 1: cam0 into the slot that is not the previous image's, cam1 into the third
        c0 = [3 * l if step == 0 else 3 * l + 1 for l in range(S)]
        ops.upload_many([s for l in range(S) for s in (c0[l], 3 * l + 2)],
                        np.stack([frames[l][step + 1][j] for l in range(S) for j in range(2)]))
        args = [lane_args(l, kind, ransac, step, seed) for l, (_, kind, ransac, seed) in enumerate(lanes)]
        if on_tables:
            on_tables(step, tables, lanes, args)
        traces.append({})
        res, nxt, cov = tr.step(ops, tables, args, grid, Wc, Hc, THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP,
                                trace=traces[-1], **LK)
        tables = {**tables, **nxt}
        cover += cov
        out.append((res, tables))
    return out, cover, traces


def same_result(a, b):
    assert a.n == b.n and a.n_total == b.n_total and a.next_id == b.next_id
    np.testing.assert_array_equal(a.ids, b.ids)
    np.testing.assert_array_equal(a.counters, b.counters)
    assert a.uv.shape == b.uv.shape == (a.n, 4) and a.uv.tobytes() == b.uv.tobytes()


def same_table(got, want):
    ids, life, cam0, cam1, next_id = got
    np.testing.assert_array_equal(ids, want.ids)
    np.testing.assert_array_equal(life, want.life)
    assert cam0.tobytes() == want.cam0.tobytes() and cam1.tobytes() == want.cam1.tobytes()
    assert next_id == want.next_id


def device_case(name):
    """The case on the device next to its reference; cached for the coverage test."""
    if name in _cache:
        return _cache[name]
    (rows, cols, gmin, gmax), lanes = CASES[name]
    S = len(lanes)
    (Wc, Hc), cap = BIG.get(name, ((W, H), tr.min_cap(tr.Grid(rows, cols, gmin, gmax))))
    fe = fe_mod.Frontend(Wc, Hc, nslot=3 * S, max_level=LK["max_level"], max_points=4096)
    got = []
    try:
        fe.tracks_create(S, cap, rows, cols, gmin, gmax)

        def on_tables(step, tables, lanes_, args):
            if step == 0:
                for l, t in tables.items():
                    fe.tracks_put(l, t.ids, t.life, t.cam0, t.cam1, t.next_id)
                    same_table(fe.tracks_get(l), t)                      # put / get round trip
            # the second step reads what the first wrote
            res = fe.tracks_step(args, THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)
            got.append((res, [fe.tracks_get(l) for l in range(S)]))
        ref, cover, traces = run_case(fe, name, on_tables)
    finally:
        fe.close()
    _cache[name] = (got, ref, cover, traces)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_step_equals_the_composition_of_set_calls(name):
    got, ref = device_case(name)[:2]
    assert len(got) == len(ref) == 2
    for step, ((res, tabs), (rres, rtabs)) in enumerate(zip(got, ref)):
        assert len(res) == len(rres) == len(CASES[name][1])
        for a, b in zip(res, rres):
            same_result(a, b)
        for l, t in enumerate(tabs):
            same_table(t, rtabs[l])
    assert sum(r.n for r in got[1][0]) > 0


def test_the_cases_cover_every_branch():
    """A condition on the inputs: the reference's counters over all CASES."""
    cover, sizes, lanes_per_call = Counter(), set(), set()
    for name, (_, lanes) in CASES.items():
        cover += device_case(name)[2]
        sizes |= {n for n, _, _, _ in lanes}
        lanes_per_call.add(len(lanes))
    assert sizes >= {0, 1, 63, 64, 65, 100} and lanes_per_call == {1, 2, 3}
    for what in ("lk_status", "bounds", "stereo", "ransac", "cell_change", "pruned_tie", "new_fewer", "new_none",
                 "no_survivors", "empty_table"):
        assert cover[what] > 0, (what, dict(cover))


def test_the_big_cases_pass_one_chunk():
    """A condition on the inputs of the BIG cases, from the reference's counters and
    lists at their first step: k_trk_compact and k_trk_assemble walk 256 rows at a
    time and carry the rows kept so far from chunk to chunk."""
    for name, (_, cap) in BIG.items():
        (rows, cols, gmin, gmax), lanes = CASES[name]
        assert cap % 256 and cap >= max(n for n, _, _, _ in lanes) + rows * cols * gmin
    # tables of 257 and of 513 rows or more; next to the largest a lane below 64 rows and an empty one
    assert [n for n, _, _, _ in CASES["4x5_3_5_257"][1]] == [257]
    assert [(n >= 513, 0 < n < 64, n == 0) for n, _, _, _ in CASES["4x5_3_5_700"][1]] == [
        (True, False, False), (False, True, False), (False, False, True)]
    assert CASES["4x5_3_5_700"][1][0][2]                         # RANSAC in the large lane: its set grids pass a block
    _, ref, _, traces = device_case("4x5_3_5_700")
    ctr = ref[0][0][0].counters
    assert ctr[0] == 700 and (ctr[:3] > 512).all() and (ctr[1:] > 256).all(), ctr    # each compaction reads three chunks
    keep = traces[0]["keep", 0]
    assert [len(k) for k in keep] == ctr[:3].tolist()
    for stage, k in enumerate(keep):                             # dropped inside the first chunk, kept inside a later one
        assert (~k[:256]).any() and k[256:].any(), stage
        assert 0 < k[:256].sum() < 256                           # the carried count is neither 0 nor the chunk's start
    keep = device_case("4x5_3_5_257")[3][0]["keep", 0][0]
    assert len(keep) == 257 and (~keep[:256]).any() and keep[256]      # the one row of the second chunk is written
    # one cell above 256 rows: gathered across chunks, ranked by lifetime with ties across the chunk edges
    _, ref, _, traces = device_case("1x1_2_16_600")
    res = ref[0][0][0]
    assert res.counters[3] > 256 and traces[0]["cell", 0] >= res.counters[3] and res.n == 16
    life = ref[0][1][0].life
    assert (life == life[0]).all() and life[0] == 5              # the longest-lived alone fill the cell


def small_context(S=3, grid=(4, 5, 3, 5), rows=(40, 12, 0), seeds=(21, 22, 23), cap=None):
    """A context with S lanes, frame 0 -> 1 in the slots and a table in each lane."""
    fe = fe_mod.Frontend(W, H, nslot=3 * S, max_level=LK["max_level"], max_points=4096)
    fe.tracks_create(S, cap or tr.min_cap(tr.Grid(*grid)), *grid)
    frames = [lane_frames(s) for s in seeds]
    fe.upload_many([3 * l + 1 + j for l in range(S) for j in range(2)],
                   np.stack([frames[l][0][j] for l in range(S) for j in range(2)]))
    tables = [lane_table(fe, l, rows[l], 0, seeds[l]) for l in range(S)]
    fe.upload_many([s for l in range(S) for s in (3 * l, 3 * l + 2)],
                   np.stack([frames[l][1][j] for l in range(S) for j in range(2)]))
    for l, t in enumerate(tables):
        fe.tracks_put(l, t.ids, t.life, t.cam0, t.cam1, t.next_id)
    args = [lane_args(l, 0, l == 0, 0, seeds[l]) for l in range(S)]
    return fe, tables, args


def test_overflow_returns_minus_3_and_changes_no_table():
    fe, tables, args = small_context()
    try:
        with pytest.raises(_lib.MsckfError, match="rc=-3") as e:
            fe.tracks_step(args, THRESHOLD, max_kp=8, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)
        for l, t in enumerate(tables):
            same_table(fe.tracks_get(l), t)
        res = fe.tracks_step(args, THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)
        assert e.value.n_total.tolist() == [r.n_total for r in res] and max(r.n_total for r in res) > 8
    finally:
        fe.close()
    # a table above 256 rows at cap 320: 260 rows + 20 cells x grid_min 3 == cap
    fe, tables, args = small_context(S=1, rows=(260,), seeds=(33,), cap=320)
    try:
        t = tables[0]
        more = (np.append(t.ids, -5), np.append(t.life, 1), np.vstack([t.cam0, t.cam0[:1]]), np.vstack([t.cam1, t.cam1[:1]]))
        with pytest.raises(_lib.MsckfError, match="rc=-1"):       # n + cells grid_min == cap + 1: no room for the new rows
            fe.tracks_put(0, *more, t.next_id)
        same_table(fe.tracks_get(0), t)
        with pytest.raises(_lib.MsckfError, match="rc=-3") as e:
            fe.tracks_step(args, THRESHOLD, max_kp=8, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)
        same_table(fe.tracks_get(0), t)
        res = fe.tracks_step(args, THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)
        assert e.value.n_total.tolist() == [res[0].n_total] and res[0].n_total > 8
        assert res[0].counters[0] == 260 and res[0].counters[3] > 0 and res[0].n + 60 <= 320
    finally:
        fe.close()


def test_bad_arguments_are_errors_and_leave_the_tables():
    fe, tables, args = small_context()
    step = lambda a, **kw: fe.tracks_step(a, THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **{**LK, **kw})
    try:
        cap = fe.tracks_cap
        for bad in ([args[0]._replace(lane=3)], [args[0]._replace(lane=-1)],                 # lane index
                    [args[0], args[1]._replace(slot_c1=9)], [args[1]._replace(slot_prev=-1)],  # slot
                    [args[0], args[1], args[0]], [args[2], args[2]._replace(slot_c1=1)],       # a lane named twice
                    [args[1]._replace(cam0=(args[1].cam0[0], 7, args[1].cam0[2]))]):           # distortion model
            with pytest.raises(_lib.MsckfError):
                step(bad)
        with pytest.raises(_lib.MsckfError):
            step(args, win=17)
        t = tables[0]
        big = np.arange(cap - 20 * 3 + 1)                                                    # n beyond cap less grid_min
        for n in (len(big), cap + 1):
            with pytest.raises(_lib.MsckfError):
                fe.tracks_put(1, np.arange(n), np.ones(n), np.zeros((n, 2)), np.zeros((n, 2)), 0)
        with pytest.raises(_lib.MsckfError):
            fe.tracks_put(3, t.ids, t.life, t.cam0, t.cam1, 0)
        with pytest.raises(_lib.MsckfError):
            fe.tracks_get(-1)
        with pytest.raises(_lib.MsckfError):
            fe.tracks_create(3, cap, 4, 5, 3, 5)                                             # a second set of tables
        for l, t in enumerate(tables):
            same_table(fe.tracks_get(l), t)
        assert [r.n > 0 for r in step(args)] == [True] * 3                                   # and the context works
    finally:
        fe.close()
    fe = fe_mod.Frontend(W, H, nslot=6, max_level=1, max_points=64)
    try:
        for bad in ((3, 160, 4, 5, 3, 5), (2, 159, 4, 5, 3, 5), (2, 4097, 4, 5, 3, 5), (2, 400, 4, 5, 3, 17),
                    (2, 400, 4, 5, 3, 0), (2, 4096, 33, 32, 1, 1), (0, 160, 4, 5, 3, 5)):
            with pytest.raises(_lib.MsckfError):
                fe.tracks_create(*bad)
        with pytest.raises(_lib.MsckfError):
            fe.tracks_get(0)                                                                 # no tables yet
    finally:
        fe.close()


def test_the_same_put_and_step_give_the_same_bytes():
    fe, tables, args = small_context()
    try:
        runs = []
        for _ in range(2):
            for l, t in enumerate(tables):
                fe.tracks_put(l, t.ids, t.life, t.cam0, t.cam1, t.next_id)
            res = fe.tracks_step(args[:2], THRESHOLD, inlier_error=INLIER_ERROR, n_hyp=N_HYP, **LK)   # a subset of lanes
            runs.append((res, [fe.tracks_get(l) for l in range(3)]))
        (ra, ta), (rb, tb) = runs
        for a, b in zip(ra, rb):
            same_result(a, b)
        for a, b in zip(ta, tb):
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))
        same_table(ta[2], tables[2])                                                         # the lane not named
        assert ra[0].n > 0 and ra[0].counters[0] == 40
    finally:
        fe.close()


# --------------------------------------------------------------- end to end --
def run_single(cfg, frames):
    ip = fe_mod.ImageProcessor(fe_mod.FrontendConfig(**{**vars(cfg), "device_tracks": False}))
    out = []
    for imu, msg in frames:
        for m in imu:
            ip.imu_callback(m)
        out.append(lr.unpack(ip.stareo_callback(msg)))
    ip.fe.close()
    return out


def run_tracks(cfgs, streams, start):
    """The streams through a MultiImageProcessor with device_tracks.  Returns
    the published frames, per step (lanes, launches), and the rows whose
    step-1 guess differs between the host's matmul and the header's ordered sum."""
    mp = fe_mod.MultiImageProcessor(len(cfgs), lane_configs=cfgs)
    differ, rows = [], [0]
    for ip in mp.lanes:
        def wrapped(lane, ip=ip, inner=ip._tracks_lane, imu=ip.integrate_imu_data):
            seen = []                                    # the (R0, R1) this frame's integrate_imu_data returns
            ip.integrate_imu_data = lambda: seen.append(imu()) or seen[0]
            a = inner(lane)
            ip.integrate_imu_data = imu
            cam0 = mp.tracks(lane)[2]
            host = ip.predict_feature_tracking(cam0, seen[0][0], ip.cam0_intrinsics)
            differ.extend((lane, k) for k in np.nonzero((host != tr.predict(a.Hpred, cam0)).any(axis=1))[0])
            rows[0] += len(cam0)
            return a
        ip._tracks_lane = wrapped
    steps = []
    got = lr.run_lanes(mp, streams, start=start, on_step=lambda s, lanes: steps.append((lanes, dict(mp.launches))))
    mp.close()
    return got, steps, differ, rows[0]


def test_lanes_with_device_tracks_publish_what_single_processors_publish():
    g = golden("frontend_ref")
    Wg, Hg = (int(v) for v in g["size"])
    cfgs, streams = [], []
    for name in SCENES:
        cfg = scene_config(g, name)
        cfg.device_pipeline = cfg.device_tracks = True
        cfgs.append(cfg)
        streams.append(lr.scene_frames(g, name))
    cfgs[0].ransac_enabled, cfgs[0].ransac_seed = True, 5
    third = scene_config(g, "rectified")                 # a third texture and motion
    third.device_pipeline = third.device_tracks = True
    cfgs.append(third)
    streams.append(lr.stream_frames(fs.texture_fn(9, W=Wg, H=Hg), Wg, Hg, 5, (-1.25, 0.5), (0.0, 0.01, 0.0), 10.0))
    alone = fe_mod.FrontendConfig(**{**vars(third), "grid_min_feature_num": 2})      # fewer features per cell
    got, steps, differ, rows = run_tracks(cfgs, streams, [0, 0, 2])                   # lane 2 starts late
    got2, steps2, differ2, rows2 = run_tracks([alone], streams[2:], [0])
    # a condition on the scenes, checked on the host: both forms of step 1 give the same float32 guesses
    assert differ == [] and differ2 == [] and rows > 500 and rows2 > 100
    want = [run_single(c, s) for c, s in zip(cfgs + [alone], streams + streams[2:])]
    for lane, (a, b) in enumerate(zip(got + got2, want)):
        assert len(a) == len(b)
        for k, ((ids, uv), (wids, wuv)) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(ids, wids, err_msg="lane %d frame %d" % (lane, k))
            assert uv.tobytes() == wuv.tobytes(), (lane, k)          # bit for bit
        assert len(a[-1][0]) >= 30
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(got[2], got2[0]))      # grid_min matters here
    # a step in which all three lanes track: two device calls
    assert steps[3][0] == [0, 1, 2]
    delta = {k: v - steps[2][1].get(k, 0) for k, v in steps[3][1].items() if v != steps[2][1].get(k, 0)}
    assert delta == {"upload": 1, "tracks_step": 1}
    # step 2: lane 2's first frame on the existing path among two tracking lanes
    delta = {k: v - steps[1][1].get(k, 0) for k, v in steps[2][1].items() if v != steps[1][1].get(k, 0)}
    assert delta == {"upload": 1, "fast": 1, "stereo_match": 1, "undistort": 1, "tracks_put": 1, "tracks_step": 1}
