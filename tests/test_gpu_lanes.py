"""The set calls of include/msckf_lanes.h (mfe_upload_many, mfe_lk_sets,
mfe_stereo_match_sets, mfe_fast_grid_sets, mfe_undistort_sets) and
MultiImageProcessor on the device.

Every operator has one kernel, the set form, and a single-stream call is that
kernel run with one set.  The single calls are pinned to the oracle and the
reference by tests/test_gpu_frontend.py and tests/test_gpu_pipeline.py, which
so exercise the set kernels directly; they are the anchor to the truth.  The
comparisons here put many sets in one call against the same kernels with one
set at a time, on the same inputs: that checks the per-set indexing (slots,
per-point set index, per-set work areas and tables), and every comparison is
bit-exact, on every point.

Per-call cases: 150 x 110 images (no multiple of 16 or 64), six slots holding
six different images; the set layouts of LAYOUTS -- 1, 2 and 11 sets, the sizes
0, 1, 63, 64, 65 and 257, an empty set first, in the middle and last; in the
11-set layout sets share a slot pair and use pairs reversed (PAIRS).

The single calls on the shared state: they work in set 0 of the detection's
work areas, which a set call with more sets reallocates and any detection
leaves its mask in; their result codes through ctypes.

End to end: three lanes (the two golden scenes and a third texture, one lane
with RANSAC, one started late) publish, bit for bit, what a single
ImageProcessor(device_pipeline=True) publishes on each stream."""
import ctypes as C

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from conftest import golden
from frontend_ref_scenes import SCENES, scene_config
import frontend_synth as fs
import frontend_lanes_ref as lr

pytestmark = pytest.mark.gpu
W, H, NSLOT, MAXP = 150, 110, 6, 2048
LK = dict(win=15, max_level=2, max_iter=30, eps=0.01)
LAYOUTS = {1: [257], 2: [64, 65], 11: [0, 1, 63, 64, 65, 0, 257, 1, 63, 64, 0]}
PAIRS = [(0, 1), (2, 3), (1, 0), (0, 1), (4, 5), (2, 3), (3, 2), (5, 4), (0, 1), (2, 3), (4, 5)]
CAMS = [0, 1, 2, 3, 1, 1, 2, 3, 0, 1, 2]          # camera(kind) of each set in the stereo test
_state = {}


def scene_images():
    """Six images: slots (0, 1) a stereo pair of 5 px disparity, (2, 3) a pair
    whose cam1 is also 25 px lower (round trip and vertical-disparity failures),
    (4, 5) a pair 3 px lower with a flat patch (LK failures; the epipolar test
    under EuRoC-like extrinsics)."""
    imgs = []
    for seed, vshift in ((11, 0.0), (12, 25.0), (13, 3.0)):
        f = fs.texture_fn(seed, W=W, H=H)
        imgs += [fs.render(f, W, H), fs.render(f, W, H, -5.0, vshift)]
    imgs[4], imgs[5] = imgs[4].copy(), imgs[5].copy()
    imgs[4][40:80, 60:110] = 128
    imgs[5][40:80, 55:105] = 128
    return imgs


def frontend():
    if "fe" not in _state:
        _state["fe"] = fe_mod.Frontend(W, H, nslot=NSLOT, max_level=LK["max_level"], max_points=MAXP)
        _state["imgs"] = scene_images()
    fe = _state["fe"]
    for s, im in enumerate(_state["imgs"]):      # tests that upload other images leave these behind them
        fe.upload(s, im)
    return fe, _state["imgs"]


def teardown_module(module):
    if "fe" in _state:
        _state["fe"].close()
    _state.clear()


def extrinsics(T_imu_cam0, T_imu_cam1):
    """R_cam0_cam1 and E as ImageProcessor.stereo_match forms them."""
    T0, T1 = fe_mod._inv_T(T_imu_cam0), fe_mod._inv_T(T_imu_cam1)
    R = T1[:3, :3].T @ T0[:3, :3]
    t = T1[:3, :3].T @ (T0[:3, 3] - T1[:3, 3])
    return R, fe_mod._skew(t) @ R


def camera(kind):
    """(cam0, cam1, R_guess, E, stereo_threshold): a rectified radtan pair, a
    distorted radtan pair under the EuRoC extrinsics at a tight threshold, an
    equidistant pair, and an equidistant pair whose solution is rejected."""
    g = golden("frontend_ref")
    K0, K1 = np.array([90.0, 90.0, 75.0, 55.0]), np.array([91.0, 89.5, 74.0, 56.0])
    if kind == 0:
        R, E = extrinsics(g["rectified_T_imu_cam0"], g["rectified_T_imu_cam1"])
        return (K0, 0, np.zeros(4)), (K0, 0, np.zeros(4)), R, E, 5.0
    R, E = extrinsics(g["euroc_T_imu_cam0"], g["euroc_T_imu_cam1"])
    if kind == 1:
        return (K0, 0, g["euroc_distortion"]), (K1, 0, g["euroc_distortion1"]), R, E, 0.3
    k = np.array([0.01, -0.005, 0.001, -0.0002]) if kind == 2 else np.array([-1.0, 0.0, 0.0, 0.0])
    return (K0, 1, k), (K1, 1, k), np.eye(3), E, 3.0      # equidistant: the reference never rectifies the guess


def points(n, seed):
    """n points over the image, a few outside it, and some on the left edge
    (their match leaves the image) and in the flat patch of slots 4, 5."""
    rng = np.random.default_rng(seed)
    p = rng.uniform([-2, -2], [W + 2, H + 2], (n, 2))
    extra = np.array([[3.5, 60.0], [4.0, 30.25], [85.0, 60.0], [90.5, 55.25], [2.0, 80.0], [80.0, 65.5]])
    m = min(n // 8, len(extra))
    p[:m] = extra[:m]
    return p


def layout_sets(n_sets):
    return [(PAIRS[i], points(n, 100 * n_sets + i)) for i, n in enumerate(LAYOUTS[n_sets])]


# -------------------------------------------------------------- upload_many --
def slot_results(fe, slots):
    a, b, c = slots
    cam0, cam1, R, E, thr = camera(1)
    p = points(65, 5)
    out = [fe.fast(s, 15) for s in slots]
    out += [fe.lk(a, b, p.astype(np.float32), p.astype(np.float32) + 0.5, **LK),
            fe.lk(c, a, p.astype(np.float32), p.astype(np.float32), **LK),
            fe.stereo_match(b, c, p, cam0, cam1, R, E, thr, **LK)]
    return [np.asarray(x) for r in out for x in r]


def test_upload_many_equals_upload():
    fe, imgs = frontend()
    slots = [4, 0, 2]                                   # not contiguous, not ascending
    new = [imgs[1], imgs[3], imgs[0]]                   # other images than the slots hold
    for s, im in zip(slots, new):
        fe.upload(s, im)
    want = slot_results(fe, slots)
    for s in slots:
        fe.upload(s, np.zeros((H, W), np.uint8))
    assert any((a != b).any() if a.shape == b.shape else True for a, b in zip(slot_results(fe, slots), want))
    fe.upload_many(slots, np.stack(new))
    got = slot_results(fe, slots)
    assert len(got) == len(want) and len(want[0]) > 20
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # a repeated slot: an error, and the slots keep what they hold
    with pytest.raises(_lib.MsckfError):
        fe.upload_many([4, 1, 4], np.stack([imgs[5], imgs[5], imgs[5]]))
    with pytest.raises(_lib.MsckfError):
        fe.upload_many([0, NSLOT], np.stack([imgs[5], imgs[5]]))
    for a, b in zip(slot_results(fe, slots), want):
        np.testing.assert_array_equal(a, b)
    # all six at once, then the untouched single path on them
    fe.upload_many(list(range(NSLOT)), np.stack(imgs))
    q, st = fe.lk(0, 1, points(64, 1).astype(np.float32), points(64, 1).astype(np.float32), **LK)
    fe.upload(0, imgs[0])
    fe.upload(1, imgs[1])
    q1, st1 = fe.lk(0, 1, points(64, 1).astype(np.float32), points(64, 1).astype(np.float32), **LK)
    np.testing.assert_array_equal(q, q1)
    np.testing.assert_array_equal(st, st1)


# ------------------------------------------------------------------ lk_sets --
@pytest.mark.parametrize("n_sets", [1, 2, 11])
def test_lk_sets_equal_lk(n_sets):
    fe, _ = frontend()
    sets = []
    for (a, b), p in layout_sets(n_sets):
        p = p.astype(np.float32)
        sets.append((a, b, p, p + np.float32(0.75)))
    got = fe.lk_sets(sets, **LK)
    assert len(got) == n_sets
    tracked = 0
    for s, (q, st) in zip(sets, got):
        rq, rst = fe.lk(*s, **LK)
        assert q.shape == rq.shape and st.shape == rst.shape == (len(s[2]),)
        np.testing.assert_array_equal(q, rq)
        np.testing.assert_array_equal(st, rst)
        tracked += int(st.sum())
    assert tracked > 0
    for (q, st), (q2, st2) in zip(got, fe.lk_sets(sets, **LK)):       # the same bits again
        assert (q == q2).all() and (st == st2).all()


# -------------------------------------------------------- stereo_match_sets --
@pytest.mark.parametrize("n_sets", [1, 2, 11])
def test_stereo_match_sets_equal_stereo_match(n_sets):
    fe, _ = frontend()
    sets = [(a, b, p) + camera(CAMS[i]) for i, ((a, b), p) in enumerate(layout_sets(n_sets))]
    got = fe.stereo_match_sets(sets, **LK)
    assert len(got) == n_sets
    reasons = set()
    for s, (c1, inl, rsn) in zip(sets, got):
        rc1, rinl, rrsn = fe.stereo_match(*s, **LK)
        assert c1.shape == rc1.shape and inl.shape == rsn.shape == (len(s[2]),)
        np.testing.assert_array_equal(c1, rc1)
        np.testing.assert_array_equal(inl, rinl)
        np.testing.assert_array_equal(rsn, rrsn)
        reasons |= set(rrsn.tolist())
    if n_sets == 11:      # radtan and equidistant sets with different E, R_guess and thresholds in one call
        assert reasons == {0, 1, 2, 3, 4, 5}
        assert {s[3][1] for s in sets} == {0, 1} and len({s[7] for s in sets}) == 3
    for a, b in zip(got, fe.stereo_match_sets(sets, **LK)):
        for x, y in zip(a, b):
            assert (x == y).all()


# ----------------------------------------------------------- fast_grid_sets --
def grid_images(W=W, H=H):
    """Six images for detection: textures with a flat band and a sparse corner,
    and one of single bright pixels (few keypoints)."""
    imgs = []
    for seed in (3, 4, 5, 6, 7):
        img = fs.render(fs.texture_fn(seed, W=W, H=H), W, H).copy()
        img[:, int(0.8 * W):] = 90
        img[:H // 4, :W // 5] = 60
        imgs.append(img)
    dots = np.full((H, W), 40, np.uint8)
    for x, y, v in [(10, 8, 200), (40, 30, 120), (70, 50, 160), (80, 5, 100), (140, 20, 160), (100, 25, 200),
                    (90, 40, 160), (120, 52, 180), (30, 100, 90)]:
        if x < W:
            dots[y, x] = v
    return imgs + [dots]


def occupied(fe, slot, n, seed, W=W, H=H):
    """n occupied points: detected corners of the slot's image (so that the mask
    removes keypoints) and points in the edge bands."""
    xy, _ = fe.fast(slot, 15)
    rng = np.random.default_rng(seed)
    edge = np.array([[1.5, 40.0], [2.9, 2.9], [W - 0.5, 70.5], [80.0, H - 1.0], [3.0, 3.0]])
    pick = xy[rng.integers(0, len(xy), n)] + rng.uniform(0, 0.99, (n, 2))
    return np.concatenate([pick[:max(n - len(edge), 1)], edge])[:n].astype(np.float32)


OCC = {1: [300], 2: [1, 0], 3: [300, 0, 65], 11: [0, 1, 300, 63, 64, 0, 65, 257, 1, 300, 0]}
# (n_sets, rows, cols, k, image rows): above 256 image rows k_row_scan_sets gives a thread two rows
GRID_SETS = [(1, 4, 5, 5, H), (2, 4, 5, 5, H), (11, 4, 5, 1, H), (11, 4, 5, 16, H), (11, 1, 1, 1, H), (11, 1, 1, 16, H),
             (1, 4, 5, 5, 300), (3, 4, 5, 5, 300)]


@pytest.mark.parametrize("n_sets,rows,cols,k,Hi", GRID_SETS,
                         ids=["-".join(str(v) for v in (c[:4] if c[4] == H else c)) for c in GRID_SETS])
def test_fast_grid_sets_equal_fast_grid(n_sets, rows, cols, k, Hi):
    if Hi == H:
        fe, Wi = frontend()[0], W
    else:                                            # 96 x 300: a narrow image holds no level above 0
        fe, Wi = fe_mod.Frontend(96, Hi, nslot=NSLOT, max_level=0, max_points=MAXP), 96
    try:
        fe.upload_many(list(range(NSLOT)), np.stack(grid_images(Wi, Hi)))
        slots = [(5 * i + 1) % NSLOT for i in range(n_sets)]          # 1 0 5 4 3 2 1 ...: every image, repeats
        sets = [(s, occupied(fe, s, n, i, Wi, Hi)) for i, (s, n) in enumerate(zip(slots, OCC[n_sets]))]
        assert [len(o) for _, o in sets] == OCC[n_sets]
        got = fe.fast_grid_sets(sets, 15, rows, cols, k)
        assert len(got) == n_sets
        for (s, occ), (xy, resp, cnt, n) in zip(sets, got):
            rxy, rresp, rcnt, rn = fe.fast_grid(s, 15, occ, rows, cols, k)
            assert n == rn and cnt.sum() == n
            np.testing.assert_array_equal(cnt, rcnt)
            np.testing.assert_array_equal(xy, rxy)
            np.testing.assert_array_equal(resp, rresp)
        for a, b in zip(got, fe.fast_grid_sets(sets, 15, rows, cols, k)):     # two consecutive calls: the same bits
            assert a[3] == b[3] and all((x == y).all() for x, y in zip(a[:3], b[:3]))
        if n_sets == 11:
            free = fe.fast_grid(slots[2], 15, np.zeros((0, 2)), rows, cols, k)[3]
            assert got[2][3] < free                                           # 300 occupied points masked keypoints
        if Hi > 256:                                 # keypoints from row 256 on, in the last row of cells
            assert all((xy[:, 1] >= 256).any() for xy, _, _, _ in got[:1])
    finally:
        if Hi != H:
            fe.close()


def test_fast_grid_sets_overflow_is_an_error():
    fe, _ = frontend()
    fe.upload_many(list(range(NSLOT)), np.stack(grid_images()))
    none = np.zeros((0, 2), np.float32)
    totals = [fe.fast_grid(s, 15, none, 4, 5, 5)[3] for s in (5, 0, 5)]
    assert totals[0] < 64 < totals[1]                     # the dots fit, the texture does not
    sl = np.array([5, 0, 5], np.int32)
    off = np.zeros(4, np.int32)
    xy, resp = np.zeros((3, 100, 2), np.float32), np.zeros((3, 100), np.float32)
    cnt, tot = np.full((3, 20), -7, np.int32), np.full(3, -7, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    call = lambda cap: fe.lib.mfe_fast_grid_sets(
        fe.h, 3, sl.ctypes.data_as(ip), off.ctypes.data_as(ip), None, 15, 4, 5, 5, cap, xy.ctypes.data_as(fp),
        resp.ctypes.data_as(fp), cnt.ctypes.data_as(ip), tot.ctypes.data_as(ip))
    assert call(64) == -3
    assert tot.tolist() == totals                          # every n_total set ...
    assert (cnt == -7).all() and not xy.any() and not resp.any()      # ... and nothing else written
    with pytest.raises(_lib.MsckfError):
        fe.fast_grid_sets([(5, none), (0, none), (5, none)], 15, 4, 5, 5, max_kp=64)
    assert call(max(totals)) == 0 and (cnt >= 0).all() and cnt.sum(axis=1).tolist() == totals


# ----------------------------------------------------------- undistort_sets --
def undistort_set(i, p):
    """Radtan (i % 4 < 2) and equidistant sets, with and without a rectification and new intrinsics."""
    cam0, cam1, R, _, _ = camera(i % 4)
    cam = cam0 if i % 2 else cam1
    Rr = None if i % 3 == 0 else R
    nK = None if i % 5 == 0 else np.array([88.0 + i, 87.0, 70.0, 50.0 + i])
    return (p, cam[0], cam[1], cam[2], Rr, nK)


@pytest.mark.parametrize("n_sets", [1, 2, 11])
def test_undistort_sets_equal_undistort(n_sets):
    fe, _ = frontend()
    first = {1: 3, 2: 1, 11: 0}[n_sets]                   # 1 set: the equidistant model whose solutions are rejected
    sets = [undistort_set(first + i, p) for i, (_, p) in enumerate(layout_sets(n_sets))]
    got = fe.undistort_sets(sets)
    rejected = 0
    for s, out in zip(sets, got):
        ref = fe.undistort(*s)
        assert out.shape == ref.shape == (len(s[0]), 2)
        assert out.tobytes() == ref.tobytes()
        rejected += int((out == -1000000.0).all(axis=1).sum())
    assert {s[2] for s in sets} == ({0, 1} if n_sets > 1 else {1})
    assert rejected > 0 if n_sets != 2 else True          # the fisheye rejection value, bit for bit
    for a, b in zip(got, fe.undistort_sets(sets)):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------ the single calls on shared state --
def test_single_calls_survive_a_grow_of_the_work_area():
    fe = fe_mod.Frontend(W, H, nslot=NSLOT, max_level=LK["max_level"], max_points=MAXP)
    try:
        for s, im in enumerate(grid_images()):
            fe.upload(s, im)
        occ = occupied(fe, 1, 65, 0)
        single = lambda: fe.fast(1, 15) + fe.fast_grid(1, 15, occ, 4, 5, 5)
        before = single()
        assert len(before[0]) > 20 and before[5] > 20
        sets = [(s, occupied(fe, s, n, i)) for i, (s, n) in enumerate(zip((0, 1, 5), OCC[3]))]
        assert len(fe.fast_grid_sets(sets, 15, 4, 5, 5)) == 3      # one set -> three: the areas are allocated again
        for a, b in zip(single(), before):
            np.testing.assert_array_equal(a, b)
    finally:
        fe.close()


def test_unmasked_fast_after_a_masked_detection():
    fe, _ = frontend()
    fe.upload_many(list(range(NSLOT)), np.stack(grid_images()))

    def same(a, b):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    r0 = fe.fast(0, 15)
    assert fe.fast_grid(0, 15, occupied(fe, 0, 300, 1), 4, 5, 5)[3] < len(r0[0])      # the mask removed keypoints
    same(fe.fast(0, 15), r0)                                  # mask = NULL is unmasked, whatever set 0's mask held
    m = np.ones((H, W), np.uint8)
    m[:, :75] = 0
    keep = r0[0][:, 0] >= 75
    assert 0 < keep.sum() < len(keep)
    same(fe.fast(0, 15, mask=m), (r0[0][keep], r0[1][keep]))
    same(fe.fast(0, 15), r0)


def test_single_calls_result_codes():
    fe, _ = frontend()
    lib, h = fe.lib, fe.h
    fp, dp, u8 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    d = lambda a: np.ascontiguousarray(a, float).ravel().ctypes.data_as(dp)
    big = MAXP + 1
    prev = np.random.default_rng(0).uniform(10, 100, (big, 2)).astype(np.float32)
    nxt0 = prev + np.float32(0.5)

    def lk(slot_next, n):
        nxt, st = nxt0.copy(), np.full(big, 9, np.uint8)
        rc = lib.mfe_lk(h, 0, slot_next, n, prev.ctypes.data_as(fp), nxt.ctypes.data_as(fp), st.ctypes.data_as(u8),
                        15, 2, 30, 0.01)
        return rc, bool((nxt == nxt0).all() and (st == 9).all())
    rc, untouched = lk(1, 10)
    assert rc == 0 and not untouched
    assert lk(NSLOT, 10) == (-1, True)                       # a bad slot: next_pts and status as passed
    assert lk(1, big) == (-1, True)                          # n above the context's max_points
    assert lk(1, 0) == (0, True)

    p = points(65, 7)
    for kind in (1, 2):                                      # radtan, equidistant
        K, model, k = camera(kind)[0]
        def und(n, R, nK):
            out = np.full((len(p), 2), -7.0)
            rc = lib.mfe_undistort(h, n, d(p), out.ctypes.data_as(dp), d(K), model, d(k), R, nK)
            return rc, out
        (rc0, a), (rc1, b) = und(len(p), None, None), und(len(p), d(np.eye(3)), d([1.0, 1.0, 0.0, 0.0]))
        assert rc0 == rc1 == 0 and a.tobytes() == b.tobytes() and (a != -7.0).all()
        rc, out = und(0, None, None)
        assert rc == 0 and (out == -7.0).all()
        out = np.full((len(p), 2), -7.0)
        assert lib.mfe_distort(h, 0, d(p), out.ctypes.data_as(dp), d(K), model, d(k)) == 0 and (out == -7.0).all()

    cam0, cam1, R, E, thr = camera(1)

    def stereo(n, model0):
        c1, inl, rsn = np.full((len(p), 2), -7, np.float32), np.full(len(p), 9, np.uint8), np.full(len(p), 9, np.uint8)
        rc = lib.mfe_stereo_match(h, 0, 1, n, d(p), d(cam0[0]), model0, d(cam0[2]), d(cam1[0]), cam1[1], d(cam1[2]),
                                  d(R), d(E), 15, 2, 30, 0.01, thr, c1.ctypes.data_as(fp), inl.ctypes.data_as(u8),
                                  rsn.ctypes.data_as(u8))
        return rc, bool((c1 == -7).all() and (inl == 9).all() and (rsn == 9).all())
    rc, untouched = stereo(len(p), cam0[1])
    assert rc == 0 and not untouched
    assert stereo(len(p), 7) == (-1, True)                   # an unknown model: the outputs untouched
    assert stereo(0, cam0[1]) == (0, True)


# ------------------------------------------------------------------- errors --
def test_bad_sets_are_errors_and_leave_the_outputs():
    fe, _ = frontend()
    fp, ip, u8 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    n = MAXP + 1
    prev = np.random.default_rng(0).uniform(10, 100, (n, 2)).astype(np.float32)
    nxt0 = prev + np.float32(0.5)

    def lk_sets(off, s0, s1):
        off, s0, s1 = (np.array(a, np.int32) for a in (off, s0, s1))
        nxt, st = nxt0.copy(), np.full(n, 9, np.uint8)
        rc = fe.lib.mfe_lk_sets(fe.h, len(s0), off.ctypes.data_as(ip), s0.ctypes.data_as(ip), s1.ctypes.data_as(ip),
                                prev.ctypes.data_as(fp), nxt.ctypes.data_as(fp), st.ctypes.data_as(u8), 15, 2, 30, 0.01)
        return rc, (nxt == nxt0).all() and (st == 9).all()

    assert lk_sets([0, 10, 20, 30], [0, 2, 4], [1, 3, 5])[0] == 0
    for case in (([0, 10, 20, 30], [0, 2, 4], [1, 3, NSLOT]),        # a bad slot in the last set
                 ([0, 10, 20, 30], [0, 2, -1], [1, 3, 5]),
                 ([0, 20, 10, 30], [0, 2, 4], [1, 3, 5]),            # set_off not monotone
                 ([1, 10, 20, 30], [0, 2, 4], [1, 3, 5]),
                 ([0, 10, 20, n], [0, 2, 4], [1, 3, 5])):            # the total above max_points
        rc, untouched = lk_sets(*case)
        assert rc < 0 and untouched, case
    # the same through the other point calls' wrappers
    cam0, cam1, R, E, thr = camera(0)
    p = points(10, 0)
    with pytest.raises(_lib.MsckfError):
        fe.stereo_match_sets([(0, 1, p, cam0, cam1, R, E, thr), (2, NSLOT, p, cam0, cam1, R, E, thr)], **LK)
    with pytest.raises(_lib.MsckfError):
        fe.stereo_match_sets([(0, 1, p, cam0, (cam1[0], 7, cam1[2]), R, E, thr)], **LK)
    with pytest.raises(_lib.MsckfError):
        fe.undistort_sets([(p, cam0[0], 0, cam0[2], None, None), (p, cam0[0], 2, cam0[2], None, None)])
    with pytest.raises(_lib.MsckfError):
        fe.fast_grid_sets([(0, p), (NSLOT, p)], 15, 4, 5, 5)
    with pytest.raises(ValueError):
        fe.undistort_sets([(np.zeros((n, 2)), cam0[0], 0, cam0[2], None, None)])
    # and the context still works
    assert fe.lk_sets([(0, 1, p.astype(np.float32), p.astype(np.float32))], **LK)[0][1].shape == (10,)


def test_create_accepts_96_slots():
    fe = fe_mod.Frontend(32, 24, nslot=_lib.MAX_SLOTS, max_level=1, max_points=16)
    img = np.arange(32 * 24, dtype=np.uint8).reshape(24, 32)
    fe.upload_many([95, 17], np.stack([img, img[::-1].copy()]))
    xy, _ = fe.fast(95, 5)
    fe.upload(3, img)
    np.testing.assert_array_equal(xy, fe.fast(3, 5)[0])
    fe.close()
    with pytest.raises(_lib.MsckfError):
        fe_mod.Frontend(32, 24, nslot=_lib.MAX_SLOTS + 1, max_level=1, max_points=16)


# --------------------------------------------------------------- end to end --
def test_three_lanes_publish_what_single_processors_publish():
    g = golden("frontend_ref")
    Wg, Hg = (int(v) for v in g["size"])
    cfgs, streams = [], []
    for name in SCENES:
        cfg = scene_config(g, name)
        cfg.device_pipeline = True
        cfgs.append(cfg)
        streams.append(lr.scene_frames(g, name))
    cfgs[0].ransac_enabled, cfgs[0].ransac_seed = True, 5
    third = scene_config(g, "rectified")                 # a third texture and motion, fewer features per cell
    third.device_pipeline, third.grid_min_feature_num = True, 2
    cfgs.append(third)
    streams.append(lr.stream_frames(fs.texture_fn(9, W=Wg, H=Hg), Wg, Hg, 5, (-1.25, 0.5), (0.0, 0.01, 0.0), 10.0))
    start = [0, 0, 2]                                    # lane 2 starts late
    want = []
    for cfg, frames in zip(cfgs, streams):
        ip = fe_mod.ImageProcessor(fe_mod.FrontendConfig(**vars(cfg)))
        out = []
        for imu, msg in frames:
            for m in imu:
                ip.imu_callback(m)
            out.append(lr.unpack(ip.stareo_callback(msg)))
        ip.fe.close()
        want.append(out)
    mp = fe_mod.MultiImageProcessor(3, lane_configs=cfgs)
    kinds, serve = [], mp._serve
    mp._serve = lambda kind, reqs: (kinds.append(kind), serve(kind, reqs))[1]
    steps = []

    def on_step(step, lanes):
        steps.append((lanes, list(kinds), dict(mp.launches)))
        del kinds[:]
    got = lr.run_lanes(mp, streams, start=start, on_step=on_step)
    mp.close()
    for lane, (a, b) in enumerate(zip(got, want)):
        assert len(a) == len(b) == len(streams[lane])
        for k, ((ids, uv), (wids, wuv)) in enumerate(zip(a, b)):
            np.testing.assert_array_equal(ids, wids, err_msg="lane %d frame %d" % (lane, k))
            assert uv.tobytes() == wuv.tobytes(), (lane, k)          # bit for bit
        assert len(a[-1][0]) >= 30
    # a step in which all three lanes track: one call per stage (lane 0 runs RANSAC)
    lanes, seq, before = steps[3][0], steps[3][1], steps[2][2]
    assert lanes == [0, 1, 2]
    assert seq == ["upload", "lk", "stereo_match", "ransac", "fast_grid", "stereo_match", "undistort"]
    delta = {k: v - before.get(k, 0) for k, v in steps[3][2].items() if v != before.get(k, 0)}
    assert delta == {"upload": 1, "lk": 1, "stereo_match": 2, "ransac": 1, "fast_grid": 1, "undistort": 1}
    # step 2: lane 2's first frame among two tracking lanes
    assert steps[2][1] == ["upload", "fast", "lk", "stereo_match", "ransac", "fast_grid", "stereo_match", "undistort"]
