"""mfe_stereo_match and mfe_fast_grid (include/msckf_pipeline.h; k_stereo_match_sets,
k_mask_clear_sets, k_row_scan_sets, k_grid_select_sets, each run with one set) on
small images: 150 x 110 (no multiple of 16 or 64, ragged last grid cells) and the
376 x 240 scenes of
tests/golden/frontend_ref.npz.

fast_grid against the reference tests/frontend_pipeline_ref.py, bit-exact on
xy, response, cell_count and n_total (integer work).

stereo_match
  * against the composed device path (Frontend.undistort, distort, lk, lk as
    ImageProcessor.stereo_match calls them): cam1_pts and the forward status
    bit-equal on every point, at 0, 1, 63, 64, 65 and 257 points;
  * against the CPU reference: cam1_pts within 1e-4 px (the bar of
    test_lk_matches_oracle_and_motion), inlier and reason identical on every
    point whose margins are >= 1e-3 px (>= 1e-6 relative for the epipolar
    test); no case may exclude more than 1 % of its points.  The cases of
    STEREO_CASES were run through the reference alone on the CPU when they
    were chosen: none of them excludes a point (every margin of every point is
    above the limits), so the cap holds with room.  Reasons reached, with the
    case that reaches each:
      0  every case
      1  flat (points on a textureless region: forward LK status 0),
         fisheye_reject (the rejected solution's (-1e6, -1e6) guess), border
      2  vshift25 (round trip >= 3 px where the match is lost)
      3  vshift25 (cam1 shifted vertically by 25 px)
      4  border (points at the left edge whose match leaves the image)
      5  euroc_vshift (EuRoC extrinsics, cam1 shifted vertically by 3 px, at
         stereo_threshold = 1: with the reference's quirk the error is
         |u1.x line.x| / |line|, which does not see the shift itself),
         fisheye_reject
    and for the pure x baseline of rect line.x = 0, so test 5 is vacuous: the
    test asserts that no point of those cases has reason 5 even at
    stereo_threshold = 0.

ImageProcessor(device_pipeline=True) on both golden scenes: ids identical to
the recorded reference frames, coordinates within 1e-4 px, every message bit
for bit that of a second ImageProcessor with the switch off, and the same with
ransac_enabled.  Two identical calls of each entry point return the same bits."""
import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
from conftest import golden
from frontend_ref_scenes import scene_config, run_scene, reference_frames
from oracle import frontend_oracle as fo
import frontend_synth as fs
import frontend_pipeline_ref as pr

pytestmark = pytest.mark.gpu
LK = dict(win=15, max_level=3, max_iter=30, eps=0.01)


# ------------------------------------------------------------------ scenes --
def extrinsics(T_imu_cam0, T_imu_cam1):
    """R_cam0_cam1 and E as ImageProcessor.stereo_match forms them."""
    T0, T1 = fe_mod._inv_T(T_imu_cam0), fe_mod._inv_T(T_imu_cam1)
    R = T1[:3, :3].T @ T0[:3, :3]
    t = T1[:3, :3].T @ (T0[:3, 3] - T1[:3, 3])
    return R, fe_mod._skew(t) @ R


def cameras(kind):
    g = golden("frontend_ref")
    if kind == "rect":
        K = g["rectified_intrinsics"]
        R, E = extrinsics(g["rectified_T_imu_cam0"], g["rectified_T_imu_cam1"])
        return (K, 0, np.zeros(4)), (K, 0, np.zeros(4)), R, E
    R, E = extrinsics(g["euroc_T_imu_cam0"], g["euroc_T_imu_cam1"])
    K0, K1 = g["euroc_intrinsics"], g["euroc_intrinsics1"]
    if kind == "euroc":
        return (K0, 0, g["euroc_distortion"]), (K1, 0, g["euroc_distortion1"]), R, E
    k = np.array([0.01, -0.005, 0.001, -0.0002]) if kind == "fisheye" else np.array([-1.0, 0.0, 0.0, 0.0])
    return (K0, 1, k), (K1, 1, k), np.eye(3), E      # equidistant: the reference never rectifies the guess


def scene_points(img, n, seed, extra=()):
    xy, _ = fo.fast_detect(img, 15)
    H, W = img.shape
    xy = xy[(xy[:, 0] > 24) & (xy[:, 0] < W - 24) & (xy[:, 1] > 24) & (xy[:, 1] < H - 24)]
    rng = np.random.default_rng(seed)
    pts = xy[rng.choice(len(xy), n, replace=False)].astype(float) + rng.uniform(-0.4, 0.4, (n, 2))
    return np.concatenate([pts, np.asarray(extra, float).reshape(-1, 2)])


def make_case(name):
    """(img0, img1, pts, cam0, cam1, R_guess, E, stereo_threshold, lk)."""
    W, H, lk = 376, 240, dict(LK)
    if name == "small":                       # 150 x 110, 3 pyramid levels
        W, H, lk["max_level"] = 150, 110, 2
    f = fs.texture_fn({"small": 11, "flat": 5}.get(name, 7), W=W, H=H)
    kind = {"euroc_vshift": "euroc", "fisheye": "fisheye", "fisheye_reject": "reject"}.get(name, "rect")
    cam0, cam1, R, E = cameras(kind)
    disp, vshift, thr, n, extra = 12.0, 0.0, 5.0, 96, []
    if name == "small":
        disp, n = 5.0, 60
        cam0 = cam1 = (np.array([90.0, 90.0, 75.0, 55.0]), 0, np.zeros(4))
    elif name == "border":
        extra = [[4.0, 60.0], [6.5, 120.25], [9.0, 200.0], [11.5, 30.5], [370.0, 100.0], [200.0, 3.0]]
    elif name == "euroc_vshift":
        disp, vshift, thr = 9.0, 3.0, 1.0
    elif name == "vshift25":
        vshift = 25.0
    elif name in ("fisheye", "fisheye_reject"):
        disp = 9.0
    img0 = fs.render(f, W, H)
    img1 = fs.render(f, W, H, -disp, vshift)
    if name == "flat":
        img0 = img0.copy()
        img0[60:180, 100:280] = 128
        img1 = img1.copy()
        img1[60:180, 88:268] = 128
        extra = [[x, y] for x in (140.0, 190.5, 240.0) for y in (100.0, 120.25, 140.0)]
        n = 60
    return img0, img1, scene_points(img0, n, 1, extra), cam0, cam1, R, E, thr, lk


STEREO_CASES = ("rect", "border", "small", "euroc_vshift", "vshift25", "flat", "fisheye", "fisheye_reject")
EXPECT_REASONS = {"rect": {0}, "border": {0, 1, 4}, "small": {0}, "euroc_vshift": {0, 5}, "vshift25": {0, 2, 3},
                  "flat": {0, 1}, "fisheye": {0}, "fisheye_reject": {0, 1, 5}}
_ctx = {}


def frontend(W, H):
    """One device context per image size, shared by the module's tests."""
    if (W, H) not in _ctx:
        _ctx[(W, H)] = fe_mod.Frontend(W, H, nslot=2, max_level=3, max_points=1024)
    return _ctx[(W, H)]


def teardown_module(module):
    for c in _ctx.values():
        c.close()
    _ctx.clear()


# ------------------------------------------------------------ stereo_match --
def composed(fe, pts, cam0, cam1, R, lk):
    """ImageProcessor.stereo_match's device calls up to the forward LK."""
    und = fe.undistort(pts, cam0[0], cam0[1], cam0[2], R, [1, 1, 0, 0])
    g = fe.distort(und, cam1[0], cam1[1], cam1[2])
    c0 = np.asarray(pts, float).reshape(-1, 2).astype(np.float32)
    c1, st = fe.lk(0, 1, c0, g.astype(np.float32), **lk)
    back, _ = fe.lk(1, 0, c1, c0.copy(), **lk)
    return c1, st, back, g


@pytest.mark.parametrize("name", STEREO_CASES)
def test_stereo_match_vs_reference(name):
    img0, img1, pts, cam0, cam1, R, E, thr, lk = make_case(name)
    fe = frontend(img0.shape[1], img0.shape[0])
    fe.upload(0, img0)
    fe.upload(1, img1)
    c1, inl, rsn = fe.stereo_match(0, 1, pts, cam0, cam1, R, E, thr, **lk)
    rc1, rinl, rrsn, mg = pr.stereo_match(img0, img1, pts, cam0, cam1, R, E, thr, **lk)
    clear = pr.clear_of_thresholds(mg)
    dev = np.abs(c1.astype(float) - rc1.astype(float)).max()
    print("%s: %d points, %d excluded, reasons %s, worst |cam1_pts - reference| = %.2e px"
          % (name, len(pts), int((~clear).sum()), sorted(set(rrsn.tolist())), dev))
    assert (~clear).sum() <= 0.01 * len(pts)
    assert dev <= 1e-4
    np.testing.assert_array_equal(rsn[clear], rrsn[clear])
    np.testing.assert_array_equal(inl[clear], rinl[clear])
    np.testing.assert_array_equal(inl, (rsn == 0).astype(np.uint8))
    assert EXPECT_REASONS[name] <= set(rrsn.tolist())
    # against the composed device path: bit-equal positions and forward status
    cc1, st, _, _ = composed(fe, pts, cam0, cam1, R, lk)
    np.testing.assert_array_equal(c1, cc1)
    np.testing.assert_array_equal(rsn != 1, st.astype(bool))
    # two identical calls: the same bits
    again = fe.stereo_match(0, 1, pts, cam0, cam1, R, E, thr, **lk)
    for a, b in zip((c1, inl, rsn), again):
        np.testing.assert_array_equal(a, b)
    if cam0[1] == 0 and name != "euroc_vshift":   # pure x baseline: line.x = 0, test 5 cannot fail
        assert np.all(E[0] == 0)
        _, _, rsn0 = fe.stereo_match(0, 1, pts, cam0, cam1, R, E, 0.0, **lk)
        assert 5 not in rsn0 and 5 not in pr.stereo_match(img0, img1, pts, cam0, cam1, R, E, 0.0, **lk)[2]
        np.testing.assert_array_equal(rsn0, rsn)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("kind", ["euroc", "fisheye"])
def test_stereo_match_vs_composed_path(kind, n):
    W, H = 376, 240
    f = fs.texture_fn(7, W=W, H=H)
    img0, img1 = fs.render(f, W, H), fs.render(f, W, H, -9.0, 1.0)
    cam0, cam1, R, E = cameras(kind)
    rng = np.random.default_rng(n)
    pts = rng.uniform([-2, -2], [W + 2, H + 2], (n, 2))      # a few outside the image
    fe = frontend(W, H)
    fe.upload(0, img0)
    fe.upload(1, img1)
    c1, inl, rsn = fe.stereo_match(0, 1, pts, cam0, cam1, R, E, 5.0, **LK)
    cc1, st, back, g = composed(fe, pts, cam0, cam1, R, LK)
    assert c1.shape == (n, 2) and inl.shape == rsn.shape == (n,)
    np.testing.assert_array_equal(c1, cc1)
    np.testing.assert_array_equal(rsn != 1, st.astype(bool))
    # tests 2-4 from the composed path's own numbers, as ImageProcessor.stereo_match applies them
    c0 = pts.astype(np.float32)
    err = np.linalg.norm(c0 - back, axis=1) if n else np.zeros(0)
    want = np.where(st == 0, 1, np.where(~(err < 3), 2, np.where(~(np.abs(g[:, 1] - c1[:, 1]) < 20), 3, np.where(
        (c1[:, 0] < 0) | (c1[:, 0] > W - 1) | (c1[:, 1] < 0) | (c1[:, 1] > H - 1), 4, 0))))
    np.testing.assert_array_equal(np.where(rsn == 5, 0, rsn), want)
    if n:
        assert (rsn == 0).sum() >= 0.5 * n


# --------------------------------------------------------------- fast_grid --
def grid_image(W, H, seed=3):
    """Texture with a flat band on the right (empty cells) and a sparse top-left
    corner (cells with few candidates)."""
    img = fs.render(fs.texture_fn(seed, W=W, H=H), W, H).copy()
    img[:, int(0.8 * W):] = 90
    img[:H // 4, :W // 5] = 60
    img[10:16, 8:14] = 220
    return img


def check_fast_grid(fe, img, occ, rows, cols, k, **kw):
    xy, resp, cnt, n = fe.fast_grid(0, 15, occ, rows, cols, k, **kw)
    rxy, rresp, rcnt, rn = pr.fast_grid(img, 15, occ, rows, cols, k)
    assert n == rn
    np.testing.assert_array_equal(cnt, rcnt)
    np.testing.assert_array_equal(xy, rxy)
    np.testing.assert_array_equal(resp, rresp)
    xy2, resp2, cnt2, n2 = fe.fast_grid(0, 15, occ, rows, cols, k, **kw)     # the same bits again
    assert n2 == n and (xy2 == xy).all() and (resp2 == resp).all() and (cnt2 == cnt).all()
    return xy, resp, cnt, n


def occupied_points(img, n_occ, seed):
    """n_occ occupied points: detected corners (so that the mask removes
    keypoints) and the four edge bands x < 3, y < 3, x >= W - 4, y >= H - 4."""
    H, W = img.shape
    xy, _ = fo.fast_detect(img, 15)
    rng = np.random.default_rng(seed)
    edge = np.array([[1.5, 40.0], [2.9, 2.9], [50.0, 0.0], [60.25, 2.0], [W - 4.0, 30.0], [W - 0.5, 70.5],
                     [33.0, H - 4.0], [80.0, H - 1.0], [W - 1.0, H - 1.0], [3.0, 3.0]])
    pick = xy[rng.choice(len(xy), max(n_occ - len(edge), 0), replace=False)] + rng.uniform(0, 0.99, (max(n_occ - len(edge), 0), 2))
    return np.concatenate([edge, pick])[:n_occ].astype(np.float32) if n_occ > 1 else (
        (xy[len(xy) // 2:len(xy) // 2 + n_occ] + 0.5).astype(np.float32))


@pytest.mark.parametrize("n_occ", [0, 1, 63, 64, 65, 300])
def test_fast_grid_occupied_counts(n_occ):
    W, H = 150, 110
    img = grid_image(W, H)
    fe = frontend(W, H)
    fe.upload(0, img)
    occ = occupied_points(img, n_occ, n_occ)
    assert len(occ) == n_occ
    xy, resp, cnt, n = check_fast_grid(fe, img, occ, 4, 5, 5)
    free = pr.fast_grid(img, 15, np.zeros((0, 2)), 4, 5, 5)[3]
    assert (n < free) if n_occ else (n == free)                   # the mask removed keypoints
    assert (cnt == 0).any() and n > 0                              # an empty cell (the flat band)
    assert (cnt > 5).any() or n_occ == 300                         # a cell above k (300 points mask most corners)


@pytest.mark.parametrize("W,H,rows,cols,k", [(150, 110, 4, 5, 1), (150, 110, 4, 5, 16), (150, 110, 1, 1, 5),
                                             (150, 110, 1, 1, 16), (150, 110, 3, 7, 3), (376, 240, 4, 5, 5),
                                             (96, 257, 4, 5, 5), (96, 300, 4, 5, 5), (96, 513, 4, 5, 5)])
def test_fast_grid_grids(W, H, rows, cols, k):
    """H > 256: the row scan gives each of its 256 threads 2 rows (H = 257: thread
    128 a single one; H = 300: the threads from 150 on none) or 3 (H = 513)."""
    img = fs.render(fs.texture_fn(7, W=W, H=H), W, H) if W == 376 else grid_image(W, H)
    if W == 96 and (W, H) not in _ctx:                             # a narrow image holds no level above 0
        _ctx[(W, H)] = fe_mod.Frontend(W, H, nslot=2, max_level=0, max_points=1024)
    fe = frontend(W, H)
    fe.upload(0, img)
    occ = occupied_points(img, 40, 1)
    xy, resp, cnt, n = check_fast_grid(fe, img, occ, rows, cols, k)
    assert cnt.sum() == n and len(xy) == np.minimum(cnt, k).sum() > 0
    assert H % rows or W % cols or (rows, cols) == (1, 1)          # ragged last cells
    if H > 256:                       # keypoints in the last row of cells, and from row 256 on where a corner can be
        ry = pr.fast_grid(img, 15, occ, rows, cols, k)[0][:, 1]
        assert (ry >= (rows - 1) * -(-H // rows)).any() and ((ry >= 256).any() or H - 3 <= 256)


def test_fast_grid_cell_fill_and_tie():
    """Single bright pixels on a dark image (each a corner that survives the
    non-max suppression, its response set by its brightness) in a 2 x 2 grid at
    k = 3: a cell with exactly k candidates, one with more, one with fewer and
    an empty one; in the cell with more, two equal responses compete for the
    last place and the earlier in raster order gets it."""
    W, H = 150, 110
    spots = [(10, 8, 200), (40, 30, 120), (70, 50, 160),                                        # cell 0: 3
             (80, 5, 100), (140, 20, 160), (100, 25, 200), (90, 40, 160), (120, 52, 180),       # cell 1: 5
             (30, 100, 90)]                                                                     # cell 2: 1
    img = np.full((H, W), 40, np.uint8)
    for x, y, v in spots:
        img[y, x] = v
    fe = frontend(W, H)
    fe.upload(0, img)
    none = np.zeros((0, 2), np.float32)
    xy, resp, cnt, n = check_fast_grid(fe, img, none, 2, 2, 3)
    assert n == len(spots) and cnt.tolist() == [3, 5, 1, 0]
    np.testing.assert_array_equal(xy, [[10, 8], [70, 50], [40, 30], [100, 25], [120, 52], [140, 20], [30, 100]])
    assert resp[5] == resp[1] and len(xy) == 7          # (90, 40), the later of the tie, did not fit
    xy, resp, cnt, _ = check_fast_grid(fe, img, none, 1, 1, 1)
    np.testing.assert_array_equal(xy, [[10, 8]])        # 200 occurs twice: (10, 8) is the earlier in raster order
    check_fast_grid(fe, img, np.array([[100.5, 25.5], [10.0, 8.0]], np.float32), 2, 2, 3)


def test_fast_grid_overflow_is_an_error():
    W, H = 150, 110
    img = grid_image(W, H)
    fe = frontend(W, H)
    fe.upload(0, img)
    n = pr.fast_grid(img, 15, np.zeros((0, 2)), 4, 5, 5)[3]
    assert n > 64
    check_fast_grid(fe, img, np.zeros((0, 2)), 4, 5, 5, max_kp=n)             # exactly at the capacity
    for cap in (n - 1, 64, 1):
        xy = np.zeros((100, 2), np.float32)
        resp = np.zeros(100, np.float32)
        cnt = np.full(20, -7, np.int32)
        tot = fe_mod.C.c_int(0)
        fp = fe_mod.C.POINTER(fe_mod.C.c_float)
        rc = fe.lib.mfe_fast_grid(fe.h, 0, 15, 0, None, 4, 5, 5, cap, xy.ctypes.data_as(fp), resp.ctypes.data_as(fp),
                                  cnt.ctypes.data_as(fe_mod.C.POINTER(fe_mod.C.c_int32)), fe_mod.C.byref(tot))
        assert rc < 0 and tot.value == n
        assert (cnt == -7).all() and not xy.any() and not resp.any()          # never a truncated selection
        with pytest.raises(_lib.MsckfError):
            fe.fast_grid(0, 15, np.zeros((0, 2)), 4, 5, 5, max_kp=cap)
    assert pr.fast_grid(img, 15, np.zeros((0, 2)), 4, 5, 5, max_kp=n - 1)[0] is None


# ---------------------------------------------------------- ImageProcessor --
@pytest.fixture(scope="module")
def scene_runs():
    """Each golden scene run once with the switch off and once with it on."""
    g = golden("frontend_ref")
    out = {}
    for name in ("rectified", "euroc"):
        for on in (False, True):
            cfg = scene_config(g, name)
            cfg.device_pipeline = on
            ip = fe_mod.ImageProcessor(cfg)
            out[name, on] = run_scene(ip, g, name)
            ip.fe.close()
    return g, out


@pytest.mark.parametrize("name", ["rectified", "euroc"])
def test_image_processor_device_pipeline(name, scene_runs):
    g, runs = scene_runs
    fx = np.array([g[name + "_intrinsics"][0], g[name + "_intrinsics"][1],
                   g[name + "_intrinsics1"][0], g[name + "_intrinsics1"][1]])
    on, off = runs[name, True], runs[name, False]
    assert len(on) == len(off) == int(g[name + "_frames"])
    for k, ((ids, uv), (oids, ouv), (rids, ruv)) in enumerate(zip(on, off, reference_frames(g, name))):
        np.testing.assert_array_equal(ids, rids, err_msg="frame %d" % k)
        assert (np.abs(uv - ruv) * fx).max() <= 1e-4, k
        np.testing.assert_array_equal(ids, oids, err_msg="frame %d" % k)
        assert uv.tobytes() == ouv.tobytes(), k                               # bit for bit


@pytest.mark.parametrize("name", ["rectified", "euroc"])
def test_image_processor_device_pipeline_with_ransac(name):
    g = golden("frontend_ref")
    got = []
    for on in (False, True):
        cfg = scene_config(g, name)
        cfg.ransac_enabled, cfg.device_pipeline = True, on
        ip = fe_mod.ImageProcessor(cfg)
        got.append(run_scene(ip, g, name))
        ip.fe.close()
    for k, ((ids, uv), (oids, ouv)) in enumerate(zip(*got)):
        np.testing.assert_array_equal(ids, oids, err_msg="frame %d" % k)
        assert uv.tobytes() == ouv.tobytes(), k
    assert len(got[0][-1][0]) >= 30
