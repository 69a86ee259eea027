"""mfe_two_point_ransac (include/msckf_ransac.h, k_two_point_ransac) against
the numpy reference tests/ransac_ref.py, at the smallest shapes that can go
wrong: set sizes around the wave (63, 64, 65), below the minimum (0, 1, 2, 3)
and over several waves (257), beyond one pass of the workgroup (513, 1031)
and at the per-set cap (4096); fewer, as many and more hypotheses than the
workgroup has waves (1, 7, 17, 64); several sets of different sizes, camera
models and rotations in one call, one of them empty; a pre-filter that
removes points (raw index != point index); each base column; a singular pair;
every status; a constructed tie; both distortion models.

Markers, status, n_raw, best h and best count must equal the reference
exactly; scale, unit and mean_dist to rtol 1e-10 (sums of a few hundred
doubles in another order, about 1e-13, of 4096 at the cap about 1e-12); m_refit and refit_err to rtol 1e-8.
Exact equality only means something away from the thresholds, so every case
first asserts, from the reference's own margins, that no compared quantity
came closer than 1e-6 (relative) to its threshold and that no solved system
had a condition number above 1e4 -- the seeds below were chosen on the CPU so
that this holds; a case that does not meet it fails.
"""
from collections import namedtuple

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import _lib
import frontend_synth as fs
import ransac_ref as rr

pytestmark = pytest.mark.gpu

MIN_MARGIN, MAX_COND = 1e-6, 1e4


def draws_for(n_sets, n_hyp, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, size=(n_sets, n_hyp, 2), dtype=np.uint32)


@pytest.fixture(scope="module")
def fe():
    ctx = fe_mod.Frontend(64, 64, nslot=1, max_level=0, max_points=16)
    yield ctx
    ctx.close()


def check(fe, sets, inlier_error, n_hyp, draws, label=""):
    """Device against reference for one call; returns the reference results."""
    ref = rr.ransac_sets(sets, inlier_error, n_hyp, draws)
    for s, (_, info, mg, _) in enumerate(ref):
        print("%s set %d: n=%d status=%d n_raw=%d best=(%d, %d) margin=%.2e cond=%.2e" % (
            label, s, len(sets[s][0]), info[0], info[1], info[5], info[6], mg["threshold"], mg["cond"]))
        assert mg["threshold"] >= MIN_MARGIN, "case too close to a threshold: %g" % mg["threshold"]
        assert mg["cond"] <= MAX_COND, "case ill-conditioned: %g" % mg["cond"]
    got = fe.two_point_ransac(sets, inlier_error, n_hyp, draws)
    assert len(got) == len(sets)
    for s, ((mk, gi), (rmk, ri, _, _)) in enumerate(zip(got, ref)):
        msg = "%s set %d" % (label, s)
        assert mk.dtype == bool
        np.testing.assert_array_equal(mk, rmk, err_msg=msg)
        assert (gi.status, gi.n_raw, gi.best_h, gi.best_count) == (ri[0], ri[1], ri[5], ri[6]), msg
        np.testing.assert_allclose([gi.scale, gi.unit, gi.mean_dist], ri[2:5], rtol=1e-10, atol=0, err_msg=msg)
        np.testing.assert_allclose(gi.m_refit, ri[7:10], rtol=1e-8, atol=0, err_msg=msg)
        np.testing.assert_allclose(gi.refit_err, ri[10], rtol=1e-8, atol=0, err_msg=msg)
        if ri[0] == 0:
            assert np.isfinite(ri[7:11]).all() and mk.sum() == ri[6]
    return ref


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 257])
def test_set_sizes(fe, n, model):
    g = rr.synth_correspondences(n, seed=100 + n, model=model)
    (_, info, _, _), = check(fe, [g["set"]], 3.0, 7, draws_for(1, 7, n), "n=%d" % n)
    assert info[0] == (2 if n < 3 else 0)


@pytest.mark.parametrize("n,far", [(513, 3), (1031, 40), (4096, 100)])
def test_sets_beyond_one_pass(fe, n, far):
    """More points than the workgroup has threads: the strided passes loop and
    the raw list is compacted over several 512-point chunks (with points
    removed in each); 4096 is the per-set cap."""
    g = rr.synth_correspondences(n, seed=300 + far, far=far, model=far % 2)
    (_, info, _, _), = check(fe, [g["set"]], 3.0, 7, draws_for(1, 7, n), "n=%d" % n)
    # the far matches go, and at most a gross outlier or two near the border, where undistortion stretches
    assert info[0] == 0 and n - far - 2 <= info[1] <= n - far


@pytest.mark.parametrize("n_hyp", [1, 7, 17, 64])
def test_hypothesis_counts(fe, n_hyp):
    """One wave per hypothesis, eight waves: 17 and 64 loop, 1 and 7 leave waves idle."""
    g = rr.synth_correspondences(101, seed=11, model=1)
    check(fe, [g["set"]], 3.0, n_hyp, draws_for(1, n_hyp, 40 + n_hyp), "n_hyp=%d" % n_hyp)


def multi_sets():
    spec = [(66, 0, (0.0, 0.003, 0.0), (0.25, 0.05, 0.0), 0),
            (0, 1, (0.0, 0.0, 0.0), (0.1, 0.0, 0.0), 0),
            (257, 0, (0.002, -0.001, 0.003), (-0.2, 0.1, 0.05), 6),
            (3, 1, (0.0, 0.0, 0.002), (0.0, 0.3, 0.0), 0),
            (131, 1, (-0.003, 0.001, 0.0), (0.1, -0.25, 0.1), 0)]
    K2 = np.array([380.0, 390.0, 310.0, 255.0])
    return [rr.synth_correspondences(n, seed=200 + i, model=m, rvec=r, t=t, far=far,
                                     intrinsics=K2 if i % 2 else rr.EUROC_K)["set"]
            for i, (n, m, r, t, far) in enumerate(spec)]


def test_several_sets_in_one_call(fe):
    """Different sizes (one empty), models, intrinsics and rotations per set,
    each with its own draws; set 2 loses 6 points to the pre-filter."""
    ref = check(fe, multi_sets(), 3.0, 17, draws_for(5, 17, 4), "multi")
    assert [int(r[1][0]) for r in ref] == [0, 2, 0, 0, 0]
    assert ref[2][1][1] == 251


def test_prefilter_shifts_raw_indices(fe):
    g = rr.synth_correspondences(71, seed=21, far=5)
    (mk, info, _, _), = check(fe, [g["set"]], 3.0, 7, draws_for(1, 7, 2), "prefilter")
    assert info[0] == 0 and info[1] == 66 and g["far"][1] and not mk[g["far"]].any()
    np.testing.assert_array_equal(mk, ~(g["outlier"] | g["far"]))


@pytest.mark.parametrize("base,t", [(0, (0.3, 0.0, 0.0)), (1, (0.0, 0.3, 0.0)), (2, (0.0, 0.0, 0.6))])
def test_each_base_column(fe, base, t):
    """Sideways motion leaves d.y (column 0) smallest, vertical motion d.x
    (column 1), forward motion the cross term (column 2)."""
    g = rr.synth_correspondences(90, seed=30 + base, t=t, rvec=(0.0, 0.0, 0.0), outlier_share=0.1)
    ref = rr.ransac_set(*g["set"], 3.0, 7, draws_for(1, 7, 5)[0])
    assert ref[3]["best_base"] == base and ref[1][0] == 0
    check(fe, [g["set"]], 3.0, 7, draws_for(1, 7, 5), "base %d" % base)
    (_, gi), = fe.two_point_ransac([g["set"]], 3.0, 7, draws_for(1, 7, 5))
    assert gi.m_refit[base] == 1.0


def test_singular_pair_is_skipped(fe):
    """Points 4 and 5 are the same match: the hypothesis that draws them has a
    zero determinant and is skipped, the others decide."""
    g = rr.synth_correspondences(64, seed=41, outlier_share=0.2)
    prev, curr = g["pts_prev"].copy(), g["pts_curr"].copy()
    prev[5], curr[5] = prev[4], curr[4]
    s = (prev, curr) + g["set"][2:]
    draws = draws_for(1, 7, 6)
    draws[0, 0] = [4, 0]          # i1 = 4, i2 = 5
    draws[0, 3] = [5 + 64, 62]    # i1 = 5, i2 = (5 + 1 + 62) mod 64 = 4
    (_, info, _, detail), = check(fe, [s], 3.0, 7, draws, "singular")
    assert detail["count"][0] == -1 and detail["count"][3] == -1 and info[0] == 0 and info[5] not in (0, 3)


def test_degenerate_motion(fe):
    g = rr.synth_correspondences(80, seed=5, t=(0.0, 0.0, 0.0), rvec=(0.002, -0.003, 0.001), noise=0.1,
                                 outlier_share=0.025)
    (mk, info, _, _), = check(fe, [g["set"]], 3.0, 7, draws_for(1, 7, 0), "degenerate")
    assert info[0] == 1 and mk.sum() == 78


def test_prefilter_leaves_too_few(fe):
    g = rr.synth_correspondences(7, seed=8, far=2, outlier_share=0.0)
    s = tuple(a[:5] if i < 2 else a for i, a in enumerate(g["set"]))   # points 1 and 4 far, 3 left ...
    s2 = tuple(a[:3] if i < 2 else a for i, a in enumerate(g["set"]))  # ... and here only 2
    ref = check(fe, [s, s2], 3.0, 7, draws_for(2, 7, 1), "few")
    assert (ref[0][1][0], ref[0][1][1]) == (0, 3) and (ref[1][1][0], ref[1][1][1]) == (2, 2)


def test_no_qualifying_hypothesis(fe):
    rng = np.random.default_rng(7)
    prev = rng.uniform([100, 80], [650, 400], (60, 2))
    ang = rng.uniform(0, 7, 60)
    curr = prev + rng.uniform(8, 30, (60, 1)) * np.stack([np.cos(ang), np.sin(ang)], 1)
    s = (prev, curr, np.eye(3), rr.EUROC_K, 0, rr.RADTAN)
    (mk, info, _, _), = check(fe, [s], 0.5, 7, draws_for(1, 7, 2), "status 3")
    assert info[0] == 3 and not mk.any()


def test_tie_goes_to_lowest_h(fe):
    s, draws = rr.tie_case()
    (mk, info, _, detail), = check(fe, [s], 0.5, 3, draws, "tie")
    assert detail["count"] == [4, 4, 4] and info[5] == 0
    # eleven hypotheses, the tied ones spread over different waves and rounds
    d11 = np.tile(np.array([[4, 0]], np.uint32), (11, 1))
    d11[[3, 9]] = [0, 0]
    (mk, info, _, detail), = check(fe, [s], 0.5, 11, d11[None], "tie over waves")
    assert detail["count"] == [4] * 11 and info[5] == 0
    np.testing.assert_array_equal(mk, np.arange(8) >= 4)


def test_same_call_twice_is_bit_identical(fe):
    sets, draws = multi_sets(), draws_for(5, 17, 4)
    a = fe.two_point_ransac(sets, 3.0, 17, draws)
    b = fe.two_point_ransac(sets, 3.0, 17, draws)
    for (ma, ia), (mb, ib) in zip(a, b):
        np.testing.assert_array_equal(ma, mb)
        ra = np.array([*ia[:7], *ia.m_refit, ia.refit_err], float)
        rb = np.array([*ib[:7], *ib.m_refit, ib.refit_err], float)
        assert ra.tobytes() == rb.tobytes()


def test_argument_errors_leave_the_context_usable(fe):
    import ctypes as C
    g = rr.synth_correspondences(20, seed=1)
    lib, dp, ip = fe.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    pp, pc = (np.ascontiguousarray(a) for a in g["set"][:2])
    R, K, k = np.eye(3).ravel(), g["intrinsics"].copy(), g["coeffs"].copy()
    draws = draws_for(1, 7, 0)
    inl, info = np.zeros(20, np.uint8), np.zeros(12)

    def call(h=None, n_sets=1, off=(0, 20), prev=pp, model=0, n_hyp=7, out=inl):
        off_a, model_a = np.array(off, np.int32), np.array([model], np.int32)
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        return lib.mfe_two_point_ransac(fe.h if h is None else h, n_sets, p(off_a, ip), p(prev, dp), p(pc, dp),
                                        p(R, dp), p(K, dp), p(model_a, ip), p(k, dp), 3.0, n_hyp,
                                        p(draws, C.POINTER(C.c_uint32)), p(out, C.POINTER(C.c_uint8)), p(info, dp))
    bad = {"null context": dict(h=C.c_void_p(None)), "n_sets < 0": dict(n_sets=-1),
           "null points": dict(prev=None), "null output": dict(out=None),
           "set_off not monotone": dict(n_sets=2, off=(0, 20, 10)), "set_off[0] != 0": dict(off=(1, 20)),
           "unknown model": dict(model=2), "n_hyp = 0": dict(n_hyp=0),
           "n_hyp above the cap": dict(n_hyp=_lib.RANSAC_MAX_HYP + 1),
           "set above the cap": dict(off=(0, _lib.RANSAC_MAX_SET_POINTS + 1))}
    for what, kw in bad.items():
        assert call(**kw) < 0, what
        assert lib.mfe_last_error(), what
    assert call(n_sets=0) == 0 and call(off=(0, 0)) == 0      # successful no-ops
    assert call() == 0 and info[0] == 0                          # and the context still works
    check(fe, [g["set"]], 3.0, 7, draws, "after errors")


# ------------------------------------------------------- ImageProcessor ----
W, H = 752, 480
StereoMsg = namedtuple("stereo_msg", ["vio_timestamp__", "cam0_msg", "cam1_msg"])
ImgMsg = namedtuple("img_msg", ["vio_timestamp__", "image"])
ImuMsg = namedtuple("imu_msg", ["vio_timestamp__", "angular_velocity", "linear_acceleration"])
SCENE = dict(frames=5, step=(3.0, -1.0), disp=12.0, rect=(150, 120, 600, 360), rect_step=(3.0, 2.0), move_from=3)
# room in the grid cells for all five frames' features (3 new per cell and frame), so that pruning
# drops nothing; and an inlier error well below the background's own flow (3.2 px): a flow shorter
# than the inlier error fits every model
SCENE_CFG = dict(grid_max_feature_num=16, ransac_threshold=1.0)


@pytest.fixture(scope="module")
def scene_frames():
    """Background plane moving by SCENE['step'] px per frame (as
    test_image_processor_synthetic_stereo); a rectangle of another texture is
    composited into both cameras, rides with the background up to frame
    move_from - 1 and then moves by rect_step per frame."""
    bg, fg = fs.texture_fn(4, W=W, H=H), fs.texture_fn(9, W=W, H=H)
    x0, y0, x1, y1 = SCENE["rect"]
    frames, rects = [], []
    off = np.zeros(2)
    for k in range(SCENE["frames"]):
        if k > 0:
            off = off + np.array(SCENE["rect_step"] if k >= SCENE["move_from"] else SCENE["step"])
        dx, dy = np.array(SCENE["step"]) * k
        pair = []
        for d in (0.0, SCENE["disp"]):
            img = fs.render(bg, W, H, dx - d, dy)
            ox, oy = off[0] - d, off[1]
            yy, xx = np.mgrid[0:H, 0:W].astype(float)
            inside = (xx - ox >= x0) & (xx - ox < x1) & (yy - oy >= y0) & (yy - oy < y1)
            img[inside] = fs.render(fg, W, H, ox, oy)[inside]
            pair.append(img)
        frames.append(pair)
        rects.append((x0 + off[0], y0 + off[1], x1 + off[0], y1 + off[1]))
    return frames, rects


def run_processor(frames, **kw):
    K = np.array([450.0, 450.0, 376.0, 240.0])
    Ti1 = np.eye(4)
    Ti1[0, 3] = -0.11
    ransac_fn = kw.pop("ransac_fn", None)
    cfg = fe_mod.FrontendConfig(T_imu_cam0=np.eye(4), T_imu_cam1=Ti1, cam0_distortion_coeffs=np.zeros(4),
                                cam1_distortion_coeffs=np.zeros(4), cam0_intrinsics=K, cam1_intrinsics=K, **kw)
    ip = fe_mod.ImageProcessor(cfg, ransac_fn=ransac_fn)
    out = []
    for k, (c0, c1) in enumerate(frames):
        t = 0.05 * k
        for j in range(10):
            ip.imu_callback(ImuMsg(t - 0.05 + 0.005 * j, np.zeros(3), np.array([0.0, 0.0, 9.81])))
        msg = ip.stareo_callback(StereoMsg(t, ImgMsg(t, c0), ImgMsg(t, c1)))
        out.append(({m.id: (m.u0 * K[0] + K[2], m.v0 * K[1] + K[3], m.u1, m.v1) for m in msg.vio_features},
                    ip.num_features["after_ransac"]))
    ip.fe.close()
    return [o[0] for o in out], [o[1] for o in out]


def test_image_processor_rejects_the_moving_rectangle(scene_frames):
    """Off, on (device) and on (numpy reference through ransac_fn) over the
    same frames.  The rectangle's step (3, 2) against the background's (3, -1)
    puts its matches 3 px off the background's epipolar lines, three times the
    1 px inlier error of SCENE_CFG.  The run with ransac_fn = the numpy
    reference, on the CPU oracle operators (test_frontend_ref.OracleFrontend),
    established these steps: there all 32 ids tracked inside the rectangle are
    gone in frame move_from and stay gone, 84 of the 85 background ids clear of
    the rectangle remain (as many as with RANSAC off), and with RANSAC off all
    32 survive to the last frame.  (At the default 3 px inlier error a 1.6 px
    background flow constrains nothing: a model through the rectangle's matches
    gathers the background too.)  The device run must publish the same ids and
    coordinates as the reference run in every frame."""
    frames, rects = scene_frames
    off, n_off = run_processor(frames, **SCENE_CFG)
    dev, n_dev = run_processor(frames, ransac_enabled=True, **SCENE_CFG)
    ref, n_ref = run_processor(frames, ransac_enabled=True, ransac_fn=rr.as_ransac_fn, **SCENE_CFG)
    assert n_dev == n_ref
    for k, (d, r) in enumerate(zip(dev, ref)):
        assert list(d) == list(r), "frame %d" % k
        for i in d:
            assert d[i] == r[i], (k, i)
    mv, last = SCENE["move_from"], SCENE["frames"] - 1

    def ids_in(run, k, margin):
        x0, y0, x1, y1 = rects[k]
        return {i for i, v in run[k].items() if
                x0 + margin <= v[0] < x1 - margin and y0 + margin <= v[1] < y1 - margin}

    def ids_far(run, k, margin):   # clear of everything the rectangle sweeps
        x0, y0, x1, y1 = SCENE["rect"]
        return {i for i, v in run[k].items() if
                not (x0 - margin <= v[0] < x1 + margin + 10 and y0 - margin <= v[1] < y1 + margin + 20)}
    born = ids_in(off, mv - 1, 20)            # tracked inside the rectangle just before it moves
    assert len(born) >= 5 and born == ids_in(ref, mv - 1, 20)
    assert born <= set(off[mv]) and born <= set(off[last])     # RANSAC off: they survive to the last frame
    assert n_ref[mv] < n_off[mv]
    for run in (ref, dev):
        assert not born & set(run[mv]) and not born & set(run[last])
        bgd = ids_far(run, mv - 1, 30)
        assert len(bgd) >= 30 and len(bgd & set(run[mv])) >= 0.9 * len(bgd)
