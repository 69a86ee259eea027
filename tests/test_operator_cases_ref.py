"""The case table of the operator sweep (tests/frontend_operator_cases.py) and
the oracle it is compared with (oracle/frontend_oracle.py), on the CPU: every
assertion here is a condition the oracle alone must meet, so that what
tests/test_gpu_operators.py compares the kernels with is itself pinned and the
table reaches the branches it is meant to reach.

  * reflect101, pyr_down and scharr against brute-force restatements: plain
    loops, the border index looked up in a written-out reflected list (a walk
    that turns at both ends, itself pinned to literal tables), the 5 x 5 and
    3 x 3 kernels as 2-D tables -- on every image of every shape and on 1 x N,
    2 x N and 3 x N strips either way;
  * the table's reach: status 1 and status 0 points for every LK window size, a
    level-0 window rejected by min_eig, FAST keypoints in the second and third
    64-column step, empty threshold-255 rows, a keypoint lost to the mask.

FAST leaves a 3 px border, so W = 65 and W = 129 can hold no keypoint at
x >= 64 and x >= 128 (asserted below as what it is); the conditions on those
columns are asked of the FAST-only shapes 70 x 11 and 134 x 11."""
import numpy as np
import pytest

from oracle import frontend_oracle as fo
import frontend_operator_cases as oc


# ------------------------------------------------ brute-force restatements --
def reflected_list(n, border):
    """BORDER_REFLECT_101 written out: the source index of every position
    -border .. n - 1 + border, by walking away from the image and turning at
    index 0 and index n - 1 (gfedcb|abcdefgh|gfedcba)."""
    def walk(start, step, count):
        out, i = [], start
        for _ in range(count):
            if n == 1:
                step = 0
            elif i + step < 0 or i + step > n - 1:
                step = -step
            i += step
            out.append(i)
        return out
    return walk(0, -1, border)[::-1] + list(range(n)) + walk(n - 1, 1, border)


def test_reflected_list_is_the_literal_border():
    assert reflected_list(1, 3) == [0, 0, 0, 0, 0, 0, 0]
    assert reflected_list(2, 3) == [1, 0, 1, 0, 1, 0, 1, 0]
    assert reflected_list(3, 3) == [1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert reflected_list(5, 2) == [2, 1, 0, 1, 2, 3, 4, 3, 2]
    assert reflected_list(8, 2) == [2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 17, 33, 65, 66, 129])
def test_reflect101_matches_the_written_out_list(n):
    border = 20
    ref = reflected_list(n, border)
    np.testing.assert_array_equal(fo.reflect101(np.arange(-border, n + border), n), ref)
    for i in (-border, -1, 0, n - 1, n, n + border - 1):      # scalars too
        assert int(fo.reflect101(i, n)) == ref[i + border]


GAUSS = [[a * b for b in (1, 4, 6, 4, 1)] for a in (1, 4, 6, 4, 1)]           # sums to 256
SCHARR_X = [[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]]
SCHARR_Y = [[-3, -10, -3], [0, 0, 0], [3, 10, 3]]


def pyr_down_brute(img):
    src = [[int(v) for v in row] for row in img]
    H, W = len(src), len(src[0])
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    ry, rx = reflected_list(H, 2), reflected_list(W, 2)
    out = np.zeros((h2, w2), np.uint8)
    for y in range(h2):
        for x in range(w2):
            s = 0
            for i in range(5):
                row = src[ry[2 * y + i]]                       # position 2 y - 2 + i, list offset 2
                for j in range(5):
                    s += GAUSS[i][j] * row[rx[2 * x + j]]
            out[y, x] = (s + 128) // 256
    return out


def scharr_brute(img):
    src = [[int(v) for v in row] for row in img]
    H, W = len(src), len(src[0])
    ry, rx = reflected_list(H, 1), reflected_list(W, 1)
    ix, iy = np.zeros((H, W), np.int16), np.zeros((H, W), np.int16)
    for y in range(H):
        for x in range(W):
            gx = gy = 0
            for i in range(3):
                row = src[ry[y + i]]                           # position y - 1 + i, list offset 1
                for j in range(3):
                    v = row[rx[x + j]]
                    gx += SCHARR_X[i][j] * v
                    gy += SCHARR_Y[i][j] * v
            assert -32768 <= gx <= 32767 and -32768 <= gy <= 32767
            ix[y, x], iy[y, x] = gx, gy
    return ix, iy


def check_operators(img):
    """pyr_down and scharr of one image, and of every level below it down to 1 x 1."""
    while True:
        ix, iy = fo.scharr(img)
        bx, by = scharr_brute(img)
        assert ix.dtype == np.int16 and iy.dtype == np.int16
        np.testing.assert_array_equal(ix, bx)
        np.testing.assert_array_equal(iy, by)
        if img.shape == (1, 1):
            return
        down = fo.pyr_down(img)
        assert down.dtype == np.uint8 and down.shape == ((img.shape[0] + 1) // 2, (img.shape[1] + 1) // 2)
        np.testing.assert_array_equal(down, pyr_down_brute(img))
        img = down


@pytest.mark.parametrize("shape", oc.SHAPES, ids=oc.shape_id)
def test_pyr_down_and_scharr_match_brute_force(shape):
    W, H = shape
    for name in oc.SWEEP_IMAGES:
        img = oc.images(shape)[name]
        assert img.shape == (H, W) and img.dtype == np.uint8
        check_operators(img)
        pyr, der = oc.pyramid(shape, name)                      # what the GPU test compares with
        assert len(pyr) == oc.MAX_LEVEL + 1 and pyr[-1].shape == ((1, 2) if W == 129 else (1, 1))
        np.testing.assert_array_equal(pyr[1], pyr_down_brute(img))
        np.testing.assert_array_equal(der[0][0], scharr_brute(img)[0])


def test_pyr_down_and_scharr_on_strips():
    rng = np.random.default_rng(7)
    for k in (1, 2, 3):
        for n in range(1, 10):
            for shape in ((k, n), (n, k)):
                check_operators(rng.integers(0, 256, shape).astype(np.uint8))
                check_operators(np.full(shape, 255, np.uint8))


def test_scharr_extremes_survive_int16():
    """The 0 / 255 steps reach +-4080 = 16 x 255, the largest Scharr response of 8-bit data."""
    for shape in oc.SHAPES:
        ix, _ = oc.pyramid(shape, "vstep")[1][0]
        _, iy = oc.pyramid(shape, "hstep")[1][0]
        assert ix.max() == 4080 and iy.max() == 4080 and ix.min() == 0 and iy.min() == 0
        ix, iy = fo.scharr(255 - oc.images(shape)["vstep"])
        assert ix.min() == -4080
        assert not oc.pyramid(shape, "checker")[1][0][0].any()   # x - 1 and x + 1 are the same colour
        assert (oc.pyramid(shape, "checker")[0][1] == 128).all()  # 255 * 128 + 128 >> 8: the rounding term decides


# ------------------------------------------------------- the table's reach --
def test_lk_rows_cover_the_contract():
    rows = oc.LK_ROWS
    assert 18 <= len(rows) <= 24
    assert {r.win for r in rows} == {3, 4, 8, 15, 16}
    assert {r.max_level for r in rows} == {0, 1, 3, 7}
    assert {r.max_iter for r in rows} == {1, 30}
    assert {r.eps for r in rows} == {0.0, 0.01}
    assert {r.shape for r in rows} == set(oc.SHAPES)
    for r in rows:
        (W, H), m = r.shape, r.win + 2
        prev, guess = oc.lk_points(r)
        assert prev.dtype == np.float32 and prev.shape == guess.shape and len(prev) >= 45
        assert (prev[:40] >= -m).all() and (prev[:40, 0] <= W + m).all() and (prev[:40, 1] <= H + m).all()
        outside = (prev[:, 0] < 0) | (prev[:, 0] > W - 1) | (prev[:, 1] < 0) | (prev[:, 1] > H - 1)
        assert outside.any() and not outside.all()
        for c in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):
            assert (prev == np.float32(c)).all(1).any()
        frac = prev - np.floor(prev)
        assert (frac == 0).all(1).any() and (frac == 0.5).all(1).any()
        assert (np.abs(guess - prev)[:, 0] >= 3 * W).sum() == 1


def test_lk_rows_give_both_statuses_for_every_window():
    for win in (3, 4, 8, 15, 16):
        st = np.concatenate([oc.lk_oracle(r)[1] for r in oc.LK_ROWS if r.win == win and r.scene == "texture"])
        assert (st == 1).sum() >= 5 and (st == 0).sum() >= 5, (win, int((st == 1).sum()), int((st == 0).sum()))


def test_lk_rows_reach_the_min_eig_skip():
    """A point whose level-0 window is inside the oracle's bounds and is rejected by min_eig:
    every such point of the constant row, and the oracle answers status 0 for it."""
    hit = 0
    for r in oc.LK_ROWS:
        if r.scene != "constant":
            continue
        prev_img, _ = oc.lk_images(r)
        prev, _ = oc.lk_points(r)
        _, st = oc.lk_oracle(r)
        for p, s in zip(prev, st):
            inb, min_eig, _ = oc.lk_level0_window(prev_img, p, r.win)
            if inb:
                assert min_eig < fo.MIN_EIG_THRESHOLD and s == 0
                hit += 1
    assert hit >= 5
    # and on the texture, where it is the exception: some windows pass the test, some do not
    passed = failed = 0
    for r in oc.LK_ROWS:
        if r.scene == "texture":
            prev_img, _ = oc.lk_images(r)
            for p in oc.lk_points(r)[0]:
                inb, min_eig, D = oc.lk_level0_window(prev_img, p, r.win)
                if inb:
                    ok = min_eig >= fo.MIN_EIG_THRESHOLD and D >= np.finfo(np.float32).eps
                    passed, failed = passed + ok, failed + (not ok)
    assert passed >= 5 and failed >= 1, (passed, failed)


def test_fast_rows_cover_the_contract():
    rows = oc.FAST_ROWS
    assert {r.threshold for r in rows} == {0, 1, 15, 254, 255, -5, 300}
    assert oc.clamped(-5) == 0 and oc.clamped(300) == 255 and oc.clamped(15) == 15
    assert {r.shape for r in rows} == set(oc.SHAPES) | set(oc.FAST_EXTRA_SHAPES)
    for shape in oc.FAST_SHAPES:
        share = 1.0 - oc.fast_mask(shape).mean()
        assert 0.35 <= share <= 0.65, (shape, share)
    assert oc.max_kp_values(0) == [0, 1] and oc.max_kp_values(1) == [0, 1, 2] and oc.max_kp_values(7) == [0, 1, 6, 7, 8]


def test_fast_rows_reach_every_column_step():
    """One wave walks a row in 64-column steps.  At W = 65 / 129 the last step holds only border
    columns; at 70 / 134 it holds a keypoint."""
    def max_x(W):
        return max((float(oc.fast_oracle(r)[0][:, 0].max()) for r in oc.FAST_ROWS
                    if r.shape[0] == W and len(oc.fast_oracle(r)[0])), default=-1.0)
    assert 0 <= max_x(65) <= 61 and 64 <= max_x(129) <= 125
    assert max_x(70) >= 64
    assert max_x(134) >= 128
    for shape in oc.FAST_SHAPES:                                # and every shape that can has keypoints at all
        if min(shape) > 8:
            assert any(len(oc.fast_oracle(r)[0]) for r in oc.FAST_ROWS if r.shape == shape), shape


def test_fast_rows_thresholds_and_masks():
    lost = 0
    for r in oc.FAST_ROWS:
        xy, resp = oc.fast_oracle(r)
        assert xy.dtype == np.float32 and resp.dtype == np.int32 and len(xy) == len(resp)
        if oc.clamped(r.threshold) == 255:
            assert len(xy) == 0, r
        if r.masked:
            full = oc.fast_oracle(r._replace(masked=False))[0]
            assert len(xy) <= len(full)
            lost += len(xy) < len(full)
            assert (oc.fast_mask(r.shape)[xy[:, 1].astype(int), xy[:, 0].astype(int)] != 0).all()
    assert lost >= 1
    for a, b in ((-5, 0), (300, 255)):                           # the clamped rows are the in-range rows
        for r in oc.FAST_ROWS:
            if r.threshold == a:
                np.testing.assert_array_equal(oc.fast_oracle(r)[0], oc.fast_oracle(r._replace(threshold=b))[0])
