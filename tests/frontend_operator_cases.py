"""The case table of the image-operator sweep: shapes, images, FAST rows and LK
rows shared by tests/test_operator_cases_ref.py (CPU: the table and the oracle
against brute-force restatements) and tests/test_gpu_operators.py (the HIP
kernels against the oracle).  Everything is drawn from default_rng(fixed seed);
the oracle's answers are computed once per process and shared (lru_cache), and
callers must not write into them.

Shapes (W, H): the context's minimum 8 x 8 and one past it, exactly one 16 x 16
tile, a tile plus one either way, one column past a 64-lane wave and one past
two.  Every context is made with max_level 7, so the deepest levels are 1 x 1
(2 x 1 at level 7 of 129 x 66).

FAST never answers within 3 px of the border, so at W = 65 and W = 129 the
second and third 64-column step of the row kernel can hold no keypoint at all
(x <= W - 4 = 61 and 125).  Two further FAST-only shapes, 70 x 11 and 134 x 11,
are the smallest neighbours at which a keypoint can sit at x >= 64 and x >= 128;
the table asks for one there.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import frontend_oracle as fo
import frontend_synth as fs

MAX_LEVEL = 7
SHAPES = [(8, 8), (9, 8), (16, 16), (17, 33), (33, 17), (65, 49), (129, 66)]
FAST_EXTRA_SHAPES = [(70, 11), (134, 11)]
FAST_SHAPES = SHAPES + FAST_EXTRA_SHAPES
MOTION = (1.3, -0.7)


def shape_id(shape):
    return "%dx%d" % shape


def _seed(W, H, salt=0):
    return 100000 * salt + 1000 * W + H


IMPULSES = {"impulse_tl": (0.0, 0.0), "impulse_t": (0.5, 0.0), "impulse_tr": (1.0, 0.0), "impulse_l": (0.0, 0.5),
            "impulse_r": (1.0, 0.5), "impulse_bl": (0.0, 1.0), "impulse_b": (0.5, 1.0), "impulse_br": (1.0, 1.0)}


@lru_cache(maxsize=None)
def images(shape):
    """The images of a shape, name -> uint8 (H, W), read-only."""
    W, H = shape
    rng = np.random.default_rng(_seed(W, H))
    yy, xx = np.mgrid[0:H, 0:W]
    f = fs.texture_fn(_seed(W, H, 1), W=W, H=H)
    out = {"random": rng.integers(0, 256, (H, W)).astype(np.uint8),
           "texture": fs.render(f, W, H),
           "moved": fs.render(f, W, H, *MOTION),            # LK's next image; not part of the image sweep
           "zeros": np.zeros((H, W), np.uint8),
           "full": np.full((H, W), 255, np.uint8),
           "vstep": np.where(xx >= W // 2, 255, 0).astype(np.uint8),
           "hstep": np.where(yy >= H // 2, 255, 0).astype(np.uint8),
           "checker": (((xx + yy) & 1) * 255).astype(np.uint8)}
    for name, (ax, ay) in IMPULSES.items():
        img = np.zeros((H, W), np.uint8)
        img[int(ay * (H - 1)), int(ax * (W - 1))] = 255
        out[name] = img
    for img in out.values():
        img.setflags(write=False)
    return out


SWEEP_IMAGES = ["random", "texture", "zeros", "full", "vstep", "hstep", "checker"] + list(IMPULSES)


@lru_cache(maxsize=None)
def pyramid(shape, name):
    """fo.build_pyramid to level 7 and fo.scharr of every level: ([img_l], [(ix_l, iy_l)])."""
    pyr = fo.build_pyramid(images(shape)[name], MAX_LEVEL)
    return pyr, [fo.scharr(p) for p in pyr]


# ------------------------------------------------------------------- FAST --
FAST_THRESHOLDS = [0, 1, 15, 254, 255, -5, 300]
FAST_IMAGES = ["random", "texture"]
FastRow = namedtuple("FastRow", ["shape", "image", "threshold", "masked"])
FAST_ROWS = [FastRow(s, i, t, m) for s in FAST_SHAPES for i in FAST_IMAGES for t in FAST_THRESHOLDS
             for m in (False, True)]


def clamped(threshold):
    """What mfe_fast makes of an out-of-range threshold."""
    return min(max(int(threshold), 0), 255)


@lru_cache(maxsize=None)
def fast_mask(shape):
    """Roughly 50 % zeros."""
    W, H = shape
    m = (np.random.default_rng(_seed(W, H, 2)).random((H, W)) >= 0.5).astype(np.uint8)
    m.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def fast_oracle(row):
    """fo.fast_detect of a FAST row at the clamped threshold: (xy float32 (n, 2), response int32 (n,))."""
    return fo.fast_detect(images(row.shape)[row.image], clamped(row.threshold),
                          mask=fast_mask(row.shape) if row.masked else None)


def max_kp_values(n):
    """The truncations of a row with n oracle keypoints: 0, 1, n - 1, n, n + 1."""
    return sorted({k for k in (0, 1, n - 1, n, n + 1) if k >= 0})


# --------------------------------------------------------------------- LK --
# scene "texture": the texture and its render moved by MOTION; "constant": a black previous
# image, whose every window the oracle rejects by min_eig (the early skip of a level)
LKRow = namedtuple("LKRow", ["shape", "win", "max_level", "max_iter", "eps", "scene"])
LK_ROWS = [
    LKRow((8, 8), 3, 7, 30, 0.01, "texture"),
    LKRow((8, 8), 16, 0, 30, 0.0, "texture"),
    LKRow((9, 8), 4, 7, 30, 0.01, "texture"),
    LKRow((9, 8), 15, 1, 1, 0.01, "texture"),
    LKRow((16, 16), 8, 3, 30, 0.01, "texture"),
    LKRow((16, 16), 16, 7, 30, 0.0, "texture"),
    LKRow((16, 16), 3, 0, 1, 0.0, "texture"),
    LKRow((17, 33), 15, 3, 30, 0.01, "texture"),
    LKRow((17, 33), 4, 1, 30, 0.0, "texture"),
    LKRow((17, 33), 15, 3, 30, 0.01, "constant"),
    LKRow((33, 17), 8, 7, 30, 0.01, "texture"),
    LKRow((33, 17), 16, 3, 1, 0.01, "texture"),
    LKRow((33, 17), 3, 1, 30, 0.01, "texture"),
    LKRow((65, 49), 15, 7, 30, 0.01, "texture"),
    LKRow((65, 49), 4, 3, 30, 0.0, "texture"),
    LKRow((65, 49), 16, 1, 30, 0.01, "texture"),
    LKRow((65, 49), 8, 0, 1, 0.0, "texture"),
    LKRow((129, 66), 15, 3, 30, 0.01, "texture"),
    LKRow((129, 66), 16, 7, 30, 0.0, "texture"),
    LKRow((129, 66), 3, 3, 30, 0.01, "texture"),
    LKRow((129, 66), 8, 1, 30, 0.01, "texture"),
    LKRow((129, 66), 4, 0, 30, 0.01, "texture"),
]


def lk_id(row):
    return "%s_w%d_l%d_i%d_e%g_%s" % (shape_id(row.shape), row.win, row.max_level, row.max_iter, row.eps, row.scene)


def lk_images(row):
    im = images(row.shape)
    return (im["zeros"] if row.scene == "constant" else im["texture"]), im["moved"]


@lru_cache(maxsize=None)
def lk_points(row):
    """(prev_pts, guess) float32 (n, 2): 40 points uniform over the image widened by win + 2 on
    every side (some start outside), the four corners, points at exact integer and exact
    half-integer coordinates, and one whose guess is about 3 W away."""
    (W, H), m = row.shape, row.win + 2
    rng = np.random.default_rng(_seed(W, H, 3 + LK_ROWS.index(row)))
    pts = rng.uniform([-m, -m], [W + m, H + m], (40, 2))
    guess = pts + rng.uniform(-1.5, 1.5, (40, 2))
    cx, cy = W // 2, H // 2
    fixed = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1],
                      [cx, cy], [cx - 2, cy + 1], [cx + 0.5, cy + 0.5], [cx - 1.5, cy], [cx, cy - 0.5]], float)
    far = np.array([[cx, cy]], float)
    prev = np.concatenate([pts, fixed, far]).astype(np.float32)
    nxt = np.concatenate([guess, fixed + [1.0, -0.5], far + [3.0 * W, 0.0]]).astype(np.float32)
    prev.setflags(write=False)
    nxt.setflags(write=False)
    return prev, nxt


@lru_cache(maxsize=None)
def lk_oracle(row):
    """fo.lk_track of an LK row: (next_pts float32 (n, 2), status uint8 (n,))."""
    prev_img, next_img = lk_images(row)
    prev, guess = lk_points(row)
    return fo.lk_track(prev_img, next_img, prev, guess, win=row.win, max_level=row.max_level,
                       max_iter=row.max_iter, eps=row.eps)


def lk_level0_window(img, pt, win):
    """The oracle's own test of a point's level-0 window, from its intermediate values:
    (in_bounds, min_eig, D) as fo.lk_track computes them (min_eig and D are None out of bounds)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ix, iy = fo.scharr(img)
    p = np.asarray(pt, np.float32) - np.float32((win - 1) * 0.5)
    ipx, ipy = int(np.floor(p[0])), int(np.floor(p[1]))
    if ipx < -win or ipx >= W or ipy < -win or ipy >= H:
        return False, None, None
    w = fo._weights(p[0] - np.float32(ipx), p[1] - np.float32(ipy))
    ixv = fo._descale(fo._patch(ix, ipx, ipy, win, w, zero_border=True), fo.W_BITS)
    iyv = fo._descale(fo._patch(iy, ipx, ipy, win, w, zero_border=True), fo.W_BITS)
    A11 = np.float32(np.sum(ixv * ixv)) * np.float32(fo.FLT_SCALE)
    A12 = np.float32(np.sum(ixv * iyv)) * np.float32(fo.FLT_SCALE)
    A22 = np.float32(np.sum(iyv * iyv)) * np.float32(fo.FLT_SCALE)
    D = A11 * A22 - A12 * A12
    min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (2 * win * win)
    return True, float(min_eig), float(D)
