"""Plain numpy restatement of include/msckf_equalize.h (the header's algorithm
text is the specification): histogram equalisation and CLAHE of an 8-bit
single-channel image, the reference of tests/test_equalize_ref.py and
tests/test_gpu_equalize.py.

cv2 is absent here, as it is for every other operator, so this restates the
published OpenCV 4.x algorithms (imgproc/histogram.cpp equalizeHist,
imgproc/clahe.cpp); parity against cv2 itself is unpinned.  Conventions of both
functions: all float arithmetic is float32, in the order written, one rounding
per operation; ``sat`` rounds half to even and clips to 0..255.

``EqualizingFrontend`` is tests/frontend_lanes_ref.py's CPU stand-in of
msckf_amd.frontend.Frontend with the equalisation argument of ``upload`` /
``upload_many`` served by these functions, so that the processors run with
FrontendConfig.equalize and without a device; ``upload_log`` records, per
``upload_many`` call, how many arguments it was given beyond (slots, images).
"""
import numpy as np

import frontend_lanes_ref as lr

F = np.float32
MODES = {0: "none", 1: "hist", 2: "clahe"}


def sat(x):
    """saturate_cast<uchar> of float32 values."""
    return np.clip(np.rint(np.asarray(x, F)), 0, 255).astype(np.uint8)


def equalize_hist(img):
    """cv2.equalizeHist."""
    img = np.asarray(img, np.uint8)
    h = np.bincount(img.ravel(), minlength=256).astype(np.int64)
    i = int(np.nonzero(h)[0][0])
    if h[i] == img.size:
        return img.copy()
    scale = F(255.0) / F(img.size - h[i])
    lut = np.zeros(256, np.uint8)
    s = np.cumsum(h[i + 1:])
    lut[i + 1:] = sat(s.astype(F) * scale)
    return lut[img]


def pad101(img, tiles):
    """The image clahe takes its histograms from: padded right and bottom
    (BORDER_REFLECT_101) unless both sides are multiples of the tile counts."""
    H, W = img.shape
    tx, ty = tiles
    if W % tx == 0 and H % ty == 0:
        return img
    return np.pad(img, ((0, ty - H % ty), (0, tx - W % tx)), mode="reflect")


def clip_of(clip_limit, area):
    """The bin limit of a tile of ``area`` pixels (0: none).  The device call
    carries clip_limit as float32."""
    cl = float(F(clip_limit))
    if not cl > 0:
        return 0
    return max(int(min(cl * area / 256, area)), 1)   # no bin holds more than area


def tile_luts(img, clip_limit, tiles):
    """(lut uint8 [ty][tx][256], tw, th) of clahe's steps 1-5."""
    tx, ty = tiles
    ext = pad101(np.asarray(img, np.uint8), tiles)
    tw, th = ext.shape[1] // tx, ext.shape[0] // ty
    area = tw * th
    lut_scale = F(255.0) / F(area)
    clip = clip_of(clip_limit, area)
    luts = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            h = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                excess = int(np.maximum(h - clip, 0).sum())
                h = np.minimum(h, clip)
                h += excess // 256
                residual = excess % 256
                if residual:
                    step = max(256 // residual, 1)
                    k = 0
                    while k < 256 and residual > 0:
                        h[k] += 1
                        k += step
                        residual -= 1
            luts[j, i] = sat(np.cumsum(h).astype(F) * lut_scale)
    return luts, tw, th


def clahe(img, clip_limit=40.0, tiles=(8, 8)):
    """cv2.createCLAHE(clip_limit, tiles).apply; tiles = (tiles_x, tiles_y)."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    tx, ty = tiles
    luts, tw, th = tile_luts(img, clip_limit, tiles)
    L = luts.astype(F)

    def axis(n, t, cnt):
        f = np.arange(n).astype(F) * (F(1.0) / F(t)) - F(0.5)
        i1 = np.floor(f)
        a = (f - i1).astype(F)
        i1 = i1.astype(int)
        return np.maximum(i1, 0), np.minimum(i1 + 1, cnt - 1), a, (F(1.0) - a).astype(F)
    x1, x2, xa, xa1 = axis(W, tw, tx)
    y1, y2, ya, ya1 = axis(H, th, ty)
    X1, X2, XA, XA1 = x1[None, :], x2[None, :], xa[None, :], xa1[None, :]
    Y1, Y2, YA, YA1 = y1[:, None], y2[:, None], ya[:, None], ya1[:, None]
    top = L[Y1, X1, img] * XA1 + L[Y1, X2, img] * XA
    bot = L[Y2, X1, img] * XA1 + L[Y2, X2, img] * XA
    res = top * YA1 + bot * YA
    assert res.dtype == F
    return sat(res)


def equalize(img, mode, clip_limit=40.0, tiles=(8, 8)):
    """An image as the device leaves it in level 0; mode by name or MFE_EQ_* number."""
    mode = MODES.get(mode, mode)
    if mode == "none":
        return np.asarray(img, np.uint8).copy()
    if mode == "hist":
        return equalize_hist(img)
    if mode == "clahe":
        return clahe(img, clip_limit, tuple(tiles))
    raise ValueError("unknown equalisation mode %r" % (mode,))


_equalize = equalize


class EqualizingFrontend(lr.LanesOracleFrontend):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.upload_log = []

    def upload(self, slot, image, equalize=None):
        super().upload(slot, image if equalize is None else _equalize(image, *equalize))

    def upload_many(self, slots, images, *eq):
        self.upload_log.append(len(eq))
        self.calls.append("upload_many")
        if len(set(int(s) for s in slots)) != len(slots):
            raise lr.pr.fe_mod._lib.MsckfError("mfe: a slot is named twice (rc=-1)")
        for k, (s, im) in enumerate(zip(slots, images)):
            self.upload(int(s), im, None if not eq else (eq[0][0][k], eq[0][1][k], eq[0][2]))
