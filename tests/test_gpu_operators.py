"""The image operators of csrc/msckf_frontend.hip against oracle/frontend_oracle.py
at odd and tiny shapes (the case table of tests/frontend_operator_cases.py, which
tests/test_operator_cases_ref.py pins on the CPU): 8 x 8 up to 129 x 66, every
context with max_level 7.

  * k_pyrdown_sets: every level 0..7 of every image, read back by mfe_download,
    is fo.build_pyramid byte for byte -- through mfe_upload and through
    mfe_upload_many with three different images per call (blockIdx.z, the 16-byte
    and the single-byte scatter);
  * k_scharr_sets: both int16 planes of every level, read back by
    mfe_download_deriv, are fo.scharr of the oracle's level; the read-back's
    rejected arguments answer -1 and write nothing;
  * k_fast_sets / k_fast_rows_sets: xy and responses equal to fo.fast_detect for
    every FAST row (thresholds 0, 1, 15, 254, 255 and the clamped -5 and 300, with
    and without a mask), the total count, and the truncation to the first max_kp
    in raster order for max_kp in {0, 1, n - 1, n, n + 1} with nothing written
    past it;
  * lk_point through mfe_lk: window 3, 4, 8, 15, 16, max_level 0, 1, 3, 7,
    max_iter 1 and 30, eps 0 and 0.01 -- status identical on every point, no
    exclusions, positions of status-1 points within 1e-4 px (the bound of
    test_gpu_frontend.py); rejected arguments answer -1 and leave next_pts and
    status as passed in.

The kernels and the oracle do the same integer sums and float32 steps, so the
expected LK deviation is 0.  Largest deviation seen on an MI355X over all 22
rows: 0 px, and no status mismatch (each row prints its own figures).

FAST never answers within 3 px of the border, so 65 and 129 columns cannot put
a keypoint into the row kernel's last 64-column step; the FAST rows therefore
also run at 70 x 11 and 134 x 11, where the oracle has keypoints at x >= 64 and
x >= 128 (tests/test_operator_cases_ref.py asserts it)."""
import ctypes as C

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
import frontend_operator_cases as oc

pytestmark = pytest.mark.gpu

NSLOT = 4
MAX_POINTS = 64
_U8P, _F32P, _I16P = C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int16)


@pytest.fixture(scope="module")
def context():
    """shape -> the shape's one context, made on first use."""
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = fe_mod.Frontend(shape[0], shape[1], nslot=NSLOT, max_level=oc.MAX_LEVEL,
                                          max_points=MAX_POINTS)
        return made[shape]
    yield get
    for fe in made.values():
        fe.close()


def check_slot(fe, slot, shape, name, bad):
    """Every level and both derivative planes of a slot against the oracle's; mismatches go to bad."""
    pyr, der = oc.pyramid(shape, name)
    for level in range(oc.MAX_LEVEL + 1):
        got = fe.download(slot, level)
        ix, iy = fe.download_deriv(slot, level)
        assert got.shape == pyr[level].shape and got.dtype == np.uint8
        assert ix.shape == got.shape and iy.shape == got.shape and ix.dtype == np.int16 and iy.dtype == np.int16
        for what, a, b in (("image", got, pyr[level]), ("ix", ix, der[level][0]), ("iy", iy, der[level][1])):
            if not np.array_equal(a, b):
                bad.append((name, level, what, int((a != b).sum())))


@pytest.mark.parametrize("shape", oc.SHAPES, ids=oc.shape_id)
def test_pyramid_and_scharr_after_upload(context, shape):
    fe, bad = context(shape), []
    for k, name in enumerate(oc.SWEEP_IMAGES):
        slot = k % NSLOT
        fe.upload(slot, oc.images(shape)[name])
        check_slot(fe, slot, shape, name, bad)
    assert not bad, bad


@pytest.mark.parametrize("shape", oc.SHAPES, ids=oc.shape_id)
def test_pyramid_and_scharr_after_upload_many(context, shape):
    """Three different images per call, into slots out of order."""
    fe, bad = context(shape), []
    names = oc.SWEEP_IMAGES
    assert len(names) % 3 == 0
    for g in range(0, len(names), 3):
        group = names[g:g + 3]
        slots = [[2, 0, 3], [1, 3, 0]][(g // 3) % 2]
        fe.upload_many(slots, np.stack([oc.images(shape)[n] for n in group]))
        for slot, name in zip(slots, group):
            check_slot(fe, slot, shape, name, bad)
    assert not bad, bad


def test_download_deriv_rejects_bad_arguments(context):
    shape = (17, 33)
    fe = context(shape)
    fe.upload(0, oc.images(shape)["random"])
    ix = np.full((33, 17), 12345, np.int16)
    iy = np.full((33, 17), -12345, np.int16)
    px, py = ix.ctypes.data_as(_I16P), iy.ctypes.data_as(_I16P)
    call = fe.lib.mfe_download_deriv
    for args, text in (((0, oc.MAX_LEVEL + 1, px, py), b"level 8 outside [0, 7]"),
                       ((0, -1, px, py), b"level -1 outside [0, 7]"),
                       ((NSLOT, 0, px, py), b"slot[0] = 4 outside [0, 4)"),
                       ((-1, 0, px, py), b"slot[0] = -1 outside [0, 4)"),
                       ((0, 0, None, py), b"null argument"),
                       ((0, 0, px, None), b"null argument")):
        assert call(fe.h, *args) == -1, args[:2]
        assert fe.lib.mfe_last_error() == text
        assert (ix == 12345).all() and (iy == -12345).all()
    assert call(None, 0, 0, px, py) == -1 and (ix == 12345).all() and (iy == -12345).all()
    with pytest.raises(fe_mod._lib.MsckfError, match="level 8"):
        fe.download_deriv(0, 8)
    assert call(fe.h, 0, 0, px, py) == 0                     # and the same buffers are written by a good call
    np.testing.assert_array_equal(ix, oc.pyramid(shape, "random")[1][0][0])
    np.testing.assert_array_equal(iy, oc.pyramid(shape, "random")[1][0][1])


# ------------------------------------------------------------------- FAST --
def fast_raw(fe, slot, threshold, mask, max_kp):
    """mfe_fast into buffers two rows longer than max_kp, filled with a sentinel:
    (xy, response, total) with the whole buffers, so that the caller sees what was written where."""
    xy = np.full((max_kp + 2, 2), -7.0, np.float32)
    resp = np.full(max_kp + 2, -7.0, np.float32)
    n = C.c_int(-1)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    fe._check(fe.lib.mfe_fast(fe.h, slot, int(threshold), None if m is None else m.ctypes.data_as(_U8P), int(max_kp),
                              xy.ctypes.data_as(_F32P), resp.ctypes.data_as(_F32P), C.byref(n)))
    return xy, resp, n.value


@pytest.mark.parametrize("shape", oc.FAST_SHAPES, ids=oc.shape_id)
def test_fast_matches_oracle(context, shape):
    fe = context(shape)
    rows = [r for r in oc.FAST_ROWS if r.shape == shape]
    assert len(rows) == 2 * 7 * 2
    uploaded, found = None, 0
    for r in rows:
        if r.image != uploaded:
            fe.upload(1, oc.images(shape)[r.image])
            uploaded = r.image
        xo, ro = oc.fast_oracle(r)
        n = len(xo)
        found += n
        mask = oc.fast_mask(shape) if r.masked else None
        xy, resp = fe.fast(1, r.threshold, mask=mask)
        np.testing.assert_array_equal(xy, xo, err_msg=str(r))
        np.testing.assert_array_equal(resp, ro.astype(np.float32), err_msg=str(r))
        for max_kp in oc.max_kp_values(n):
            xy, resp, total = fast_raw(fe, 1, r.threshold, mask, max_kp)
            k = min(n, max_kp)
            assert total == n, (r, max_kp, total, n)
            np.testing.assert_array_equal(xy[:k], xo[:k], err_msg="%s max_kp %d" % (r, max_kp))
            np.testing.assert_array_equal(resp[:k], ro[:k].astype(np.float32), err_msg="%s max_kp %d" % (r, max_kp))
            assert (xy[k:] == -7.0).all() and (resp[k:] == -7.0).all(), (r, max_kp)
    print("%s: %d FAST rows, %d oracle keypoints in all" % (oc.shape_id(shape), len(rows), found))


# --------------------------------------------------------------------- LK --
@pytest.mark.parametrize("row", oc.LK_ROWS, ids=oc.lk_id)
def test_lk_matches_oracle(context, row):
    fe = context(row.shape)
    prev_img, next_img = oc.lk_images(row)
    fe.upload_many([3, 2], np.stack([prev_img, next_img]))
    prev, guess = oc.lk_points(row)
    o, so = oc.lk_oracle(row)
    g, sg = fe.lk(3, 2, prev, guess, win=row.win, max_level=row.max_level, max_iter=row.max_iter, eps=row.eps)
    ok = so == 1
    dev = float(np.abs(g[ok].astype(np.float64) - o[ok]).max()) if ok.any() else 0.0
    print("%s: %d points, %d tracked by the oracle, worst deviation %.3e px, %d status mismatches"
          % (oc.lk_id(row), len(prev), int(ok.sum()), dev, int((sg != so).sum())))
    np.testing.assert_array_equal(sg, so, err_msg="status differs at points %s" % np.nonzero(sg != so)[0])
    assert dev <= 1e-4, dev


def test_lk_rejects_bad_arguments(context):
    shape = (33, 17)
    fe = context(shape)
    im = oc.images(shape)
    fe.upload_many([0, 1], np.stack([im["texture"], im["moved"]]))
    prev = np.ascontiguousarray([[10.0, 8.0], [20.5, 5.0], [3.0, 3.0]], np.float32)
    for win, max_level, max_iter, text in ((2, 3, 30, b"window 2 outside [3, 16]"),
                                           (17, 3, 30, b"window 17 outside [3, 16]"),
                                           (15, 8, 30, b"max_level 8 outside [0, 7]"),
                                           (15, 3, 0, b"max_iter must be positive")):
        nxt = np.ascontiguousarray(prev + np.float32([1.0, -0.5]))
        kept = nxt.copy()
        st = np.full(len(prev), 9, np.uint8)
        rc = fe.lib.mfe_lk(fe.h, 0, 1, len(prev), prev.ctypes.data_as(_F32P), nxt.ctypes.data_as(_F32P),
                           st.ctypes.data_as(_U8P), win, max_level, max_iter, 0.01)
        assert rc == -1 and fe.lib.mfe_last_error() == text, (win, max_level, max_iter, rc)
        np.testing.assert_array_equal(nxt, kept)
        assert (st == 9).all()
    g, s = fe.lk(0, 1, prev, prev + np.float32([1.0, -0.5]), win=16, max_level=7, max_iter=1, eps=0.0)   # the limits pass
    assert g.shape == (3, 2) and s.shape == (3,)
