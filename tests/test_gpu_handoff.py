"""The device-side hand-off of include/msckf_handoff.h at the C-ABI level:
mfe_tracks_msg_put / _get, mfe_tracks_step_msg and msckf_map_add_lost_tracks.

No tolerance is involved anywhere in this file: the message calls move bytes,
mfe_tracks_step_msg runs the body of mfe_tracks_step (pinned bit for bit by
tests/test_gpu_tracks.py) and msckf_map_add_lost_tracks runs the kernel of
msckf_map_add_lost (pinned by tests/test_gpu_feature_map.py), so every
comparison is with the existing call on a second context, bit for bit.

The front-end contexts are tests/test_gpu_tracks.py's small_context (150 x 110
images, three lanes: 40 rows with RANSAC, 12 rows, an empty table); the filter
contexts tests/test_gpu_feature_map.py's make_ctx with tables of
feature_map_cases.random_table and messages cut from feature_map_cases.messages
/ big_messages."""
import re

import numpy as np
import pytest

import msckf_amd.frontend as fe_mod
from msckf_amd import MsckfError, _lib, synth
import feature_map_ref as fr
import feature_map_cases as fc
import test_gpu_feature_map as tm
import test_gpu_tracks as tt

pytestmark = pytest.mark.gpu
STEP = dict(inlier_error=tt.INLIER_ERROR, n_hyp=tt.N_HYP, **tt.LK)
SIZES = [0, 1, 63, 64, 65, 256, 257, 513]   # a wavefront, one 256-row pass of k_map_add_lost, two passes
FE_CAP = 640                                # rows of a lane's message table in the map tests (no multiple of 256)


def rc_of(err):
    return int(re.search(r"rc=(-?\d+)", str(err.value)).group(1))


def same_message(got, ids, uv):
    valid, gi, gu = got
    assert valid
    np.testing.assert_array_equal(gi, np.asarray(ids, np.int64))
    assert gu.shape == (len(gi), 4) and gu.tobytes() == np.ascontiguousarray(uv, np.float64).tobytes()


def message_tables(n_lanes=3, cap=FE_CAP):
    """A front-end context with message tables only: no image is needed to put a message."""
    fe = fe_mod.Frontend(tt.W, tt.H, nslot=3 * n_lanes, max_level=1, max_points=64)
    fe.tracks_create(n_lanes, cap, 4, 5, 3, 5)
    return fe


# ------------------------------------------------------------ the messages --
def test_msg_put_get_round_trip_and_errors():
    fe, tables, args = tt.small_context()
    rng = np.random.default_rng(1)
    try:
        cap = fe.tracks_cap
        valid, ids0, uv0 = fe.tracks_msg_get(0)          # a lane starts without a message
        assert not valid and len(ids0) == 0 and uv0.shape == (0, 4)
        msgs = {}
        for lane, n in ((0, 100), (1, cap), (2, 0)):
            msgs[lane] = (fc.weird_ids(rng, n), rng.standard_normal((n, 4)))
            fe.tracks_msg_put(lane, *msgs[lane])
        for lane, (ids, uv) in msgs.items():
            same_message(fe.tracks_msg_get(lane), ids, uv)
        ids, uv = msgs[0]
        rep = ids.copy()
        rep[57] = rep[3]
        for bad in (lambda: fe.tracks_msg_put(0, rep, uv),                                           # a repeated id
                    lambda: fe.tracks_msg_put(0, np.arange(cap + 1), np.zeros((cap + 1, 4))),         # n > cap
                    lambda: fe.tracks_msg_put(3, ids, uv), lambda: fe.tracks_msg_put(-1, ids, uv),    # lane
                    lambda: fe.tracks_msg_get(3)):
            with pytest.raises(MsckfError) as e:
                bad()
            assert rc_of(e) == -1
        for lane, (ids, uv) in msgs.items():             # a refused put leaves the message as it was
            same_message(fe.tracks_msg_get(lane), ids, uv)
        for l, t in enumerate(tables):                   # the track tables never saw any of it
            tt.same_table(fe.tracks_get(l), t)
        assert [r.n > 0 for r in fe.tracks_step(args, tt.THRESHOLD, **STEP)] == [True] * 3   # and the context works
    finally:
        fe.close()
    bare = fe_mod.Frontend(tt.W, tt.H, nslot=3, max_level=1, max_points=64)
    try:
        with pytest.raises(MsckfError) as e:             # no tables, no messages
            bare.tracks_msg_put(0, np.arange(3), np.zeros((3, 4)))
        assert rc_of(e) == -1
    finally:
        bare.close()


def second_frame(fe, lanes, seeds=(21, 22, 23)):
    """Frame 2 into the slots a second step reads (tests/test_gpu_tracks.py's rotation)."""
    frames = {l: tt.lane_frames(seeds[l]) for l in lanes}
    fe.upload_many([s for l in lanes for s in (3 * l + 1, 3 * l + 2)],
                   np.stack([frames[l][2][j] for l in lanes for j in range(2)]))
    return [tt.lane_args(l, 0, l == 0, 1, seeds[l]) for l in lanes]


def same_step(ra, rb, fe_a, fe_b, lanes):
    """``rb`` (to_message) against ``ra``: the numbers, the tables and the message."""
    for a, b, l in zip(ra, rb, lanes):
        assert b.ids is None and b.uv is None
        assert a.n == b.n and a.n_total == b.n_total and a.next_id == b.next_id
        np.testing.assert_array_equal(a.counters, b.counters)
        same_message(fe_b.tracks_msg_get(l), a.ids, a.uv)
    for l in range(3):
        for x, y in zip(fe_a.tracks_get(l), fe_b.tracks_get(l)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_step_msg_equals_step():
    """Three lanes (lane 0 with RANSAC, lane 2 empty), then a subset in another
    order; the -3 step; what invalidates a message."""
    (fe_a, tables, args), (fe_b, _, _) = tt.small_context(), tt.small_context()
    try:
        assert args[0].ransac is not None and args[1].ransac is None and len(tables[2].ids) == 0
        ra = fe_a.tracks_step(args, tt.THRESHOLD, **STEP)
        rb = fe_b.tracks_step(args, tt.THRESHOLD, to_message=True, **STEP)
        same_step(ra, rb, fe_a, fe_b, [0, 1, 2])
        assert ra[0].n > 0 and ra[2].n > 0 and ra[0].counters[3] < ra[0].counters[0]
        kept = fe_b.tracks_msg_get(1)
        # a subset, lane 2 before lane 0: the unnamed lane 1 keeps its message
        sub = second_frame(fe_a, [2, 0])
        second_frame(fe_b, [2, 0])
        ra2 = fe_a.tracks_step(sub, tt.THRESHOLD, **STEP)
        rb2 = fe_b.tracks_step(sub, tt.THRESHOLD, to_message=True, **STEP)
        same_step(ra2, rb2, fe_a, fe_b, [2, 0])
        assert ra2[1].counters[0] == ra[0].n > 0        # the second step read what the first wrote
        same_message(fe_b.tracks_msg_get(1), *kept[1:])
        # -3: the named lanes' messages are invalid, the unnamed lane's and every table untouched
        before = [fe_b.tracks_get(l) for l in range(3)]
        with pytest.raises(MsckfError, match="rc=-3") as e:
            fe_b.tracks_step(sub, tt.THRESHOLD, max_kp=8, to_message=True, **STEP)
        assert len(e.value.n_total) == 2 and max(e.value.n_total) > 8
        assert not fe_b.tracks_msg_get(2)[0] and not fe_b.tracks_msg_get(0)[0]
        same_message(fe_b.tracks_msg_get(1), *kept[1:])
        for l in range(3):
            for x, y in zip(before[l], fe_b.tracks_get(l)):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        # a bad argument is refused before anything changes: lane 1's message stays
        with pytest.raises(MsckfError, match="rc=-1"):
            fe_b.tracks_step([sub[0], sub[0]], tt.THRESHOLD, to_message=True, **STEP)
        same_message(fe_b.tracks_msg_get(1), *kept[1:])
        # the same step again succeeds and equals the host-fed path's third step
        ra3 = fe_a.tracks_step(sub, tt.THRESHOLD, **STEP)
        rb3 = fe_b.tracks_step(sub, tt.THRESHOLD, to_message=True, **STEP)
        same_step(ra3, rb3, fe_a, fe_b, [2, 0])
        # mfe_tracks_put and mfe_tracks_step invalidate the lanes they name, and only those
        t = fe_b.tracks_get(2)
        fe_b.tracks_put(2, *t)
        assert not fe_b.tracks_msg_get(2)[0] and fe_b.tracks_msg_get(0)[0] and fe_b.tracks_msg_get(1)[0]
        fe_b.tracks_step(sub[1:], tt.THRESHOLD, **STEP)
        assert not fe_b.tracks_msg_get(0)[0] and fe_b.tracks_msg_get(1)[0]
    finally:
        fe_a.close()
        fe_b.close()


# ------------------------------------------- the map fed from the messages --
def same_outputs(got, want, what=""):
    assert len(got) == len(want)
    for w, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0] and a[1] == b[1], (what, w)
        np.testing.assert_array_equal(a[2], b[2], err_msg="%s filter %d" % (what, w))
        np.testing.assert_array_equal(a[3], b[3], err_msg="%s filter %d" % (what, w))


def same_maps(a, b, filters, what=""):
    for f in filters:
        for x, y in zip(a.map_get(f), b.map_get(f)):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (what, f)


def host_fed(ctx, filters, msgs):
    off = np.cumsum([0] + [len(m[0]) for m in msgs])
    return ctx.map_add_lost(filters, off, np.concatenate([m[0] for m in msgs]).astype(np.int64),
                            np.concatenate([m[1] for m in msgs]).reshape(-1, 4))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_add_lost_tracks_equals_add_lost(dtype):
    """Messages of every size of SIZES into a 300-row table (above one pass), next
    to two smaller filters, filters [2, 0, 1] fed from lanes [0, 2, 1] with unequal
    n; then a subset of the filters."""
    cap, ncams = 1024, [6, 7, 8]
    prs = [tm.small_problem(6, 1), tm.small_problem(7, 3), tm.small_problem(8, 2)]
    a, b = tm.make_ctx(prs, 8, dtype, cap=cap), tm.make_ctx(prs, 8, dtype, cap=cap)
    fe = message_tables()
    try:
        rng = np.random.default_rng(11)
        tabs = {0: fc.random_table(rng, 40, 8, ncams[0]), 1: fc.random_table(rng, 100, 8, ncams[1]),
                2: fc.random_table(rng, 300, 8, ncams[2])}
        _, big_ids, big_z = fc.big_messages(rng, tabs[2], cap)[0]
        assert len(big_ids) >= max(SIZES)
        small = fc.messages(rng, tabs[0], cap)
        mid = fc.messages(rng, tabs[1], cap)
        for k, size in enumerate(SIZES):
            for ctx in (a, b):
                for f, t in tabs.items():
                    tm.put(ctx, f, t)
            msgs = [(big_ids[:size], big_z[:size]), small[k % len(small)][1:], mid[k % len(mid)][1:]]   # filters 2, 0, 1
            if size >= 64:   # a mixed message: tracked and new ids
                row = set(tabs[2]["ids"].tolist())
                hits = sum(int(i) in row for i in msgs[0][0])
                assert 0 < hits < size
            for lane, m in zip((0, 2, 1), msgs):
                fe.tracks_msg_put(lane, *m)
            want = host_fed(a, [2, 0, 1], msgs)
            got = b.map_add_lost_tracks([2, 0, 1], fe, [0, 2, 1])
            same_outputs(got, want, "size %d" % size)
            same_maps(a, b, (0, 1, 2), "size %d" % size)
            assert want[0][1] == 300 and len(want[0][2]) > 0                           # candidates in the large table
            for lane, m in zip((0, 2, 1), msgs):                                       # the messages stay, and stay valid
                same_message(fe.tracks_msg_get(lane), *m)
            # a subset: filter 1 alone, from lane 0's message (the large one)
            want = host_fed(a, [1], msgs[:1])
            got = b.map_add_lost_tracks([1], fe, [0])
            same_outputs(got, want, "subset, size %d" % size)
            same_maps(a, b, (0, 1, 2), "subset, size %d" % size)
    finally:
        a.close()
        b.close()
        fe.close()


def test_add_lost_tracks_overflow_and_errors():
    """feature_map_cases.overflow_case: -3, every table and the lost-form refusal
    as in the host-fed call; then the -1 checks, each leaving tables and messages."""
    rng = np.random.default_rng(3)
    prs = [tm.small_problem(6, 1), tm.small_problem(6, 2)]
    a, b = tm.make_ctx(prs, 8, cap=1024), tm.make_ctx(prs, 8, cap=1024)
    bare = tm.make_ctx(prs[:1], 8, with_map=False)
    fe, plain = message_tables(), fe_mod.Frontend(tt.W, tt.H, nslot=3, max_level=1, max_points=64)
    try:
        t, ids, z = fc.overflow_case(1024)
        assert len(ids) <= FE_CAP
        small = fc.random_table(rng, 20, 8, 6)
        empty = (np.zeros(0, np.int64), np.zeros((0, 4)))
        fe.tracks_msg_put(0, ids, z)
        fe.tracks_msg_put(1, *empty)
        for ctx in (a, b):
            tm.put(ctx, 0, t)
            tm.put(ctx, 1, small)
        # filter 1 has a lost table from a good call, and its descriptor loads
        want = host_fed(a, [1], [empty])
        got = b.map_add_lost_tracks([1], fe, [1])
        same_outputs(got, want)
        info = got[0][3]
        assert len(info) > 0
        nxt1 = fr.add_lost(small, *empty, 5, 1024)[0]
        for ctx in (a, b):
            ctx.map_load(_lib.MAP_LOAD_LOST, [1], [0, len(info)], info[:, 3], info[:, 0])
        with pytest.raises(MsckfError) as e:
            host_fed(a, [1, 0], [empty, (ids, z)])
        assert rc_of(e) == -3
        with pytest.raises(MsckfError) as e:
            b.map_add_lost_tracks([1, 0], fe, [1, 0])
        assert rc_of(e) == -3
        for ctx in (a, b):
            tm.assert_table(ctx, 0, t)
            tm.assert_table(ctx, 1, nxt1)
            with pytest.raises(MsckfError) as e:     # the failed call wrote over filter 1's lost table
                ctx.map_load(_lib.MAP_LOAD_LOST, [1], [0, len(info)], info[:, 3], info[:, 0])
            assert rc_of(e) == -1
        same_message(fe.tracks_msg_get(0), ids, z)
        fe.tracks_msg_put(2, ids[:-1], z[:-1])       # one id fewer fills the map exactly
        want = host_fed(a, [0], [(ids[:-1], z[:-1])])
        got = b.map_add_lost_tracks([0], fe, [2])
        same_outputs(got, want)
        assert got[0][0] == 300 and got[0][1] == 700
        same_maps(a, b, (0, 1))
        # ---- -1, before anything is copied or launched
        state = [b.map_get(f) for f in (0, 1)]
        fresh = message_tables()                     # lanes that never got a message
        try:
            for call in (lambda: b.map_add_lost_tracks([0], fresh, [0]),            # no valid message
                         lambda: b.map_add_lost_tracks([0, 1], fe, [0, 0]),         # a lane named twice
                         lambda: b.map_add_lost_tracks([0], fe, [3]),               # lanes out of range
                         lambda: b.map_add_lost_tracks([0], fe, [-1]),
                         lambda: b.map_add_lost_tracks([0], plain, [0]),            # a front-end without tracks
                         lambda: b.map_add_lost_tracks([2], fe, [0]),               # the checks of msckf_map_add_lost
                         lambda: b.map_add_lost_tracks([0, 0], fe, [0, 1]),
                         lambda: bare.map_add_lost_tracks([0], fe, [0])):
                with pytest.raises(MsckfError) as e:
                    call()
                assert rc_of(e) == -1
            fe.tracks_put(1, np.arange(4), np.ones(4), np.zeros((4, 2)), np.zeros((4, 2)), 9)
            with pytest.raises(MsckfError) as e:     # tracks_put made lane 1's message invalid
                b.map_add_lost_tracks([0], fe, [1])
            assert rc_of(e) == -1
        finally:
            fresh.close()
        for f, st in zip((0, 1), state):
            for x, y in zip(st, b.map_get(f)):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        same_message(fe.tracks_msg_get(0), ids, z)
        same_message(fe.tracks_msg_get(2), ids[:-1], z[:-1])
        assert not fe.tracks_msg_get(1)[0]
        # the lost table of the last good call is still there: the -1 calls launched nothing
        info = got[0][3]
        b.map_load(_lib.MAP_LOAD_LOST, [0], [0, len(info)], info[:, 3], info[:, 0])
    finally:
        for c in (a, b, bare, fe, plain):
            c.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lost_load_after_the_hand_off(dtype):
    """A lost-form msckf_map_load plus update after the hand-off gives the
    results and the filter states it gives after the host-fed call (the tables of
    tests/test_gpu_feature_map.py's check_lost_load)."""
    rng = np.random.default_rng(5)
    prs = [synth.make_update_problem(8, 30, seed=11), None, synth.make_update_problem(6, 24, seed=12)]
    a, b = tm.make_ctx(prs, 10, dtype), tm.make_ctx(prs, 10, dtype)
    fe = message_tables()
    try:
        tabs = {f: tm.problem_table(prs[f], 10, rng, drop_newest=True) for f in (0, 2)}
        msgs = [(rng.permutation(tabs[f]["ids"])[:5], rng.standard_normal((5, 4))) for f in (0, 2)]
        for ctx in (a, b):
            for f in (0, 2):
                tm.put(ctx, f, tabs[f])
        for lane, m in zip((2, 1), msgs):
            fe.tracks_msg_put(lane, *m)
        want = host_fed(a, [0, 2], msgs)
        got = b.map_add_lost_tracks([0, 2], fe, [2, 1])
        same_outputs(got, want)
        assert all(len(g[2]) >= 10 for g in got)
        off = np.cumsum([0] + [len(g[2]) for g in got])
        rows, counts = np.concatenate([g[3][:, 3] for g in got]), np.concatenate([g[3][:, 0] for g in got])
        for ctx in (a, b):
            ctx.map_load(_lib.MAP_LOAD_LOST, [0, 2], off, rows, counts)
            ctx.batch_update(row_cap=1500, triangulate=True)
        ra, rb = a.batch_results(), b.batch_results()
        tm.assert_same_results(ra, rb)
        assert ra[0].any() and ra[3].any() and ra[4].max() > 0
        tm.assert_same_state(a, b, (0, 2))
        same_maps(a, b, (0, 2))
    finally:
        a.close()
        b.close()
        fe.close()


def test_step_hand_off_step_hand_off():
    """Ordering: a step, the hand-off, the next step, the hand-off -- the second
    call reads the second message.  Frame by frame against the host-fed path
    (mfe_tracks_step, then msckf_map_add_lost with its arrays)."""
    (fe_a, _, args), (fe_b, _, _) = tt.small_context(), tt.small_context()
    prs = [tm.small_problem(6, 1), tm.small_problem(7, 3), tm.small_problem(8, 2)]
    a, b = tm.make_ctx(prs, 8), tm.make_ctx(prs, 8)
    try:
        filters, lanes = [2, 0, 1], [0, 2, 1]
        seen = []
        for frame in range(2):
            if frame:
                args = second_frame(fe_a, [0, 1, 2])
                second_frame(fe_b, [0, 1, 2])
            ra = fe_a.tracks_step(args, tt.THRESHOLD, **STEP)
            rb = fe_b.tracks_step(args, tt.THRESHOLD, to_message=True, **STEP)
            assert [r.n for r in ra] == [r.n for r in rb] and min(r.n for r in ra) > 0
            want = host_fed(a, filters, [(ra[l].ids, ra[l].uv) for l in lanes])
            got = b.map_add_lost_tracks(filters, fe_b, lanes)
            same_outputs(got, want, "frame %d" % frame)
            same_maps(a, b, (0, 1, 2), "frame %d" % frame)
            seen.append([(g[0], g[1]) for g in got])
        # frame 0 fills empty maps; frame 1 tracks the survivors and appends the new features
        assert all(t == 0 and nb == 0 for t, nb in seen[0])
        assert all(0 < t <= nb for t, nb in seen[1])
        assert len(b.map_get(2)[0]) >= seen[1][0][1] > 0
    finally:
        for c in (a, b, fe_a, fe_b):
            c.close()
