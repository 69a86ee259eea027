"""msckf_keyframe_select (include/msckf_keyframes.h) on the GPU.  Every
comparison is exact:
  * the slots against the numpy restatement tests/keyframe_ref.py on its fixed
    cases (tests/test_keyframe_ref.py holds them against the host's method and
    asserts what they cover), in fp64 and fp32 contexts of four filters with 4,
    5, 22 and 70 cam states, three of them named out of slot order; descriptors
    and tables against tests/feature_map_ref.py; the loads and the commit that
    follow against msckf_map_prune_select with the same slots on a twin context;
  * the deferred results of a lost-form update ride in the call's copy, and the
    choice reads the cam states as that update left them;
  * errors leave tables, open select and outputs as they were; a repeat gives
    the same bits;
  * MSCKF / MultiMSCKF(device_map=True, device_keyframes=True) against
    device_map=True alone, end to end."""
import ctypes as C
import re

import numpy as np
import pytest

import msckf_amd
from conftest import golden
from msckf_amd import FilterConfig, MsckfError, _lib, synth
from msckf_amd._lib import Context, pack_cams, pack_imu
from msckf_amd.replay import FeatureStream, replay
from msckf_amd.scheduler import MultiMSCKF
import feature_map_ref as fr
import keyframe_ref as kr
from feature_map_cases import random_table, weird_ids

pytestmark = pytest.mark.gpu

NMAX, CAP = 72, 512
ROWS = (0, 1, 37, 300)
ORDERS = ([2, 0, 3], [3, 1, 0])       # three of the four filters, out of slot order; between them every filter


# ------------------------------------------------------------------ helpers --
_PROBLEMS, _TABLES = {}, {}


def problem(n):
    if n not in _PROBLEMS:
        _PROBLEMS[n] = synth.make_update_problem(n, 2, seed=60 + n)
    return _PROBLEMS[n]


def table(rows, ncams):
    if (rows, ncams) not in _TABLES:
        _TABLES[rows, ncams] = random_table(np.random.default_rng(1000 * rows + ncams), rows, NMAX, ncams,
                                            newest_free=False)
    return _TABLES[rows, ncams]


def put(ctx, f, t):
    ctx.map_put(f, t["ids"], fr.mask_words(t["obs"]), t["z"], t["p_w"], t["init"])


def assert_table(ctx, f, t, msg=""):
    ids, mask, z, p_w, init = ctx.map_get(f)
    np.testing.assert_array_equal(ids, t["ids"], err_msg=msg)
    np.testing.assert_array_equal(mask, fr.mask_words(t["obs"]), err_msg=msg)
    np.testing.assert_array_equal(z, fr.masked_z(t), err_msg=msg)
    np.testing.assert_array_equal(p_w, t["p_w"], err_msg=msg)
    np.testing.assert_array_equal(init, t["init"], err_msg=msg)


def assert_same_tables(a, b, slots):
    for f in slots:
        for x, y in zip(a.map_get(f), b.map_get(f)):
            np.testing.assert_array_equal(x, y)


def rc_of(err):
    return int(re.search(r"rc=(-?\d+)", str(err.value)).group(1))


def four_filter_ctx(dtype):
    """Filters 0..3 with 4, 5, 22 and 70 cam states (kr.SIZES), cam capacity 72."""
    ctx = Context(FilterConfig(), n_filters=4, n_cam_capacity=NMAX, dtype=dtype)
    for f, n in enumerate(kr.SIZES):
        pr = problem(n)
        ctx.set_state(f, pack_imu(gravity=pr.gravity, alias=True, **pr.imu),
                      pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P)
    ctx.map_create(CAP)
    return ctx


def set_cams(ctx, f, cams):
    pr = problem(len(cams))
    ctx.set_state(f, pack_imu(gravity=pr.gravity, alias=True, **pr.imu), cams, None)


@pytest.fixture(scope="module", params=[np.float64, np.float32], ids=["fp64", "fp32"])
def pair(request):
    dev, twin = four_filter_ctx(request.param), four_filter_ctx(request.param)
    yield request.param, dev, twin
    dev.close()
    twin.close()


def offs(xs):
    return np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)


def cat(xs, dt):
    return np.concatenate([np.asarray(x, dt) for x in xs])


def load_group(dev, twin, g, group, dtype):
    """The group's cams into both contexts' filters, tables of ROWS rows in a
    turn that depends on the group; returns {filter: (stored cams, rate, table)}."""
    out = {}
    for f, case in enumerate(group):
        want = kr.rounded(case)["cams"] if dtype == np.float32 else case["cams"]
        tab = table(ROWS[(f + g) % 4], case["n"])
        for ctx in (dev, twin):
            set_cams(ctx, f, case["cams"])
            put(ctx, f, tab)
        stored = dev.get_state(f, want_P=False)[1]
        np.testing.assert_array_equal(stored, want)          # the context stores the poses cast to its scalar
        out[f] = (stored, case["rate"], tab)
    return out


def select_and_follow(dev, twin, named, st, msg):
    """msckf_keyframe_select on ``dev`` against the references, then the loads and
    the commit on both contexts.  Returns what the device returned."""
    got = dev.keyframe_select(named, [st[f][1] for f in named])
    slots, tabs, infos = {}, {}, {}
    for w, f in enumerate(named):
        cams, rate, tab = st[f]
        ref = kr.choice(cams, rate)
        np.testing.assert_array_equal(got[w][0], ref.slots, err_msg="%s filter %d" % (msg, f))
        slots[f] = ref.slots
        tabs[f], iid, infos[f] = fr.prune_select(tab, fr.removed_mask(ref.slots, NMAX))
        np.testing.assert_array_equal(got[w][1], iid)
        np.testing.assert_array_equal(got[w][2], infos[f])
        assert_table(dev, f, tabs[f], "select %s filter %d" % (msg, f))
    for f in set(st) - set(named):                            # the filter not named keeps its table
        assert_table(dev, f, st[f][2])
    sel = twin.map_prune_select(named, offs([slots[f] for f in named]), cat([slots[f] for f in named], np.int32))
    for w in range(len(named)):
        np.testing.assert_array_equal(sel[w][0], got[w][1])
        np.testing.assert_array_equal(sel[w][1], got[w][2])
    assert_same_tables(dev, twin, named)
    # the open select serves both prune forms of msckf_map_load and the commit
    tri = {f: infos[f][~infos[f][:, 2].astype(bool)] for f in named}
    ents = {f: (tri[f][:, 3], np.zeros(len(tri[f]), bool), np.zeros((len(tri[f]), 3))) for f in named}
    if sum(len(tri[f]) for f in named):
        res = []
        for ctx in (dev, twin):
            rng_t = ctx.map_load(_lib.MAP_LOAD_PRUNE_TRI, named, offs([tri[f] for f in named]),
                                 cat([tri[f][:, 3] for f in named], np.int32),
                                 cat([tri[f][:, 0] for f in named], np.int32))
            ctx.batch_triangulate()
            res.append(ctx.batch_results())
        np.testing.assert_array_equal(res[0][2], res[1][2])
        np.testing.assert_array_equal(res[0][3], res[1][3])
        for f in named:
            a, b = rng_t[f]
            ents[f] = (tri[f][:, 3], res[0][3][a:b], res[0][2][a:b])
    if sum(len(infos[f]) for f in named):
        pw = np.full((sum(len(infos[f]) for f in named), 3), np.nan)
        for ctx in (dev, twin):
            ctx.map_load(_lib.MAP_LOAD_PRUNE_UPDATE, named, offs([infos[f] for f in named]),
                         cat([infos[f][:, 3] for f in named], np.int32),
                         cat([infos[f][:, 1] for f in named], np.int32), pw)
    for ctx in (dev, twin):
        ctx.map_prune_commit(named, offs([ents[f][0] for f in named]), cat([ents[f][0] for f in named], np.int32),
                             cat([ents[f][1] for f in named], np.uint8),
                             np.concatenate([np.asarray(ents[f][2], float).reshape(-1, 3) for f in named]))
    assert_same_tables(dev, twin, named)
    for f in named:
        assert_table(dev, f, fr.prune_commit(tabs[f], fr.removed_mask(slots[f], NMAX), *ents[f]),
                     "commit %s filter %d" % (msg, f))
    return got


# ------------------------------------------- the choice and the select in it --
def test_choice_and_select_vs_reference(pair):
    dtype, dev, twin = pair
    seen = set()
    for g, group in enumerate(kr.groups()):
        for named in ORDERS:
            st = load_group(dev, twin, g, group, dtype)
            select_and_follow(dev, twin, named, st, "group %d %s" % (g, named))
            seen.update((f, kr.choice(st[f][0], st[f][1]).outcome) for f in named)
    # every outcome was asked of every filter (size), the second mask word included
    assert seen == {(f, o) for f in range(4) for o in kr.OUTCOMES}


def test_repeat_gives_the_same_bits(pair):
    dtype, dev, twin = pair
    group, named = kr.groups()[1], ORDERS[0]
    runs = []
    for rep in range(2):
        st = load_group(dev, twin, 3, group, dtype)           # the state restored: cams and tables put again
        got = dev.keyframe_select(named, [st[f][1] for f in named])
        out = [x for r in got for x in r]
        for f in range(4):
            out.extend(dev.map_get(f))
        runs.append(out)
    assert len(runs[0]) == len(runs[1]) and any(len(r[1]) for r in got)
    for x, y in zip(*runs):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------ deferred results ride along --
def problem_table(pr, Nmax, rng):
    """The problem's tracks without their newest observation as a table (map
    order = feature order); every second row initialised at its landmark."""
    t = fr.empty(Nmax)
    F = pr.F
    obs, z = np.zeros((F, Nmax), bool), np.zeros((F, Nmax, 4))
    for f in range(F):
        for r in range(pr.obs_off[f], pr.obs_off[f + 1]):
            if pr.obs_cam[r] == pr.N - 1:
                continue
            obs[f, pr.obs_cam[r]] = True
            z[f, pr.obs_cam[r]] = pr.obs_z[r]
    t["ids"] = weird_ids(rng, F)
    t["obs"], t["z"] = obs, z
    t["init"] = np.arange(F) % 2 == 0
    t["p_w"] = np.where(t["init"][:, None], pr.landmarks + 1e-3 * rng.standard_normal((F, 3)), 0.0)
    return t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_deferred_results_ride_along(dtype):
    """A lost-form update of filters 0 and 2 is enqueued and its Pending kept;
    msckf_keyframe_select then returns its results in its own copy -- what
    msckf_batch_results returns on the twin -- and chooses from the cam states
    the update left (the twin's, read after its update)."""
    rng = np.random.default_rng(5)
    prs = [synth.make_update_problem(8, 30, seed=11), None, synth.make_update_problem(6, 24, seed=12)]
    ctxs = []
    for _ in range(2):
        ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=10, dtype=dtype)
        for f in (0, 2):
            ctx.set_state(f, pack_imu(gravity=prs[f].gravity, alias=True, **prs[f].imu),
                          pack_cams(prs[f].cam_q, prs[f].cam_p, prs[f].cam_q_null), prs[f].P)
        ctx.map_create(256)
        ctxs.append(ctx)
    dev, twin = ctxs
    try:
        tabs = {f: problem_table(prs[f], 10, rng) for f in (0, 2)}
        msg = {f: (rng.permutation(tabs[f]["ids"])[:5], rng.standard_normal((5, 4))) for f in (0, 2)}
        before = {f: dev.get_state(f, want_P=False)[1] for f in (0, 2)}
        for ctx in (dev, twin):
            for f in (0, 2):
                put(ctx, f, tabs[f])
            got = ctx.map_add_lost([0, 2], [0, 5, 10], np.concatenate([msg[0][0], msg[2][0]]),
                                   np.concatenate([msg[0][1], msg[2][1]]))
            infos = {f: got[w][3] for w, f in enumerate((0, 2))}
            ranges = ctx.map_load(_lib.MAP_LOAD_LOST, [0, 2], offs([infos[0], infos[2]]),
                                  cat([infos[f][:, 3] for f in (0, 2)], np.int32),
                                  cat([infos[f][:, 0] for f in (0, 2)], np.int32))
            ctx.batch_update(row_cap=1500, triangulate=True)
        cur = {f: fr.add_lost(tabs[f], msg[f][0], msg[f][1], prs[f].N - 1, 256)[0] for f in (0, 2)}
        pends = dev.pending([(f,) + ranges[f] for f in (0, 2)])
        assert dev._pending is not None
        rates = {0: 0.9, 2: 0.9}
        got = dev.keyframe_select([2, 0], [rates[2], rates[0]])
        assert dev._pending is None                            # read in the select's copy
        ref = twin.batch_results()
        assert ref[0].any() and ref[3].any() and ref[4].max() > 0
        for pend, f in zip(pends, (0, 2)):
            a, b = ranges[f]
            acc, gam, p, v, rows = pend.get()
            np.testing.assert_array_equal(acc, ref[0][a:b])
            np.testing.assert_array_equal(gam, ref[1][a:b])
            np.testing.assert_array_equal(p, ref[2][a:b])
            np.testing.assert_array_equal(v, ref[3][a:b])
            assert rows == ref[4][f]
        assert dev._pending is None                            # and Pending.get() read nothing more
        for w, f in enumerate((2, 0)):
            after = twin.get_state(f, want_P=False)[1]
            assert (after != before[f]).any()                  # the update moved the cam states
            ch = kr.choice(after, rates[f])
            np.testing.assert_array_equal(got[w][0], ch.slots)
            nxt, iid, info = fr.prune_select(cur[f], fr.removed_mask(ch.slots, 10))
            np.testing.assert_array_equal(got[w][1], iid)
            np.testing.assert_array_equal(got[w][2], info)
            assert_table(dev, f, nxt)
        for x, y in zip(dev.get_state(0), twin.get_state(0)):
            np.testing.assert_array_equal(x, y)
    finally:
        dev.close()
        twin.close()


# ------------------------------------------------------------------- errors --
def raw_select(ctx, filters, rates, slots):
    """The C call itself, so that the caller's slot array can be looked at after an error."""
    filters, rates = np.ascontiguousarray(filters, np.int32), np.ascontiguousarray(rates, np.float64)
    k = len(filters)
    ninv = np.zeros(k, np.int32)
    did, dinfo = np.zeros((k, ctx.map_cap or 1), np.int64), np.zeros((k, ctx.map_cap or 1, _lib.MAP_INFO), np.int32)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    return ctx.lib.msckf_keyframe_select(ctx.h, k, p(filters, C.c_int32), p(rates, C.c_double), 0.2618, 0.4, 0.5,
                                         p(slots, C.c_int32), p(ninv, C.c_int32), p(did, C.c_int64),
                                         p(dinfo, C.c_int32), None, None, None, None, None)


def test_errors_leave_tables_select_and_slots():
    rng = np.random.default_rng(3)
    prs = [synth.make_update_problem(6, 2, seed=s) for s in (1, 2, 3)]
    ncams = [6, 3, 6]                                          # filter 1 keeps the first three cam states only

    def make(with_map):
        ctx = Context(FilterConfig(), n_filters=3, n_cam_capacity=8)
        for f, pr in enumerate(prs):
            n, D = ncams[f], 21 + 6 * ncams[f]
            ctx.set_state(f, pack_imu(gravity=pr.gravity, alias=True, **pr.imu),
                          pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null)[:n], pr.P[:D, :D])
        if with_map:
            ctx.map_create(256)
        return ctx
    ctx, bare = make(True), make(False)
    try:
        tabs = {f: random_table(rng, 40 + f, 8, ncams[f], newest_free=False) for f in range(3)}
        for f in range(3):
            ctx.map_put(f, tabs[f]["ids"], fr.mask_words(tabs[f]["obs"]), tabs[f]["z"], tabs[f]["p_w"],
                        tabs[f]["init"])
        # an open select of filter 0, from a good call
        got = ctx.keyframe_select([0], [0.9])[0]
        ch = kr.choice(ctx.get_state(0, want_P=False)[1], 0.9)
        np.testing.assert_array_equal(got[0], ch.slots)
        rm0 = fr.removed_mask(ch.slots, 8)
        tabs[0], iid, info = fr.prune_select(tabs[0], rm0)
        np.testing.assert_array_equal(got[2], info)

        def unchanged():
            for f in range(3):
                assert_table(ctx, f, tabs[f])
        for filters in ([2, 1], [1], [0, 1, 2]):               # filter 1 has 3 cam states
            slots = np.full((len(filters), 2), -7, np.int32)
            assert raw_select(ctx, filters, [0.9] * len(filters), slots) == -1
            assert "cam states" in ctx.lib.msckf_last_error().decode()
            assert (slots == -7).all()
            unchanged()
        for call in (lambda: ctx.keyframe_select([2, 2], [0.9, 0.9]),      # a filter named twice
                     lambda: ctx.keyframe_select([3], [0.9]),              # no such filter
                     lambda: ctx.keyframe_select([-1], [0.9]),
                     lambda: bare.keyframe_select([0], [0.9])):            # no map created
            with pytest.raises(MsckfError) as e:
                call()
            assert rc_of(e) == -1
            unchanged()
        slots = np.full((1, 2), -7, np.int32)
        assert raw_select(bare, [0], [0.9], slots) == -1 and (slots == -7).all()
        # filter 0's select is still open with its slots: both prune loads and the commit go through
        tri = info[~info[:, 2].astype(bool)]
        assert len(tri)
        ctx.map_load(_lib.MAP_LOAD_PRUNE_TRI, [0], [0, len(tri)], tri[:, 3], tri[:, 0])
        ctx.batch_triangulate()
        res = ctx.batch_results()
        ctx.map_prune_commit([0], [0, len(tri)], tri[:, 3], res[3], res[2])
        tabs[0] = fr.prune_commit(tabs[0], rm0, tri[:, 3], res[3], res[2])
        unchanged()
        with pytest.raises(MsckfError) as e:                   # and is closed now
            ctx.map_prune_commit([0], [0, 0], [], [], np.zeros((0, 3)))
        assert rc_of(e) == -1
        # a valid call afterwards
        got = ctx.keyframe_select([2], [0.2])[0]
        np.testing.assert_array_equal(got[0], [0, 1])          # the rate is below the threshold: the two oldest
        nxt, iid, info = fr.prune_select(tabs[2], fr.removed_mask([0, 1], 8))
        np.testing.assert_array_equal(got[1], iid)
        np.testing.assert_array_equal(got[2], info)
        assert_table(ctx, 2, nxt)
    finally:
        ctx.close()
        bare.close()


# --------------------------------------------------------------- end to end --
def late_start(st, k0):
    a = int(st.frame_off[k0])
    return FeatureStream(st.imu, st.frame_t[k0:], st.frame_off[k0:] - a, st.feat_id[a:], st.feat_z[a:], st.gt)


_STREAMS = []


def streams():
    if not _STREAMS:
        g = golden("sequence_s1")
        _STREAMS.extend([FeatureStream.from_synthetic(synth.make_sequence(int(g["n_frames"]), int(g["seed"]))),
                         FeatureStream.from_synthetic(synth.make_sequence(90, 7)),
                         late_start(FeatureStream.from_synthetic(synth.make_sequence(140, 11)), 7)])
    return _STREAMS


@pytest.fixture
def outcomes(monkeypatch):
    """Records the outcome of every choice the runs of a test make (printed, not
    asserted: it depends on the poses the device computed)."""
    seen, n = [], FilterConfig().max_cam_state_size
    names = {(n - 3, n - 2): "both_newest", (0, n - 2): "oldest_second", (0, n - 3): "oldest_first",
             (0, 1): "two_oldest"}
    inner = Context.keyframe_select

    def recording(self, filters, rates, *a, **kw):
        out = inner(self, filters, rates, *a, **kw)
        seen.extend(names.get(tuple(int(s) for s in r[0]), "other %s" % (r[0],)) for r in out)
        return out
    monkeypatch.setattr(Context, "keyframe_select", recording)
    yield seen
    print("keyframe outcomes taken: %s" % {k: seen.count(k) for k in sorted(set(seen))})


def single(st, dtype, **kw):
    flt = msckf_amd.MSCKF(dtype=dtype, device_map=True, **kw)
    try:
        traj = replay(flt, st)
        return traj, flt.gate_log, flt.gamma_log, flt.shape_log, flt.state_cov(), list(flt.cam_ids)
    finally:
        flt.close()


def assert_same_run(a, b):
    np.testing.assert_array_equal(a[0].t, b[0].t)
    np.testing.assert_array_equal(a[0].p, b[0].p)
    assert a[1] == b[1] and len(a[1]) > 100
    assert a[2] == b[2]
    assert a[3] == b[3]
    np.testing.assert_array_equal(a[4], b[4])
    assert a[5] == b[5]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_keyframes_equal_host_choice(dtype, which, outcomes):
    st = streams()[which]
    assert_same_run(single(st, dtype, device_keyframes=True), single(st, dtype))
    assert len(outcomes) > 10


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_device_keyframes_equal_host_choice(dtype, outcomes):
    sts = streams()
    out = []
    for kw in ({"device_keyframes": True}, {}):
        ms = MultiMSCKF(3, dtype=dtype, device_map=True, **kw)
        try:
            trajs = ms.run_streams(sts, arrays=True)
            out.append(([(trajs[i], ln.gate_log, ln.gamma_log, ln.shape_log, ln.state_cov(), list(ln.cam_ids))
                         for i, ln in enumerate(ms.lanes)], dict(ms.launches)))
        finally:
            ms.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert_same_run(a, b)
    la, lb = out[0][1], out[1][1]
    print("launches with device_keyframes: %s\nlaunches without: %s" % (la, lb))
    assert la["map_keyframe_select"] > 0 and "map_prune_select" not in la
    assert la["map_prune_commit"] == la["map_keyframe_select"]
    assert "map_keyframe_select" not in lb and lb["map_prune_select"] == lb["map_prune_commit"]
    assert la["states"] < lb["states"]
