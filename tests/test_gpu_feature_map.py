"""The feature map kept on the device (include/msckf_map.h) on the GPU.  Every
comparison is exact:
  * each call against the numpy reference tests/feature_map_ref.py, tables
    written by msckf_map_put and read by msckf_map_get -- within one 256-row
    pass of the kernels (cap 256) and beyond it (cap 1024 and 2048, tables up
    to 2048 rows, messages up to 800; the inputs are tests/feature_map_cases.py);
  * msckf_map_load + the unchanged update chain against msckf_batch_load of the
    reference's arrays + the same chain on a second context, all three forms;
  * MSCKF(device_map=True) / MultiMSCKF(.., device_map=True) against the host
    map end to end; a forced online reset;
  * errors leave the tables as they were; repeats give the same bits."""
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
import feature_map_cases as fc
from feature_map_cases import messages, random_table, weird_ids

pytestmark = pytest.mark.gpu

CAP = 256


# ------------------------------------------------------------------ helpers --
def set_problem_state(ctx, f, pr):
    imu = pack_imu(gravity=pr.gravity, alias=True, **pr.imu)
    ctx.set_state(f, imu, pack_cams(pr.cam_q, pr.cam_p, pr.cam_q_null), pr.P)


def make_ctx(problems, Nmax, dtype=np.float64, cap=CAP, with_map=True):
    """A context with one slot per entry of ``problems`` (None: an idle slot)."""
    ctx = Context(FilterConfig(), n_filters=len(problems), n_cam_capacity=Nmax, dtype=dtype)
    for f, pr in enumerate(problems):
        if pr is not None:
            set_problem_state(ctx, f, pr)
    if with_map:
        ctx.map_create(cap)
    return ctx


def put(ctx, f, t):
    ctx.map_put(f, t["ids"], fr.mask_words(t["obs"]), t["z"], t["p_w"], t["init"])


def assert_table(ctx, f, t, msg=""):
    ids, mask, z, p_w, init = ctx.map_get(f)
    np.testing.assert_array_equal(ids, t["ids"], err_msg=msg)
    np.testing.assert_array_equal(mask, fr.mask_words(t["obs"]), err_msg=msg)
    np.testing.assert_array_equal(z, fr.masked_z(t), err_msg=msg)
    np.testing.assert_array_equal(p_w, t["p_w"], err_msg=msg)
    np.testing.assert_array_equal(init, t["init"], err_msg=msg)


def small_problem(N, seed, F=4):
    return synth.make_update_problem(N, F, seed=seed)


def rc_of(err):
    return int(re.search(r"rc=(-?\d+)", str(err.value)).group(1))


# ----------------------------------------------- per call vs the reference --
def check_add_lost(cap, tabs, msgs, ncams):
    """Every message pair through one launch naming filters 2 and 0, twice from the
    same put state, against the reference; the idle slot 1 stays empty."""
    ctx = make_ctx([small_problem(6, 1), None, small_problem(8, 2)], Nmax=8, cap=cap)
    try:
        for k in range(max(len(m) for m in msgs.values())):
            first = None
            for rep in range(2):                       # a repeat from the same put state: the same bits
                for f in (0, 2):
                    put(ctx, f, tabs[f])
                mk = {f: msgs[f][min(k, len(msgs[f]) - 1)] for f in (0, 2)}
                off = np.cumsum([0, len(mk[2][1]), len(mk[0][1])])
                got = ctx.map_add_lost([2, 0], off, np.concatenate([mk[2][1], mk[0][1]]),
                                       np.concatenate([mk[2][2], mk[0][2]]))
                state = [ctx.map_get(f) for f in (0, 2)]
                for w, f in enumerate((2, 0)):
                    nxt, tracked, nb, cid, info = fr.add_lost(tabs[f], mk[f][1], mk[f][2], ncams[f] - 1, cap)
                    assert got[w][0] == tracked and got[w][1] == nb, (f, mk[f][0])
                    np.testing.assert_array_equal(got[w][2], cid)
                    np.testing.assert_array_equal(got[w][3], info)
                    assert_table(ctx, f, nxt, "%d %s" % (f, mk[f][0]))
                if first is None:
                    first = (got, state)
                else:
                    for a, b in zip(first[0], got):
                        for x, y in zip(a, b):
                            np.testing.assert_array_equal(x, y)
                    for a, b in zip(first[1], state):
                        for x, y in zip(a, b):
                            np.testing.assert_array_equal(x, y)
            assert_table(ctx, 1, fr.empty(8))          # the idle slot stays empty
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256])
def test_add_lost_vs_reference(n):
    rng = np.random.default_rng(100 + n)
    ncams = [6, None, 8]
    tabs = {f: random_table(rng, n if f == 0 else max(n - 3, 0), 8, ncams[f]) for f in (0, 2)}
    msgs = {f: messages(rng, tabs[f], CAP) for f in (0, 2)}
    check_add_lost(CAP, tabs, msgs, ncams)


@pytest.mark.parametrize("cap,n", fc.BIG)
def test_add_lost_beyond_one_chunk(cap, n):
    """Tables and messages above 256 rows: the table loop of k_map_add_lost runs up
    to 8 times and the message loop up to 4 times, nnew, nkeep and ncand carried
    (tests/test_feature_map_ref.py asserts that of these inputs).  At n = 513, 1023
    and 2047 the launch's other filter has 40 rows and a one-chunk message."""
    tabs, msgs, ncams = fc.add_lost_tables(n, cap)
    name, ids, z = msgs[0][0]
    assert name == "mixed"
    fc.assert_add_lost_spans_chunks(tabs[0], ids, z, ncams[0] - 1, cap)
    check_add_lost(cap, tabs, msgs, ncams)


def check_prune(cap, ncams, tables, rng):
    """prune_select and prune_commit of filters 0 and 2 in one launch each, at the
    three slot choices, against the reference.  ``tables()`` -> {filter: table}."""
    ctx = make_ctx([small_problem(ncams, 3), None, small_problem(ncams, 4)], Nmax=8, cap=cap)
    try:
        for slots in fc.prune_slots(ncams):
            tabs = tables()
            for f in (0, 2):
                put(ctx, f, tabs[f])
            rm = fr.removed_mask(slots, 8)
            got = ctx.map_prune_select([0, 2], [0, 2, 4], slots + slots[::-1])
            ents = []
            for w, f in enumerate((0, 2)):
                tabs[f], iid, info = fr.prune_select(tabs[f], rm)
                np.testing.assert_array_equal(got[w][0], iid)
                np.testing.assert_array_equal(got[w][1], info)
                assert_table(ctx, f, tabs[f], "select %d %s" % (f, slots))
                ents.append(fc.prune_entries(rng, info))
            ctx.map_prune_commit([2, 0], [0, len(ents[1][0]), len(ents[1][0]) + len(ents[0][0])],
                                 np.concatenate([ents[1][0], ents[0][0]]), np.concatenate([ents[1][1], ents[0][1]]),
                                 np.concatenate([ents[1][2], ents[0][2]]))
            for w, f in enumerate((0, 2)):
                tabs[f] = fr.prune_commit(tabs[f], rm, *ents[w])
                assert not tabs[f]["obs"][:, ncams - 2:].any()
                assert_table(ctx, f, tabs[f], "commit %d %s" % (f, slots))
    finally:
        ctx.close()


@pytest.mark.parametrize("ncams", [4, 6, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256])
def test_prune_select_commit_vs_reference(ncams, n):
    rng = np.random.default_rng(7 * ncams + n)
    check_prune(CAP, ncams, lambda: {f: random_table(rng, n, 8, ncams, newest_free=False) for f in (0, 2)}, rng)


@pytest.mark.parametrize("cap,n", fc.BIG)
def test_prune_select_commit_beyond_one_chunk(cap, n):
    """Tables above 256 rows: k_map_prune_select's loop runs up to 8 times with ninv
    carried, k_map_prune_commit's entry loop more than once from n = 1023 on (more
    than 256 entries, rows >= 256 among them; tests/test_feature_map_ref.py asserts
    that of these inputs)."""
    rng = fc.prune_rng(n)
    check_prune(cap, 8, lambda: fc.prune_tables(n, rng), rng)


# ------------------------------------------------------- load equals load --
def problem_table(pr, Nmax, rng, drop_newest):
    """The problem's tracks as a table (map order = feature order); every
    second row initialised at its landmark."""
    t = fr.empty(Nmax)
    F = pr.F
    obs, z = np.zeros((F, Nmax), bool), np.zeros((F, Nmax, 4))
    for f in range(F):
        for r in range(pr.obs_off[f], pr.obs_off[f + 1]):
            if drop_newest and pr.obs_cam[r] == pr.N - 1:
                continue
            obs[f, pr.obs_cam[r]] = True
            z[f, pr.obs_cam[r]] = pr.obs_z[r]
    t["ids"] = weird_ids(rng, F)
    t["obs"], t["z"] = obs, z
    t["init"] = np.arange(F) % 2 == 0
    t["p_w"] = np.where(t["init"][:, None], pr.landmarks + 1e-3 * rng.standard_normal((F, 3)), 0.0)
    return t


def padded(t, rng, total, pad_obs):
    """t's rows, in their order, at random rows 256.. of a ``total``-row table on
    both sides of row 512; the other rows observe the slots ``pad_obs[i % len]``
    (rows no load names).  Returns the table and the rows of t in it."""
    F, Nmax = t["obs"].shape
    pos = np.sort(rng.choice(np.arange(256, total), F, replace=False))
    assert pos[0] < 512 <= pos[-1]
    T = dict(ids=weird_ids(rng, total), obs=np.zeros((total, Nmax), bool), z=rng.standard_normal((total, Nmax, 4)),
             p_w=rng.standard_normal((total, 3)), init=rng.random(total) < 0.5)
    for i in range(total):
        T["obs"][i, np.array(pad_obs[i % len(pad_obs)], int)] = True
    for k in ("obs", "z", "p_w", "init"):
        T[k][pos] = t[k]
    return T, pos


def batch_from(per_slot, B, with_pw):
    """msckf_batch_load arguments from per-slot reference loads {slot: load()}."""
    feat_off, obs_off, cams, zs, pws, chis = [0], [0], [], [], [], []
    for s in range(B):
        if s in per_slot:
            off, oc, oz, pw, chi = per_slot[s]
            obs_off.extend(obs_off[-1] + off[1:].astype(np.int64))
            cams.append(oc)
            zs.append(oz)
            if with_pw:
                pws.append(pw)
                chis.append(chi)
            feat_off.append(feat_off[-1] + len(off) - 1)
        else:
            feat_off.append(feat_off[-1])
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)  # noqa: E731
    return (np.array(feat_off), np.array(obs_off), cat(cams, (0,)).astype(np.int32), cat(zs, (0, 4)),
            cat(pws, (0, 3)) if with_pw else None, cat(chis, (0,)) if with_pw else None)


def assert_same_state(a, b, slots):
    for f in slots:
        for x, y in zip(a.get_state(f), b.get_state(f)):
            np.testing.assert_array_equal(x, y)


def assert_same_results(ra, rb):
    for x, y in zip(ra, rb):
        np.testing.assert_array_equal(x, y)


def check_lost_load(dtype, row_cap, cap=CAP, pad=0):
    """``pad``: the problems' rows among that many rows of a larger table, from row
    256 on, the others too short to be candidates or observed at the newest slot."""
    rng = np.random.default_rng(5)
    prs = [synth.make_update_problem(8, 30, seed=11), None, synth.make_update_problem(6, 24, seed=12)]
    dev, ref = make_ctx(prs, 10, dtype, cap=cap), make_ctx(prs, 10, dtype, with_map=False)
    try:
        loads, rows, counts, off = {}, [], [], [0]
        tabs = {f: problem_table(prs[f], 10, rng, drop_newest=True) for f in (0, 2)}
        if pad:
            for f in (0, 2):
                s = prs[f].N - 1
                tabs[f], pos = padded(tabs[f], rng, pad, [[], [s], [0, s], [1], [2, 3], list(range(s + 1)), [s - 1]])
        for f in (0, 2):
            put(dev, f, tabs[f])
        msg = {f: (rng.permutation(tabs[f]["ids"])[:5], rng.standard_normal((5, 4))) for f in (0, 2)}
        got = dev.map_add_lost([0, 2], [0, 5, 10], np.concatenate([msg[0][0], msg[2][0]]),
                               np.concatenate([msg[0][1], msg[2][1]]))
        for w, f in enumerate((0, 2)):
            _, _, _, cid, info = fr.add_lost(tabs[f], msg[f][0], msg[f][1], prs[f].N - 1, cap)
            np.testing.assert_array_equal(got[w][3], info)
            assert len(cid) >= 10 and (~info[:, 2].astype(bool)).any() and info[:, 2].any()
            if pad:                            # every loaded row beyond the first chunk, in two chunks or more
                assert info[:, 3].min() >= 256 and info[:, 3].max() >= 512 and len(cid) <= prs[f].F
            loads[f] = fr.load(tabs[f], _lib.MAP_LOAD_LOST, info[:, 3], info[:, 0])
            rows.append(info[:, 3])
            counts.append(info[:, 0])
            off.append(off[-1] + len(cid))
        dev.map_load(_lib.MAP_LOAD_LOST, [0, 2], off, np.concatenate(rows), np.concatenate(counts))
        dev.batch_update(row_cap=row_cap, triangulate=True)
        ref.batch_load(*batch_from(loads, 3, True))
        ref.batch_update(row_cap=row_cap, triangulate=True)
        ra, rb = dev.batch_results(), ref.batch_results()
        assert_same_results(ra, rb)
        assert ra[0].any() and ra[3].any() and ra[4].max() > 0
        print("rows stacked with row_cap %d: %s" % (row_cap, ra[4]))
        if row_cap == 60:                      # the cap broke the list: at most one feature's rows beyond it
            assert ra[4].max() <= 60 + 4 * 8 - 3
        else:
            assert ra[4].max() > 60 + 4 * 8 - 3
        assert_same_state(dev, ref, (0, 2))
    finally:
        dev.close()
        ref.close()


@pytest.mark.parametrize("row_cap", [1500, 60])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lost_load_equals_batch_load(dtype, row_cap):
    check_lost_load(dtype, row_cap)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lost_load_from_rows_beyond_256(dtype):
    check_lost_load(dtype, 1500, cap=1024, pad=700)


def check_prune_loads(dtype, cap=CAP, pad=0):
    """``pad``: as in check_lost_load, the other rows observing at most one of the
    removed slots."""
    rng = np.random.default_rng(6)
    prs = [synth.make_update_problem(8, 30, seed=21), None, synth.make_update_problem(7, 24, seed=22)]
    dev, ref = make_ctx(prs, 10, dtype, cap=cap), make_ctx(prs, 10, dtype, with_map=False)
    try:
        tabs = {f: problem_table(prs[f], 10, rng, drop_newest=False) for f in (0, 2)}
        if pad:
            for f in (0, 2):
                tabs[f], pos = padded(tabs[f], rng, pad, [[], [0], [4, 5], [5], [prs[f].N - 1], [0, 2, 4]])
                assert pos[0] >= 256
        slots = {0: [0, 1], 2: [0, 3]}
        for f in (0, 2):
            put(dev, f, tabs[f])
        got = dev.map_prune_select([0, 2], [0, 2, 4], slots[0] + slots[2])
        infos, rm = {}, {}
        for w, f in enumerate((0, 2)):
            rm[f] = fr.removed_mask(slots[f], 10)
            tabs[f], iid, infos[f] = fr.prune_select(tabs[f], rm[f])
            np.testing.assert_array_equal(got[w][1], infos[f])
            if pad:
                assert infos[f][:, 3].min() >= 256 and infos[f][:, 3].max() >= 512
        # triangulation form: the involved, uninitialised rows with all their observations
        tri = {f: infos[f][~infos[f][:, 2].astype(bool)] for f in (0, 2)}
        assert all(len(tri[f]) >= 1 for f in (0, 2))
        rng_t = dev.map_load(_lib.MAP_LOAD_PRUNE_TRI, [2, 0], [0, len(tri[2]), len(tri[2]) + len(tri[0])],
                             np.concatenate([tri[2][:, 3], tri[0][:, 3]]), np.concatenate([tri[2][:, 0], tri[0][:, 0]]))
        dev.batch_triangulate()
        ref.batch_load(*batch_from({f: fr.load(tabs[f], _lib.MAP_LOAD_PRUNE_TRI, tri[f][:, 3], tri[f][:, 0])
                                    for f in (0, 2)}, 3, False))
        ref.batch_triangulate()
        ra, rb = dev.batch_results(), ref.batch_results()
        np.testing.assert_array_equal(ra[2], rb[2])
        np.testing.assert_array_equal(ra[3], rb[3])
        assert ra[3].any()
        # update form: the involved observations of the rows initialised before or just now
        loads, rows, counts, pws, off, ents = {}, [], [], [], [0], {}
        for f in (0, 2):
            a, b = rng_t[f]
            p, ok = ra[2][a:b], ra[3][a:b]
            ents[f] = (tri[f][:, 3], ok, p)
            pw = np.full((len(infos[f]), 3), np.nan)
            good = infos[f][:, 2].astype(bool)
            un = np.flatnonzero(~good)
            pw[un] = np.where(ok[:, None], p, np.nan)
            good[un] = ok
            upd = np.flatnonzero(good)
            loads[f] = fr.load(tabs[f], _lib.MAP_LOAD_PRUNE_UPDATE, infos[f][upd, 3], infos[f][upd, 1], rm[f], pw[upd])
            rows.append(infos[f][upd, 3])
            counts.append(infos[f][upd, 1])
            pws.append(pw[upd])
            off.append(off[-1] + len(upd))
        dev.map_load(_lib.MAP_LOAD_PRUNE_UPDATE, [0, 2], off, np.concatenate(rows), np.concatenate(counts),
                     np.concatenate(pws))
        dev.batch_update(row_cap=0, triangulate=False)
        ref.batch_load(*batch_from(loads, 3, True))
        ref.batch_update(row_cap=0, triangulate=False)
        ra, rb = dev.batch_results(), ref.batch_results()
        assert_same_results(ra, rb)
        assert ra[0].any() and ra[3].all()
        assert_same_state(dev, ref, (0, 2))
        dev.map_prune_commit([0, 2], [0, len(ents[0][0]), len(ents[0][0]) + len(ents[2][0])],
                             np.concatenate([ents[0][0], ents[2][0]]), np.concatenate([ents[0][1], ents[2][1]]),
                             np.concatenate([ents[0][2], ents[2][2]]))
        for f in (0, 2):
            assert_table(dev, f, fr.prune_commit(tabs[f], rm[f], *ents[f]))
    finally:
        dev.close()
        ref.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prune_loads_equal_batch_load(dtype):
    check_prune_loads(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_prune_loads_from_rows_beyond_256(dtype):
    check_prune_loads(dtype, cap=1024, pad=700)


def test_second_mask_word():
    """n_cam_capacity 72, 70 cam states, tracks crossing slots 63 / 64."""
    rng = np.random.default_rng(9)
    pr = synth.make_update_problem(70, 2, seed=31)
    dev, ref = make_ctx([pr], 72), make_ctx([pr], 72, with_map=False)
    try:
        n = 40
        t = fr.empty(72)
        obs = np.zeros((n, 72), bool)
        for i in range(n):
            a = 56 + i % 8
            obs[i, a:a + 3 + i % 9] = True           # slots 56..74 clipped below: all cross 63 / 64
        obs[:, 69:] = False
        t.update(ids=weird_ids(rng, n), obs=obs, z=rng.standard_normal((n, 72, 4)) * 0.1,
                 p_w=rng.standard_normal((n, 3)), init=np.arange(n) % 3 == 0)
        put(dev, 0, t)
        ids_m = np.concatenate([t["ids"][::3], [77, -78]]).astype(np.int64)
        z_m = rng.standard_normal((len(ids_m), 4))
        got = dev.map_add_lost([0], [0, len(ids_m)], ids_m, z_m)[0]
        nxt, tracked, nb, cid, info = fr.add_lost(t, ids_m, z_m, 69, CAP)
        assert got[0] == tracked and len(cid) > 5
        np.testing.assert_array_equal(got[2], cid)
        np.testing.assert_array_equal(got[3], info)
        assert_table(dev, 0, nxt)
        rm = fr.removed_mask([63, 64], 72)
        gi = dev.map_prune_select([0], [0, 2], [64, 63])[0]
        sel, iid, sinfo = fr.prune_select(nxt, rm)
        np.testing.assert_array_equal(gi[0], iid)
        np.testing.assert_array_equal(gi[1], sinfo)
        assert len(iid) > 3
        assert_table(dev, 0, sel)
        tri = sinfo[~sinfo[:, 2].astype(bool)]
        dev.map_load(_lib.MAP_LOAD_PRUNE_TRI, [0], [0, len(tri)], tri[:, 3], tri[:, 0])
        dev.batch_triangulate()
        ref.batch_load(*batch_from({0: fr.load(sel, _lib.MAP_LOAD_PRUNE_TRI, tri[:, 3], tri[:, 0])}, 1, False))
        ref.batch_triangulate()
        ra, rb = dev.batch_results(), ref.batch_results()
        np.testing.assert_array_equal(ra[2], rb[2])
        np.testing.assert_array_equal(ra[3], rb[3])
        dev.map_prune_commit([0], [0, len(tri)], tri[:, 3], ra[3], ra[2])
        assert_table(dev, 0, fr.prune_commit(sel, rm, tri[:, 3], ra[3], ra[2]))
    finally:
        dev.close()
        ref.close()


# --------------------------------------------------------------- end to end --
def late_start(st, k0):
    a = int(st.frame_off[k0])
    return FeatureStream(st.imu, st.frame_t[k0:], st.frame_off[k0:] - a, st.feat_id[a:], st.feat_z[a:], st.gt)


_STREAMS, _BIG_STREAM = [], []


def streams():
    if not _STREAMS:
        g = golden("sequence_s1")
        _STREAMS.extend([FeatureStream.from_synthetic(synth.make_sequence(int(g["n_frames"]), int(g["seed"]))),
                         FeatureStream.from_synthetic(synth.make_sequence(90, 7)),
                         late_start(FeatureStream.from_synthetic(synth.make_sequence(140, 11)), 7)])
    return _STREAMS


def single(st, dtype, **kw):
    flt = msckf_amd.MSCKF(dtype=dtype, **kw)
    try:
        traj = replay(flt, st)
        return traj, flt.gate_log, flt.gamma_log, flt.shape_log, flt.state_cov()
    finally:
        flt.close()


def assert_same_run(a, b):
    np.testing.assert_array_equal(a[0].t, b[0].t)
    np.testing.assert_array_equal(a[0].p, b[0].p)
    assert a[1] == b[1] and len(a[1]) > 100
    assert a[2] == b[2]
    assert a[3] == b[3]
    np.testing.assert_array_equal(a[4], b[4])


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_map_equals_host_map(dtype, which):
    st = streams()[which]
    assert_same_run(single(st, dtype, device_map=True), single(st, dtype))


def big_stream():
    """400 features in every frame: the map passes 256 rows (tests/test_feature_map_ref.py
    asserts it on the stand-in), so every map kernel loops at the default map_capacity."""
    if not _BIG_STREAM:
        _BIG_STREAM.append(FeatureStream.from_synthetic(synth.make_sequence(30, 3, max_features=400, n_landmarks=2000)))
    return _BIG_STREAM[0]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_map_equals_host_map_above_256_rows(dtype):
    st = big_stream()
    assert np.diff(st.frame_off).min() > 256
    assert_same_run(single(st, dtype, device_map=True), single(st, dtype))


def test_multi_device_map_equals_host_map_mixed_sizes():
    """A 400-feature lane next to a 150-feature lane: the two workgroups of one
    launch loop a different number of times."""
    sts = [big_stream(), streams()[1]]
    out = []
    for kw in ({"device_map": True}, {}):
        ms = MultiMSCKF(2, **kw)
        try:
            trajs = ms.run_streams(sts, arrays=bool(kw))
            out.append([(trajs[i], ln.gate_log, ln.gamma_log, ln.shape_log, ln.state_cov())
                        for i, ln in enumerate(ms.lanes)])
        finally:
            ms.close()
    for a, b in zip(*out):
        assert_same_run(a, b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_multi_device_map_equals_host_map(dtype):
    sts = streams()
    out = []
    for kw in ({"device_map": True}, {}):
        ms = MultiMSCKF(3, dtype=dtype, **kw)
        try:
            trajs = ms.run_streams(sts, arrays=bool(kw))
            out.append(([(trajs[i], ln.gate_log, ln.gamma_log, ln.shape_log, ln.state_cov())
                         for i, ln in enumerate(ms.lanes)], dict(ms.launches)))
        finally:
            ms.close()
    for a, b in zip(out[0][0], out[1][0]):
        assert_same_run(a, b)
    la, n_rounds = out[0][1], max(s.n_frames for s in sts)
    # one batched call per new request kind per round (the update: one per form)
    assert 0 < la["map_add_lost"] <= n_rounds
    assert 0 < la["map_prune_select"] <= n_rounds and la["map_prune_commit"] == la["map_prune_select"]
    assert la["map_triangulate"] <= la["map_prune_select"] and la["map_update"] <= 2 * n_rounds
    assert "update" not in la and "triangulate" not in la
    assert not any(k.startswith("map_") for k in out[1][1])


def test_forced_online_reset():
    g = golden("sequence_s3")
    st = FeatureStream.from_synthetic(synth.make_sequence(int(g["n_frames"]), int(g["seed"])))
    runs = []
    for kw in ({"device_map": True}, {}):
        cfg = FilterConfig()
        cfg.position_std_threshold = float(g["position_std_threshold"])
        flt = msckf_amd.MSCKF(cfg, **kw)
        seen = []

        def on_result(res, flt=flt, seen=seen):
            if len(flt.reset_log) > len(seen):
                seen.append(len(flt.map_server))
        try:
            traj = replay(flt, st, on_result=on_result)
            runs.append((traj.p, list(flt.reset_log), list(flt.gate_log), seen, flt.state_cov()))
        finally:
            flt.close()
    a, b = runs
    assert a[1] == b[1] and len(a[1]) >= 1
    assert a[3] == b[3] == [0] * len(a[1])         # the map is empty after each reset
    np.testing.assert_array_equal(a[0], b[0])
    assert a[2] == b[2]
    np.testing.assert_array_equal(a[4], b[4])


# ------------------------------------------------------------------- errors --
def test_errors_leave_the_tables():
    rng = np.random.default_rng(3)
    ctx = make_ctx([small_problem(6, 1), None, small_problem(6, 2)], Nmax=8)
    bare = make_ctx([small_problem(6, 1)], Nmax=8, with_map=False)
    roomy = make_ctx([small_problem(6, 1), small_problem(6, 2)], Nmax=8, cap=1024)
    try:
        tabs = {0: random_table(rng, 250, 8, 6), 2: random_table(rng, 20, 8, 6)}
        for f in (0, 2):
            put(ctx, f, tabs[f])

        def unchanged():
            for f in (0, 2):
                assert_table(ctx, f, tabs[f])
        z7 = rng.standard_normal((7, 4))
        new7 = (1 << 45) + np.arange(7, dtype=np.int64)
        # slot 2 has a lost table from a good call, and its descriptor loads
        nxt2, _, _, cid2, info2 = fr.add_lost(tabs[2], np.zeros(0, np.int64), np.zeros((0, 4)), 5, CAP)
        got2 = ctx.map_add_lost([2], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4)))[0]
        np.testing.assert_array_equal(got2[3], info2)
        assert len(cid2) > 0
        tabs[2] = nxt2
        ctx.map_load(_lib.MAP_LOAD_LOST, [2], [0, len(info2)], info2[:, 3], info2[:, 0])
        with pytest.raises(MsckfError) as e:        # 250 + 7 = 257 rows; slot 2's good message changes nothing either
            ctx.map_add_lost([2, 0], [0, 3, 10], np.concatenate([new7[:3], new7]), np.concatenate([z7[:3], z7]))
        assert rc_of(e) == -3
        unchanged()
        with pytest.raises(MsckfError) as e:        # the failed call wrote over slot 2's lost table: its old
            ctx.map_load(_lib.MAP_LOAD_LOST, [2], [0, len(info2)], info2[:, 3], info2[:, 0])   # descriptor is refused
        assert rc_of(e) == -1
        unchanged()
        with pytest.raises(MsckfError) as e:        # a repeated id
            ctx.map_add_lost([0], [0, 3], np.array([5, 6, 5], np.int64), z7[:3])
        assert rc_of(e) == -1
        unchanged()
        for call in (lambda: ctx.map_add_lost([3], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4))),
                     lambda: ctx.map_add_lost([-1], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4))),
                     lambda: ctx.map_add_lost([0, 0], [0, 0, 0], np.zeros(0, np.int64), np.zeros((0, 4))),
                     lambda: ctx.map_prune_select([0], [0, 1], [6]),           # no such cam slot
                     lambda: ctx.map_prune_select([0], [0, 2], [1, 1]),
                     lambda: ctx.map_load(_lib.MAP_LOAD_LOST, [0], [0, 1], [0], [3]),   # no add_lost before it
                     lambda: ctx.map_prune_commit([0], [0, 0], [], [], np.zeros((0, 3))),  # no open select
                     lambda: ctx.map_put(7, *[tabs[2][k] if k != "obs" else fr.mask_words(tabs[2]["obs"])
                                              for k in ("ids", "obs", "z", "p_w", "init")]),
                     lambda: ctx.map_get(5),
                     lambda: bare.map_add_lost([0], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4))),
                     lambda: bare.map_clear([0])):
            with pytest.raises(MsckfError) as e:
                call()
            assert rc_of(e) == -1
        with pytest.raises(MsckfError) as e:
            bare.map_get(0)
        assert rc_of(e) == -1
        with pytest.raises(MsckfError) as e:        # a table of 257 rows
            big = random_table(rng, 257, 8, 6)
            put(ctx, 2, big)
        assert rc_of(e) == -3
        unchanged()
        # a good call still works afterwards, and clear empties one slot only
        got = ctx.map_add_lost([0], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4)))[0]
        nxt = fr.add_lost(tabs[0], np.zeros(0, np.int64), np.zeros((0, 4)), 5, CAP)
        np.testing.assert_array_equal(got[3], nxt[4])
        assert_table(ctx, 0, nxt[0])
        ctx.map_clear([0])
        assert_table(ctx, 0, fr.empty(8))
        assert_table(ctx, 2, tabs[2])
        # overflow beyond one pass: 700 rows + 325 new ids = cap + 1, the new ids in every chunk of a 625-row message
        t, ids, z = fc.overflow_case(1024)
        small = random_table(rng, 20, 8, 6)
        put(roomy, 0, t)
        put(roomy, 1, small)
        with pytest.raises(MsckfError) as e:
            roomy.map_add_lost([1, 0], [0, 0, len(ids)], ids, z)
        assert rc_of(e) == -3
        assert_table(roomy, 0, t)
        assert_table(roomy, 1, small)
        got = roomy.map_add_lost([0], [0, len(ids) - 1], ids[:-1], z[:-1])[0]      # one id fewer fills the map exactly
        nxt = fr.add_lost(t, ids[:-1], z[:-1], 5, 1024)
        assert got[0] == nxt[1] == 300 and got[1] == 700
        np.testing.assert_array_equal(got[2], nxt[3])
        np.testing.assert_array_equal(got[3], nxt[4])
        assert_table(roomy, 0, nxt[0])
        assert_table(roomy, 1, small)
    finally:
        ctx.close()
        bare.close()
        roomy.close()


def test_dof_above_99_is_refused():
    pr = synth.make_update_problem(102, 2, seed=41)
    ctx = make_ctx([pr], Nmax=104)
    try:
        t = fr.empty(104)
        obs = np.zeros((2, 104), bool)
        obs[0, :101] = True            # M = 101: dof 100 in the lost form
        obs[1, 3:50] = True
        t.update(ids=np.array([4, 9], np.int64), obs=obs, z=np.zeros((2, 104, 4)), p_w=np.zeros((2, 3)),
                 init=np.zeros(2, bool))
        put(ctx, 0, t)
        got = ctx.map_add_lost([0], [0, 0], np.zeros(0, np.int64), np.zeros((0, 4)))[0]
        np.testing.assert_array_equal(got[3][:, 0], [101, 47])
        assert_table(ctx, 0, fr.empty(104))
        with pytest.raises(MsckfError) as e:
            ctx.map_load(_lib.MAP_LOAD_LOST, [0], [0, 2], got[3][:, 3], got[3][:, 0])
        assert rc_of(e) == -1 and "degrees of freedom" in str(e.value)
        with pytest.raises(fr.MapError):
            fr.load(t, _lib.MAP_LOAD_LOST, got[3][:, 3], got[3][:, 0])
        assert_table(ctx, 0, fr.empty(104))
        ctx.map_load(_lib.MAP_LOAD_LOST, [0], [0, 1], got[3][1:, 3], got[3][1:, 0])   # the other row alone loads
    finally:
        ctx.close()


def test_repeats_give_the_same_bits():
    """put -> add_lost -> lost load + update -> prune_select -> tri load +
    triangulate -> commit, twice from the same put state and filter state."""
    rng = np.random.default_rng(8)
    pr = synth.make_update_problem(8, 30, seed=51)
    tab = problem_table(pr, 10, rng, drop_newest=True)
    msg_ids, msg_z = rng.permutation(tab["ids"])[:12], rng.standard_normal((12, 4))
    ctx = make_ctx([None, pr], 10)
    runs = []
    try:
        for rep in range(2):
            set_problem_state(ctx, 1, pr)
            put(ctx, 1, tab)
            out = list(ctx.map_add_lost([1], [0, 12], msg_ids, msg_z)[0])
            info = out[3]
            ctx.map_load(_lib.MAP_LOAD_LOST, [1], [0, len(info)], info[:, 3], info[:, 0])
            ctx.batch_update(row_cap=1500, triangulate=True)
            out.extend(ctx.batch_results())
            sel = ctx.map_prune_select([1], [0, 2], [0, 1])[0]
            out.extend(sel)
            tri = sel[1][~sel[1][:, 2].astype(bool)]
            ctx.map_load(_lib.MAP_LOAD_PRUNE_TRI, [1], [0, len(tri)], tri[:, 3], tri[:, 0])
            ctx.batch_triangulate()
            res = ctx.batch_results()
            out.extend(res[2:4])
            ctx.map_prune_commit([1], [0, len(tri)], tri[:, 3], res[3], res[2])
            out.extend(ctx.map_get(1))
            out.extend(ctx.get_state(1))
            runs.append(out)
        assert len(runs[0][2]) > 5 and len(runs[0]) == len(runs[1])
        for x, y in zip(*runs):
            np.testing.assert_array_equal(x, y)
    finally:
        ctx.close()
