"""Inputs of tests/test_gpu_feature_map.py, kept apart from it so that the
conditions on them are checked without a device (tests/test_feature_map_ref.py).

The map kernels (csrc/msckf_map.hip) walk a table and a message in chunks of
256 rows and carry running counts from chunk to chunk; ``BIG`` holds the
(cap, n) pairs above one chunk, ``big_messages`` the messages above one, and
``add_lost_chunks`` / ``prune_chunks`` state, from the numpy reference's own
outputs, what each chunk of an input holds."""
import numpy as np

import feature_map_ref as fr

CHUNK = 256            # MAP_BLOCK of csrc/msckf_map.hip
NMAX_BIG = 8           # a 2048-row z table is 0.5 MB per filter per table set
# (cap, n): the chunk edges of a 1024-row map, the largest map the ABI allows and a mid value
BIG = [(1024, 257), (1024, 511), (1024, 512), (1024, 513), (1024, 1023), (1024, 1024),
       (2048, 1300), (2048, 2047), (2048, 2048)]
# the second named filter's row count: fewer than 64 rows next to a table above 512 (another
# trip count in the same launch), else a few rows fewer as in the one-chunk test
SECOND_N = {257: 254, 511: 508, 512: 509, 513: 40, 1023: 40, 1024: 1021, 1300: 1297, 2047: 40, 2048: 2045}
MIN_ROWS = 64          # a chunk with fewer table rows is not asked to hold every kind of row


def weird_ids(rng, n):
    """Distinct ids: non-monotone, negative, above 2**32."""
    pool = np.concatenate([rng.choice(np.arange(-5000, 5000), n, replace=False),
                           (1 << 32) + rng.choice(np.arange(1, 100000), n, replace=False) * 7,
                           -(1 << 40) - np.arange(n)]).astype(np.int64)
    return rng.permutation(pool)[:n]


def random_table(rng, n, Nmax, ncams, newest_free=True, full=0.0, init=0.5):
    """n rows over ``ncams`` cam slots: track lengths 0 (empty mask), 1, 2, 3 and
    the whole window occur; ``newest_free``: no observation at the newest slot.
    ``full``: that fraction of the rows from the 11th on spans the whole window
    (the tables above 256 rows need more than 256 involved rows per prune);
    ``init``: the fraction of initialised rows."""
    t = fr.empty(Nmax)
    hi = ncams - 1 if newest_free else ncams
    obs = np.zeros((n, Nmax), bool)
    for i in range(n):
        M = [0, 1, 2, 3, hi][i % 5] if i < 10 else int(rng.integers(0, hi + 1))
        if full and i >= 10 and rng.random() < full:
            M = hi
        M = min(M, hi)
        a = int(rng.integers(0, hi - M + 1))
        obs[i, a:a + M] = True
        if i % 7 == 3 and M >= 2:          # a gap: observations need not be contiguous
            obs[i, a + 1] = False
    t["ids"] = weird_ids(rng, n)
    t["obs"] = obs
    t["z"] = rng.standard_normal((n, Nmax, 4))
    t["p_w"] = rng.standard_normal((n, 3))
    t["init"] = rng.random(n) < init
    return t


def messages(rng, t, cap):
    """(name, ids, z): empty, all new, all tracked, mixed -- as far as cap allows."""
    n = len(t["ids"])
    fresh = (1 << 50) + rng.permutation(400)[:min(40, cap - n)].astype(np.int64)
    some = rng.permutation(t["ids"])[:min(n, 90)]
    out = [("empty", np.zeros(0, np.int64))]
    if len(fresh):
        out.append(("new", fresh))
    if len(some):
        out.append(("tracked", some))
    if len(some) and len(fresh):
        out.append(("mixed", rng.permutation(np.concatenate([some[::2], fresh[::2]]))))
    return [(name, ids, rng.standard_normal((len(ids), 4))) for name, ids in out]


def big_messages(rng, t, cap):
    """(name, ids, z) for a table above 256 rows: a shuffled mix of up to 400
    tracked and up to 400 new ids (528 rows at the least where the map has room
    for 400 new rows), more than 256 new ids alone (where there is room) and more
    than 256 tracked ids alone."""
    n = len(t["ids"])
    fresh = (1 << 50) + rng.permutation(1000)[:min(400, cap - n)].astype(np.int64)
    some = rng.permutation(t["ids"])[:min(n // 2, 400)]
    out = [("mixed", rng.permutation(np.concatenate([some, fresh])))]
    if len(fresh) > CHUNK:
        out.append(("new", fresh[:300]))
    out.append(("tracked", rng.permutation(t["ids"])[:min(n, 300)]))
    return [(name, ids, rng.standard_normal((len(ids), 4))) for name, ids in out]


def add_lost_tables(n, cap):
    """The tables and messages of test_add_lost_beyond_one_chunk: {filter: table},
    {filter: messages}, the cam counts per slot."""
    rng = np.random.default_rng(1000 + n)
    ncams = [6, None, 8]
    tabs = {0: random_table(rng, n, NMAX_BIG, ncams[0]), 2: random_table(rng, SECOND_N[n], NMAX_BIG, ncams[2])}
    msgs = {0: big_messages(rng, tabs[0], cap),
            2: big_messages(rng, tabs[2], cap) if SECOND_N[n] > CHUNK else messages(rng, tabs[2], cap)[1:]}
    return tabs, msgs, ncams


def prune_tables(n, rng):
    """The two tables of one slot choice of test_prune_select_commit_beyond_one_chunk."""
    return {0: random_table(rng, n, NMAX_BIG, 8, newest_free=False, full=0.5, init=0.25),
            2: random_table(rng, SECOND_N[n], NMAX_BIG, 8, newest_free=False, full=0.5, init=0.25)}


def prune_slots(ncams):
    return [0, 1], [0, ncams // 2], [ncams - 3, ncams - 2]


def prune_rng(n):
    return np.random.default_rng(5000 + n)


def prune_entries(rng, info):
    """prune_commit's entries of one filter: the involved, uninitialised rows."""
    rows = info[~info[:, 2].astype(bool), 3]
    return rows, rng.random(len(rows)) < 0.6, rng.standard_normal((len(rows), 3))


def chunks(n):
    return [(a, min(a + CHUNK, n)) for a in range(0, n, CHUNK)]


def add_lost_chunks(t, ids, z, s, cap):
    """What k_map_add_lost meets per 256-row chunk, from the reference's outputs.
    Returns a dict: ``table`` [(table rows, kept, dropped, candidates, nkeep and
    ncand at the chunk's start)] over the chunks of the n + nnew rows it walks,
    ``message`` [(new ids, tracked ids matching a table row >= 256)] over the
    chunks of the message, ``desc_rows`` the descriptor's rows."""
    nxt, tracked, n, cid, info = fr.add_lost(t, ids, z, s, cap)
    ids = np.asarray(ids, np.int64)
    row_of = {int(v): i for i, v in enumerate(t["ids"])}
    mrow = np.array([row_of.get(int(v), -1) for v in ids], int)
    ntot = n + int((mrow < 0).sum())
    kept = np.ones(ntot, bool)
    kept[:n] = t["obs"][:, s]
    kept[mrow[mrow >= 0]] = True
    cand = np.zeros(ntot, bool)
    cand[info[:, 3]] = True
    assert kept.sum() == len(nxt["ids"]) and not (kept & cand).any()
    tab = [(max(min(b, n) - a, 0), int(kept[a:b].sum()), int((~kept[a:b]).sum()), int(cand[a:b].sum()),
            int(kept[:a].sum()), int(cand[:a].sum())) for a, b in chunks(ntot)]
    msg = [(int((mrow[a:b] < 0).sum()), int((mrow[a:b] >= CHUNK).sum())) for a, b in chunks(len(ids))]
    return dict(table=tab, message=msg, desc_rows=info[:, 3].copy())


def assert_add_lost_spans_chunks(t, ids, z, s, cap):
    """The mixed message of a table above 256 rows: every chunk of the walk with
    at least MIN_ROWS table rows keeps a row, drops a row and has a candidate; the
    running nkeep and ncand are carried (non-zero, and not the chunk's start
    index) into every later chunk; with MIN_ROWS rows beyond the first chunk, the
    descriptor names rows >= 256 and tracked ids match rows >= 256.  With room
    for 400 new rows, every chunk of the message holds a new id (nnew is carried)
    and the message is 513 rows or more."""
    n = len(t["ids"])
    c = add_lost_chunks(t, ids, z, s, cap)
    assert len(c["table"]) >= 2, "one chunk only"
    for k, (rows, kept, dropped, cand, nkeep0, ncand0) in enumerate(c["table"]):
        if rows >= MIN_ROWS:
            assert kept > 0 and dropped > 0 and cand > 0, (n, k, c["table"][k])
        if k:
            assert 0 < nkeep0 != k * CHUNK and 0 < ncand0 != k * CHUNK, (n, k, c["table"][k])
    if n - CHUNK >= MIN_ROWS:
        assert (c["desc_rows"] >= CHUNK).any() and sum(m[1] for m in c["message"]) > 0
    if cap - n >= 400:
        assert len(ids) >= 513 and len(c["message"]) >= 3 and all(m[0] > 0 for m in c["message"]), c["message"]
    return c


def prune_chunks(t, rm):
    """Per chunk of the table: (involved rows, rows with one observation dropped,
    involved uninitialised rows), and the descriptor's rows."""
    _, _, info = fr.prune_select(t, rm)
    k = (t["obs"] & rm).sum(axis=1)
    inv = k >= 2
    return [(int(inv[a:b].sum()), int((k[a:b] == 1).sum()), int((inv & ~t["init"])[a:b].sum()))
            for a, b in chunks(len(t["ids"]))], info[:, 3].copy()


def assert_prune_spans_chunks(t, rm):
    """Involved rows in every chunk with at least MIN_ROWS rows; with MIN_ROWS
    rows beyond the first chunk, a dropped single observation in a chunk after
    the first and descriptor rows >= 256.  Returns the
    number of prune_commit's entries and of those with a row >= 256."""
    n = len(t["ids"])
    per, rows = prune_chunks(t, rm)
    assert len(per) >= 2, "one chunk only"
    for k, (a, b) in enumerate(chunks(n)):
        if b - a >= MIN_ROWS:
            assert per[k][0] > 0, (n, k, per)
    if n - CHUNK >= MIN_ROWS:
        assert sum(p[1] for p in per[1:]) > 0 and (rows >= CHUNK).any(), (n, per)
    return sum(p[2] for p in per), sum(p[2] for p in per[1:])


def overflow_case(cap):
    """(table, ids, z): 700 rows and a shuffled message of 300 tracked ids and
    cap + 1 - 700 new ones, its last id new: n + nnew == cap + 1, and without
    the last id the map is filled exactly."""
    rng = np.random.default_rng(77)
    t = random_table(rng, 700, NMAX_BIG, 6)
    fresh = (1 << 50) + rng.permutation(1000)[:cap + 1 - 700].astype(np.int64)
    ids = rng.permutation(np.concatenate([rng.permutation(t["ids"])[:300], fresh[:-1]]))
    ids = np.concatenate([ids, fresh[-1:]])
    return t, ids, rng.standard_normal((len(ids), 4))


def prune_conditions(n):
    """The inputs of test_prune_select_commit_beyond_one_chunk in its own order of
    draws: per slot choice (entries of filter 0, those with a row >= 256)."""
    rng = prune_rng(n)
    out = []
    for slots in prune_slots(8):
        tabs = prune_tables(n, rng)
        rm = fr.removed_mask(slots, NMAX_BIG)
        out.append(assert_prune_spans_chunks(tabs[0], rm))
        for f in (0, 2):
            prune_entries(rng, fr.prune_select(tabs[f], rm)[2])
    return out
