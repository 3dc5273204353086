"""icl_pairs_between / icl_pairs_between_dev (imageclust_amd/csrc/pairs.hip): every pair (query row, library row) whose exact
WardDistance is at most a threshold, as a CSR list over the queries, with no distance matrix and no cap on a query's partners.  Bar:
row_ptr and col equal the checker's (tests/pairs_between_cases.py: the oracle's values thresholded in plain numpy, the excluded column
left out, pairs in (i, j) order) and val equals it as uint32 bit patterns -- no tolerance anywhere -- for every band and tile edge, both
load paths, every split count, the dense and the empty result, sizes on both sides, NaN / Inf rows, exclude and the capacity convention."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pairs_between_cases as BC

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)
SHAPES = [(1, 1, 1), (2, 3, 3), (5, 7, 5), (130, 3, 5), (3, 130, 8), (129, 300, 33), (257, 260, 64)]
SPLIT_SHAPE = (64, 700, 16)


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(nq, n, d, kind, rich):
    """One input, computed once and never modified: (Q, L, q_size, l_size, exclude, V).  Every third query is an exact copy of a library
    row (few_copies: both sides draw from the same patterns).  rich: mixed sizes on both sides, one NaN row, a +Inf and a -Inf entry, and
    every other planted query -- a query that is a library row -- excludes the row it came from."""
    seed = 1000 * nq + n
    if kind == "copies":
        patterns = max(100, (max(nq, n) + 2) // 3 + 20)
        Q, L, plant = BC.few_copies(nq, d, seed, patterns=patterns), BC.few_copies(n, d, seed, patterns=patterns), {}
    else:
        Q, L, plant = BC.planted(nq, n, d, seed, kind)
    qs = ls = ex = None
    if rich:
        qs, ls = BC.mixed_sizes(nq, seed + 5), BC.mixed_sizes(n, seed + 6)
        ex = np.full(nq, -1, np.int64)
        for i in list(plant)[::2]:
            ex[i] = plant[i]
        if n >= 3:
            L[n - 1, d - 1] = np.nan
            L[n // 2, 0] = -np.inf
        if nq >= 2:
            Q[nq - 1, 0] = np.inf
    V = BC.oracle_values(Q, L, qs, ls)
    return frozen(Q, L, qs, ls, ex, V)


def mid_threshold(V):
    """between the zero pairs (the planted copies, the ties) and every other value, read from the oracle's values; 1 where V has no other"""
    V = np.asarray(V, np.float32)
    zero = V == 0
    other = V[~zero]
    other = other[~np.isnan(other)]
    return BC.between(V, zero) if zero.any() and len(other) else np.float32(1.0)


def dev_form(ctx, Q, L, thr, **kw):
    """ctx.pairs_between_dev on device copies of Q and L"""
    bufs = [ctx.malloc(max(a.nbytes, 16)) for a in (Q, L)]
    try:
        for p, a in zip(bufs, (Q, L)):
            if a.size:
                ctx.h2d(p, a)
        return ctx.pairs_between_dev(bufs[0], len(Q), bufs[1], len(L), Q.shape[1], thr, **kw)
    finally:
        for p in bufs:
            ctx.free(p)


def check(ctx, P, thr, forms=("host", "dev"), **kw):
    Q, L, qs, ls, ex, V = P
    want = BC.select(V, thr, ex)
    for form in forms:
        if form == "host":
            got = ctx.pairs_between(Q, L, thr, q_size=qs, l_size=ls, exclude=ex, **kw)
        else:
            got = dev_form(ctx, Q, L, thr, q_size=qs, l_size=ls, exclude=ex, **kw)
        assert BC.same(got, want), "%s form, threshold %r: %s" % (form, thr, BC.why(got, want))
    return want


@pytest.mark.parametrize("nq,n,d", SHAPES)
def test_every_shape_input_and_threshold(ctx, nq, n, d):
    kinds = ["random", "ties"] + (["copies"] if d >= 8 else [])   # (100 distinct integer patterns need some room)
    for kind in kinds:
        for rich in (False, True):
            P = problem(nq, n, d, kind, rich)
            V, ex = P[5], P[4]
            rp, col, val = check(ctx, P, np.float32(-0.0))
            if kind != "copies" and not rich:
                assert rp[-1] >= (nq + 2) // 3 and (val == 0).all()                          # the planted copies are found
            check(ctx, P, mid_threshold(V))
            rp, col, val = check(ctx, P, INF)                                                # every tile flagged, every row full
            assert rp[-1] == (~np.isnan(V)).sum() - (0 if ex is None else (~np.isnan(V[np.flatnonzero(ex >= 0), ex[ex >= 0]])).sum())
            st = ctx.last_pairs_between_stats()
            assert st["hit_tiles"] == (st["tiles"] if rp[-1] else 0) or rich
            rp, col, val = check(ctx, P, np.float32(-1.0))                                   # nothing listed: no fill launch
            assert rp[-1] == 0 and not rp.any() and len(col) == 0
            st = ctx.last_pairs_between_stats()
            assert st["hit_tiles"] == 0 and st["pairs"] == nq * n
    if nq >= 129 and n >= 260:
        Q, L, qs, ls, ex, V = problem(nq, n, d, "random", True)
        assert np.isnan(V[:, n - 1]).all() and np.isinf(V[nq - 1, :n - 1]).all() and np.isinf(V[:nq - 1, n // 2]).all()
        rp, col, val = BC.select(V, INF, ex)
        assert n - 1 not in col and np.isinf(val).sum() >= nq + n - 3    # the NaN row pairs with nobody, the Inf rows only under +Inf


def raw_call(ctx, P, thr, cap, pad=16, sentinel=77, dev=False, with_buffers=True):
    """The entry point itself, with col / val of cap + pad entries filled with a sentinel -> (code, row_ptr, col, val, total)"""
    Q, L, qs, ls, ex, V = P
    nq, n, d = len(Q), len(L), Q.shape[1]
    p = lambda a: None if a is None else a.ctypes.data
    rp, tot = np.full(nq + 1, sentinel, np.int64), ctypes.c_int64(-5)
    col, val = np.full(cap + pad, sentinel, np.int32), np.full(cap + pad, float(sentinel), np.float32)
    if not dev:
        rc = ctx.L.icl_pairs_between(ctx.h, p(Q), p(qs), nq, p(L), p(ls), n, d, float(thr), p(ex), p(rp), p(col) if with_buffers else None,
                                     p(val) if with_buffers else None, cap, ctypes.byref(tot))
        return rc, rp, col, val, tot.value
    bufs = [ctx.malloc(max(a.nbytes, 16)) for a in (Q, L, col, val)]
    try:
        for b, a in zip(bufs, (Q, L, col, val)):
            if a.size:
                ctx.h2d(b, a)
        rc = ctx.L.icl_pairs_between_dev(ctx.h, bufs[0], p(qs), nq, bufs[1], p(ls), n, d, float(thr), p(ex), p(rp), bufs[2] if with_buffers else None,
                                         bufs[3] if with_buffers else None, cap, ctypes.byref(tot))
        ctx.sync()
        ctx.d2h(col, bufs[2])
        ctx.d2h(val, bufs[3])
        return rc, rp, col, val, tot.value
    finally:
        for b in bufs:
            ctx.free(b)


def test_every_split_count_gives_the_same_bits(ctx):
    from imageclust_amd import _lib

    nq, n, d = SPLIT_SHAPE
    assert (n + 127) // 128 == 6
    try:
        for kind, rich in (("ties", True), ("random", False)):
            P = problem(nq, n, d, kind, rich)
            for thr in (INF, mid_threshold(P[5])):
                wr, wc, wv = BC.select(P[5], thr, P[4])
                total = int(wr[-1])
                assert total > 0
                for forced, used in ((1, 1), (2, 2), (3, 3), (7, 6), (0, 6)):   # 7 is held to the 6 tiles; auto: one band, room for every tile
                    ctx.set_nearest_options(forced)
                    for dev in (False, True):
                        rc, rp, col, val, tot = raw_call(ctx, P, thr, total, dev=dev)
                        assert rc == _lib.ICL_OK and tot == total and ctx.last_pairs_between_stats()["splits"] == used
                        got = (rp, col[:total], val[:total])
                        assert BC.same(got, (wr, wc, wv)), "%d splits, dev=%s: %s" % (forced, dev, BC.why(got, (wr, wc, wv)))
                        assert (col[total:] == 77).all() and (val[total:] == 77.0).all()   # nothing beyond *total is written
    finally:
        ctx.set_nearest_options(0)


def test_self_join_with_exclude_mirrors_pairs_within(ctx):
    nq, n, d = SPLIT_SHAPE
    E = BC.tie_rows(n, d, 31, distinct=40)
    E.setflags(write=False)
    sizes = BC.mixed_sizes(n, 32)
    for sz in (None, sizes):
        for thr in (np.float32(0.0), np.float32(6.0)):
            rp, col, val = ctx.pairs_between(E, E, thr, q_size=sz, l_size=sz, exclude=np.arange(n))
            wr, wc, wv = ctx.pairs_within(E, thr, size=sz)
            assert wr[-1] > n
            lower = {(i, int(wc[p])): wv[p].view(np.uint32) for i in range(n) for p in range(int(wr[i]), int(wr[i + 1]))}
            got = {(i, int(col[p])): val[p].view(np.uint32) for i in range(n) for p in range(int(rp[i]), int(rp[i + 1]))}
            assert len(got) == rp[-1] == 2 * len(lower)                     # row i lists its j < i and its j > i, never itself
            assert got == {**lower, **{(j, i): v for (i, j), v in lower.items()}}
            assert all((np.diff(col[rp[i]:rp[i + 1]]) > 0).all() for i in range(n))


def test_agrees_with_nearest_where_k_holds_every_partner_and_goes_beyond_it(ctx):
    nq, n, d = SPLIT_SHAPE
    Q, L = BC.few_copies(nq, d, 41, patterns=250), BC.few_copies(n, d, 41, patterns=250)   # the same patterns on both sides, each at most 3 times
    V = BC.oracle_values(Q, L)
    thr = np.float32(np.sort(V, axis=1)[:, 40].min())        # every query has fewer than 64 partners under it (asserted below)
    for t in (np.float32(0.0), thr):
        rp, col, val = ctx.pairs_between(Q, L, t)
        assert 0 < np.diff(rp).max() <= 64 and rp[-1] > nq // 2
        idx, nv = ctx.nearest(Q, L, 64)
        for i in range(nq):
            with np.errstate(invalid="ignore"):
                keep = (idx[i] >= 0) & (nv[i] <= t)
            order = np.argsort(idx[i][keep])                  # nearest lists by (value, j), the join by j
            assert np.array_equal(idx[i][keep][order], col[rp[i]:rp[i + 1]])
            assert np.array_equal(nv[i][keep][order].view(np.uint32), val[rp[i]:rp[i + 1]].view(np.uint32))
    # a stock photo held 70 times: the k = 64 route drops six partners, the join lists all 70
    L2 = L.copy()
    at = np.random.default_rng(42).permutation(n)[:70]
    L2[at] = Q[5]
    base = int((V[5] == 0).sum())
    rp, col, val = ctx.pairs_between(Q, L2, 0.0)
    mine = col[rp[5]:rp[6]]
    assert set(at) <= set(mine.tolist()) and 70 <= len(mine) <= 70 + base and (val[rp[5]:rp[6]] == 0).all() and (np.diff(mine) > 0).all()
    idx, nv = ctx.nearest(Q, L2, 64)
    assert ((idx[5] >= 0) & (nv[5] <= 0)).sum() == 64 < len(mine)
    want = BC.expected(Q, L2, 0.0)
    assert BC.same((rp, col, val), want), BC.why((rp, col, val), want)


def test_stats_and_the_other_reports_left_alone(ctx):
    P = problem(257, 260, 64, "random", True)
    Q, L, qs, ls, ex, V = P
    ctx.nearest(Q, L, 3)
    ctx.pairs_within(L, 1.0)
    others = (ctx.last_nearest_stats(), ctx.last_pairs_stats(), ctx.last_fit_stats())
    try:
        for forced in (0, 2):
            ctx.set_nearest_options(forced)
            for thr in (mid_threshold(V), INF, np.float32(-1.0)):
                check(ctx, P, thr, forms=("host",))
                st, (tiles, hit, pairs) = ctx.last_pairs_between_stats(), BC.tile_stats(V, thr, ex)
                assert (st["tiles"], st["hit_tiles"], st["pairs"]) == (tiles, hit, pairs) and tiles == 9
                assert st["splits"] == (2 if forced else 3) and 0 < st["workspace_bytes"] < 64 * (257 + 260)   # O(nq splits + bands tiles), no nq x n array
        rc, rp, col, val, tot = raw_call(ctx, P, INF, 0, with_buffers=False)   # the size query alone: the fill pass did not run
        assert ctx.last_pairs_between_stats()["pairs"] == BC.tile_stats(V, INF, ex, filled=False)[2] == 257 * 260
    finally:
        ctx.set_nearest_options(0)
    assert others == (ctx.last_nearest_stats(), ctx.last_pairs_stats(), ctx.last_fit_stats())


def test_capacity_convention(ctx):
    from imageclust_amd import _lib

    P = problem(129, 300, 33, "ties", True)
    wr, wc, wv = BC.select(P[5], 0.0, P[4])
    total = int(wr[-1])
    assert total > 300
    for dev in (False, True):
        rc, rp, col, val, tot = raw_call(ctx, P, 0.0, total - 1, pad=0, dev=dev)       # one short: an error, with row_ptr and total complete
        assert rc == _lib.ICL_ERR_ARG and tot == total and np.array_equal(rp, wr) and b"do not fit" in ctx.L.icl_last_error(ctx.h)
        assert (col == 77).all() and (val == 77.0).all()
        rc, rp, col, val, tot = raw_call(ctx, P, 0.0, 0, dev=dev, with_buffers=False)  # the size query
        assert rc == _lib.ICL_OK and tot == total and np.array_equal(rp, wr)
        rc, rp, col, val, tot = raw_call(ctx, P, 0.0, total, pad=0, dev=dev)           # a buffer of exactly *total
        assert rc == _lib.ICL_OK and tot == total and BC.same((rp, col, val), (wr, wc, wv))
    for hint in (1, total, total + 100):                                               # the wrapper's hint: too small, exact, generous
        check(ctx, P, 0.0, cap=hint)


def test_empty_sides(ctx):
    d = 8
    Q, L = BC.random_rows(5, d, 1), BC.random_rows(0, d, 2)
    for a, b in ((Q, L), (L, Q), (L, L)):
        for got in (ctx.pairs_between(a, b, INF), dev_form(ctx, a, b, INF)):
            rp, col, val = got
            assert rp.tolist() == [0] * (len(a) + 1) and len(col) == 0 and len(val) == 0
        assert ctx.last_pairs_between_stats() == {"splits": 0, "tiles": 0, "hit_tiles": 0, "pairs": 0, "workspace_bytes": 0}


def test_bad_arguments_write_nothing(ctx):
    from imageclust_amd import _lib

    nq, n, d = 4, 5, 4
    Q, L = np.zeros((nq, d), np.float32), np.zeros((n, d), np.float32)
    ok_q, ok_l, ok_ex = np.ones(nq, np.int32), np.ones(n, np.int32), np.array([-1, 0, 4, -1], np.int64)
    bad_q, bad_l, hi, lo = ok_q.copy(), ok_l.copy(), ok_ex.copy(), ok_ex.copy()
    bad_q[2], bad_l[4], hi[1], lo[0] = 0, -3, n, -2
    rp, col, val, tot = np.full(nq + 1, 77, np.int64), np.full(32, 77, np.int32), np.full(32, 77.0, np.float32), ctypes.c_int64(-5)
    p = lambda a: None if a is None else a.ctypes.data
    dbuf, filler = ctx.malloc(1024), np.full(1024, 0x4D, np.uint8)
    try:
        ctx.h2d(dbuf, filler)  # the device form's col (dbuf + 512) and val (dbuf + 768) are read back below

        def host(h=ctx.h, Q=Q, qs=ok_q, nq=nq, L=L, ls=ok_l, n=n, d=d, thr=1.0, ex=ok_ex, rp=rp, col=col, val=val, cap=32, tot=tot):
            return ctx.L.icl_pairs_between(h, p(Q), p(qs), nq, p(L), p(ls), n, d, thr, p(ex), p(rp), p(col), p(val), cap,
                                           None if tot is None else ctypes.byref(tot))

        def dev(h=ctx.h, Q=dbuf, qs=ok_q, nq=nq, L=dbuf + 256, ls=ok_l, n=n, d=d, thr=1.0, ex=ok_ex, rp=rp, col=dbuf + 512, val=dbuf + 768, cap=32,
                tot=tot):
            return ctx.L.icl_pairs_between_dev(h, Q, p(qs), nq, L, p(ls), n, d, thr, p(ex), p(rp), col, val, cap, None if tot is None else ctypes.byref(tot))

        cases = dict(null_ctx=dict(h=None), null_Q=dict(Q=None), null_L=dict(L=None), null_row_ptr=dict(rp=None), null_total=dict(tot=None),
                     null_col=dict(col=None), null_val=dict(val=None), null_both_with_cap=dict(col=None, val=None, cap=1), d0=dict(d=0),
                     neg_nq=dict(nq=-1, qs=None, ex=None), neg_n=dict(n=-1, ls=None), huge_n=dict(n=1 << 31, ls=None), q_size_0=dict(qs=bad_q),
                     l_size_neg=dict(ls=bad_l), exclude_n=dict(ex=hi), exclude_below=dict(ex=lo), neg_cap=dict(cap=-1),
                     nan_threshold=dict(thr=float("nan")))
        for fn in (host, dev):
            for name, kw in cases.items():
                assert fn(**kw) == _lib.ICL_ERR_ARG, (fn.__name__, name)
                assert (rp == 77).all() and (col == 77).all() and (val == 77.0).all() and tot.value == -5, (fn.__name__, name)
        # 2^24 bands of queries x 1024 forced splits are 2^34 workgroups: more than one launch's grid, refused before anything is read
        ctx.set_nearest_options(1024)
        for fn in (host, dev):
            assert fn(nq=1 << 31, qs=None, ex=None, n=1024 * 128, ls=None) == _lib.ICL_ERR_ARG and b"grid" in ctx.L.icl_last_error(ctx.h)
            assert (rp == 77).all() and tot.value == -5
        ctx.set_nearest_options(0)
        back = np.zeros(1024, np.uint8)
        ctx.sync()
        ctx.d2h(back, dbuf)
        assert (back == 0x4D).all()           # nothing reached the device buffers either
        assert host() == _lib.ICL_OK and tot.value == 18 and rp.tolist() == [0, 5, 9, 13, 18]
        assert col[5:9].tolist() == [1, 2, 3, 4] and (col[18:] == 77).all() and (val[:18] == 0).all()
    finally:
        ctx.set_nearest_options(0)
        ctx.free(dbuf)
    with pytest.raises(_lib.ICLError) as ei:
        ctx.pairs_between(Q, L, float("nan"))
    assert ei.value.code == _lib.ICL_ERR_ARG and "NaN" in str(ei.value)


def test_clustering_duplicates_through_a_real_context(ctx):
    from imageclust_amd import clustering as CL
    from tests import pairs_cases as PC

    d = 24
    held = BC.random_rows(200, d, 71)
    batch = BC.random_rows(100, d, 72)
    batch[0::7] = held[3:3 + 15]                       # re-uploads of held images
    batch[50] = batch[1]                               # a copy inside the batch
    batch[51] = batch[1] + np.float32(1e-3)            # ... and a near copy of it
    batch[60] = held[3]                                # a second re-upload of the image batch[0] re-uploads
    hid, bid = ["h%d" % i for i in range(200)], ["n%d" % i for i in range(100)]
    thr = np.float32(0.01)

    def states():
        real = CL.Clustering(3, 6, ctx=ctx)
        stand = CL.Clustering(3, 6, between_engine=lambda Q, L, t: BC.expected(Q, L, t), pairs_engine=lambda E, t: PC.expected(E, t))
        for st in (real, stand):
            st.add(held, hid)
        return real, stand

    real, stand = states()
    got, want = real.duplicates_of(batch, bid, thr), stand.duplicates_of(batch, bid, thr)
    assert [[(k, np.float32(v).view(np.uint32)) for k, v in row] for row in got] == [[(k, np.float32(v).view(np.uint32)) for k, v in row] for row in want]
    assert sum(1 for row in want if row) == 15 + 3 and want[60] == [("h3", 0.0), ("n0", 0.0)] and [k for k, _ in want[51]] == ["n1", "n50"]
    assert CL.DuplicatesOf(batch, bid, held, hid, thr, ctx=ctx) == CL.DuplicatesOf(batch, bid, held, hid, thr, engine=lambda Q, L, t: BC.expected(Q, L, t))
    sr, ss = real.add(batch, bid, skip_duplicates=thr), stand.add(batch, bid, skip_duplicates=thr)
    assert sr == ss and len(sr) == 18 and ("n60", "h3", 0.0) in sr and ("n51", "n1") == sr[[s for s, _, _ in sr].index("n51")][:2]
    assert list(real.embeddings) == list(stand.embeddings) and len(real.clusters) == 200 + 100 - 18
