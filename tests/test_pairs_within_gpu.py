"""icl_pairs_within / icl_pairs_within_dev (imageclust_amd/csrc/pairs.hip): every pair of rows whose exact WardDistance is at most a
threshold, as a CSR list over the strict lower triangle, with no distance matrix and no cap on a row's partners.  Bar: row_ptr and col
equal the checker's (tests/pairs_cases.py: the oracle's matrix thresholded in plain numpy, pairs in (i, j) order) and val equals it as
uint32 bit patterns, for every tile edge, both load paths, a second band of tile rows, ties at the threshold, the dense and the empty
result, sizes, NaN / Inf rows and the capacity convention; and a tile row of more than 256 tiles against a CSR that follows from a sort."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pairs_cases as PC

pytestmark = pytest.mark.gpu

INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def ties300():
    """tie_rows(300, 36, 21, distinct=7) and the oracle's matrix of them, computed once for the tests that share them (never modified)"""
    E = PC.tie_rows(300, 36, 21, distinct=7)
    V = PC.oracle_matrix(E)
    E.setflags(write=False)
    V.setflags(write=False)
    return E, V


def median_of(V):
    low = PC.lower_values(V)
    low = low[~np.isnan(low)]
    return np.float32(np.median(low)) if len(low) else np.float32(0)


def check(ctx, E, thr, sizes=None, V=None, **kw):
    """ctx.pairs_within against the checker; V: the oracle's matrix when the caller already holds it"""
    V = PC.oracle_matrix(E, sizes) if V is None else V
    got, want = ctx.pairs_within(E, thr, size=sizes, **kw), PC.select(V, thr)
    assert PC.same(got, want), "threshold %r: %s" % (thr, PC.why(got, want))
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 127, 128, 129, 257, 300])
def test_tile_edges(ctx, n):
    E = PC.random_rows(n, 36, 100 + n)
    V = PC.oracle_matrix(E)
    rp, col, _ = check(ctx, E, median_of(V), V=V)
    assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(col) and (len(col) > 0) == (n >= 2)
    assert ctx.last_pairs_stats()["tiles"] == (0 if n < 2 else PC.tile_stats(V, median_of(V))[0])


@pytest.mark.parametrize("d", [1, 3, 4, 1001, 2048])
def test_both_load_paths_and_a_long_chain(ctx, d):
    E = PC.random_rows(129, d, 300 + d)
    V = PC.oracle_matrix(E)
    check(ctx, E, median_of(V), V=V)


def test_band_order_second_band_and_its_cap(ctx):
    E = PC.random_rows(1300, 8, 5)  # 11 tile rows: a whole band of 8, then a band of 3 with its triangular cap
    V = PC.oracle_matrix(E)
    low = np.sort(PC.lower_values(V))
    check(ctx, E, low[len(low) // 50], V=V)  # 2 % of the pairs: hits in every tile, rows with dozens of partners across all of their tiles
    st, (tiles, hit, pairs) = ctx.last_pairs_stats(), PC.tile_stats(V, low[len(low) // 50])
    assert tiles == 11 * 12 // 2 and hit > 60 and (st["tiles"], st["hit_tiles"], st["pairs"]) == (tiles, hit, pairs)
    check(ctx, E, low[40], V=V)              # 41 pairs: most tiles are skipped by the fill pass
    st, (tiles, hit, pairs) = ctx.last_pairs_stats(), PC.tile_stats(V, low[40])
    assert 0 < hit <= 41 and (st["tiles"], st["hit_tiles"], st["pairs"]) == (tiles, hit, pairs)
    assert 0 < st["workspace_bytes"] < 64 * 1300  # O(n + tiles), no n x n array


def line_rows(n, quiet_tile_row=100, seed=257):
    """n rows (x_i, 0, 0, 0) whose expected pairs at threshold 0.5 follow from a sort: x is a permutation of the multiples of 4 below 4 n,
    then a few dozen rows are overwritten with another row's x plus 1.  All values are integers below 2^24, so a pair with |x_i - x_j| <= 1
    has the value 0 or 0.5 exactly (the sum is 0 or 1, the sizes' factor 1 * 1 / (1 + 1)) and every other pair is at least 0.5 * 3^2 = 4.5.
    The last row's partners lie in tile columns 0, 255, 256 and -- where the last tile row has a row below it -- in its diagonal tile; no
    row of tile row `quiet_tile_row` is a copy or is copied.  -> (E float32[n][4], (row_ptr, col, val) expected, hit tiles expected)"""
    rng = np.random.default_rng(seed)
    x = 4 * rng.permutation(n).astype(np.int64)
    last, first_of_last = n - 1, (n - 1) // 128 * 128
    copies = [(5, last), (255 * 128 + 77, last), (256 * 128 + 3, last)]  # (the row overwritten, the row whose x it takes)
    if first_of_last < last:
        copies.append((first_of_last, last))
    taken = {r for pair in copies for r in pair}
    free = [r for r in rng.permutation(n).tolist() if r // 128 != quiet_tile_row and r not in taken][:80]
    copies += list(zip(free[:40], free[40:]))
    for dst, src in copies:
        x[dst] = x[src] + 1
    assert 0 <= x.min() and x.max() < 1 << 24
    # rows whose x share x // 4 are each other's partners (x is 0 or 1 mod 4), and nobody else's
    key = x // 4
    order = np.argsort(key, kind="stable")
    ks, start, count = np.unique(key[order], return_index=True, return_counts=True)
    pairs = []
    for s, c in zip(start[count > 1], count[count > 1]):
        rows = np.sort(order[s:s + c])
        pairs += [(int(i), int(j)) for a, i in enumerate(rows) for j in rows[:a]]
    pairs.sort()
    pi, pj = np.array(pairs, np.int64).T
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(pi, minlength=n), out=row_ptr[1:])
    val = (np.float32(0.5) * ((x[pi] - x[pj]) ** 2).astype(np.float32)).astype(np.float32)
    assert set(np.unique(val).tolist()) == {0.0, 0.5}
    E = np.zeros((n, 4), np.float32)
    E[:, 0] = x
    return E, (row_ptr, pj.astype(np.int32), val), len(set(zip((pi // 128).tolist(), (pj // 128).tolist())))


@pytest.mark.parametrize("n", [257 * 128 + 1, 257 * 128 + 64])
def test_a_tile_row_longer_than_256_tiles(ctx, n):
    """The fill walk reads a band's flags 256 at a time: tile row 257 (258 tiles) crosses that boundary.  n = 257 * 128 + 1 leaves one
    row in the last tile row, whose diagonal tile then holds no pair j < i at all; the second n gives that tile 64 rows and a pair."""
    E, want, hit_tiles = line_rows(n)
    rp, col, _ = want
    tile_cols = set((col[rp[n - 1]:rp[n]] // 128).tolist())   # of the last row's partners
    assert tile_cols == ({0, 255, 256, 257} if n > 257 * 128 + 1 else {0, 255, 256}) and (n - 1) // 128 == 257
    assert rp[101 * 128] == rp[100 * 128] and rp[-1] == 40 + len(tile_cols) * (len(tile_cols) + 1) // 2 and hit_tiles > 40   # (an ordinary tile row without a pair)
    buf = ctx.malloc(E.nbytes)
    try:
        ctx.h2d(buf, E)
        for size in (None, np.ones(n, np.int32)):             # the two sources of sizes must give the same bits
            got = ctx.pairs_within_dev(buf, n, 4, 0.5, size=size, cap=int(rp[-1]))
            assert PC.same(got, want), "size %s: %s" % ("None" if size is None else "ones", PC.why(got, want))
            st = ctx.last_pairs_stats()
            assert st["tiles"] == 258 * 259 // 2 and st["hit_tiles"] == hit_tiles
    finally:
        ctx.free(buf)


def test_exact_ties_at_the_threshold(ctx):
    E, V = ties300()
    low = PC.lower_values(V)
    assert (low == 0).sum() > 5000            # 7 patterns over 300 rows: duplicates inside tiles, across tiles and on diagonal tiles
    rp, col, val = check(ctx, E, 0.0, V=V)
    assert rp[-1] == (low == 0).sum() and (val == 0).all()
    for i in (5, 130, 299):                   # exactly the earlier rows with the same pattern
        assert col[rp[i]:rp[i + 1]].tolist() == [j for j in range(i) if (E[j] == E[i]).all()]
    neg = check(ctx, E, np.float32(-0.0), V=V)
    assert PC.same(neg, (rp, col, val))
    t = np.unique(low)[2]                     # a value that occurs, many times
    assert t > 0 and (low == t).sum() > 100
    at = check(ctx, E, t, V=V)
    below = check(ctx, E, np.nextafter(t, np.float32(0)), V=V)
    assert at[0][-1] - below[0][-1] == (low == t).sum() and (below[2] < t).all() and (at[2] == t).sum() == (low == t).sum()


@pytest.mark.parametrize("thr", [INF, PC.MAXF])
def test_dense_every_pair_and_every_tile(ctx, thr):
    E, V = ties300()
    rp, col, _ = check(ctx, E, thr, V=V)
    assert rp[-1] == 44850 and np.array_equal(rp, np.arange(301, dtype=np.int64) * (np.arange(301) - 1) // 2)
    st = ctx.last_pairs_stats()
    assert st["tiles"] == 6 and st["hit_tiles"] == st["tiles"] and st["pairs"] == 2 * 44850


def test_empty_result(ctx):
    E, V = ties300()
    rp, col, val = check(ctx, E, -1.0, V=V)
    assert rp[-1] == 0 and not rp.any() and len(col) == 0 and len(val) == 0
    st = ctx.last_pairs_stats()
    assert st["tiles"] == 6 and st["hit_tiles"] == 0 and st["pairs"] == 44850
    check(ctx, E, -INF, V=V)


def test_mixed_sizes(ctx):
    E = PC.random_rows(300, 36, 31)
    E[200] = E[7]
    sizes = PC.mixed_sizes(300, 32)
    V = PC.oracle_matrix(E, sizes)
    assert not np.array_equal(V, PC.oracle_matrix(E))
    check(ctx, E, median_of(V), sizes=sizes, V=V)
    rp, col, val = check(ctx, E, 0.0, sizes=sizes, V=V)
    assert rp[-1] == 1 and col.tolist() == [7]
    Et, _ = ties300()
    check(ctx, Et, 40.0, sizes=sizes)


def test_nan_row_and_inf_row(ctx):
    E = PC.random_rows(300, 36, 41)
    E[140, 3] = np.nan
    E[260, 35] = np.inf
    V = PC.oracle_matrix(E)
    low = PC.lower_values(V)
    assert np.isnan(V[140, :140]).all() and np.isinf(V[260, :140]).all() and np.isnan(V[260, 140])
    for thr in (INF, PC.MAXF, median_of(V), 0.0):
        rp, col, val = check(ctx, E, thr, V=V)
        assert not np.isnan(val).any()
        assert rp[141] == rp[140] and 140 not in col                    # the NaN row pairs with nobody
        assert (np.isinf(val).sum() == 298) if thr == INF else not np.isinf(val).any()  # the Inf row: only under +Inf, and not with the NaN row
    assert (~np.isnan(low)).sum() == 44850 - 299


def test_capacity_convention(ctx):
    from imageclust_amd import _lib

    E, V = ties300()
    wr, wc, wv = PC.select(V, 0.0)
    total = int(wr[-1])
    p = lambda a: None if a is None else a.ctypes.data

    def call(cap, with_buffers=True):
        rp, tot = np.full(301, 77, np.int64), ctypes.c_int64(-5)
        col, val = np.full(total + 8, 77, np.int32), np.full(total + 8, 77.0, np.float32)
        rc = ctx.L.icl_pairs_within(ctx.h, p(E), None, 300, 36, 0.0, p(rp), p(col) if with_buffers else None, p(val) if with_buffers else None,
                                    cap, ctypes.byref(tot))
        return rc, rp, col, val, tot.value

    rc, rp, col, val, tot = call(0, with_buffers=False)                  # the size query
    assert rc == _lib.ICL_OK and tot == total and np.array_equal(rp, wr)
    rc, rp, col, val, tot = call(total - 1)                              # one short: an error, with row_ptr and total complete
    assert rc == _lib.ICL_ERR_ARG and tot == total and np.array_equal(rp, wr) and b"do not fit" in ctx.L.icl_last_error(ctx.h)
    rc, rp, col, val, tot = call(0)                                      # buffers of no capacity at all
    assert rc == _lib.ICL_ERR_ARG and tot == total and np.array_equal(rp, wr) and (col == 77).all()
    rc, rp, col, val, tot = call(total)                                  # exactly enough
    assert rc == _lib.ICL_OK and tot == total and PC.same((rp, col[:total], val[:total]), (wr, wc, wv))
    assert (col[total:] == 77).all() and (val[total:] == 77.0).all()
    for hint in (1, total, total + 100):                                 # the wrapper's hint: too small, exact, generous
        assert PC.same(ctx.pairs_within(E, 0.0, cap=hint), (wr, wc, wv))


def test_device_buffers_and_the_scalar_load_path(ctx):
    E, V = ties300()
    t = np.unique(PC.lower_values(V))[2]
    want = PC.select(V, t)
    buf = ctx.malloc(E.nbytes + 16)
    try:
        for off in (0, 4):                    # 16-byte aligned rows take the wide loads; one float further on nothing is aligned
            ctx.h2d(buf + off, E)
            got = ctx.pairs_within_dev(buf + off, 300, 36, t)
            assert PC.same(got, want), "offset %d: %s" % (off, PC.why(got, want))
            got = ctx.pairs_within_dev(buf + off, 300, 36, t, size=np.ones(300, np.int32), cap=7)
            assert PC.same(got, want), "offset %d, sizes of 1: %s" % (off, PC.why(got, want))
    finally:
        ctx.free(buf)
    assert PC.same(ctx.pairs_within(E, t), want)


def test_equals_from_matrix_over_the_distance_matrix(ctx):
    from imageclust_amd import _lib

    E = PC.random_rows(300, 36, 51)
    sizes = PC.mixed_sizes(300, 52)
    for sz in (None, sizes):
        D = ctx.ward_distance_matrix(E, sz)
        for thr in (median_of(D), np.float32(np.sort(PC.lower_values(D))[100])):
            got, want = ctx.pairs_within(E, thr, size=sz), _lib.pairs_within_from_matrix(D, thr)
            assert PC.same(got, want), PC.why(got, want)


def test_agrees_with_near_duplicates_where_that_route_is_complete(ctx):
    from imageclust_amd import clustering as CL

    E = PC.few_copies(300, 36, 61)            # 100 distinct integer patterns, each used at most three times
    V = PC.oracle_matrix(E)
    partners = ((V == 0).sum(1) - 1)          # (the diagonal is 0 too)
    assert partners.max() == 2 and (np.diag(V) == 0).all()
    ids = ["img_%d" % i for i in range(300)]
    got = CL.DuplicatePairs(E, ids, 0.0, ctx=ctx)
    assert got == CL.NearDuplicates(E, ids, 8, 0.0, ctx=ctx) and len(got) == partners.sum() // 2 == 300
    groups = CL.DuplicateGroups(E, ids, 0.0, ctx=ctx)
    firsts = [int(g[0][4:]) for g in groups]
    assert len(groups) == 100 and all(len(g) == 3 for g in groups) and firsts == sorted(firsts)
    # ... and where it is not: 7 patterns over 300 rows give every image dozens of partners, more than k can hold
    Et, Vt = ties300()
    allp = CL.DuplicatePairs(Et, ids, 0.0, ctx=ctx)
    assert len(allp) == (PC.lower_values(Vt) == 0).sum() > len(CL.NearDuplicates(Et, ids, 8, 0.0, ctx=ctx))
    assert len(CL.DuplicateGroups(Et, ids, 0.0, ctx=ctx)) == 7


def test_bad_arguments_write_nothing(ctx):
    from imageclust_amd import _lib

    n, d = 5, 4
    E = np.zeros((n, d), np.float32)
    ok_s = np.ones(n, np.int32)
    bad0, badn = ok_s.copy(), ok_s.copy()
    bad0[2], badn[4] = 0, -3
    rp, col, val, tot = np.full(n + 1, 77, np.int64), np.full(32, 77, np.int32), np.full(32, 77.0, np.float32), ctypes.c_int64(-5)
    p = lambda a: None if a is None else a.ctypes.data
    dbuf, filler = ctx.malloc(1024), np.full(1024, 0x4D, np.uint8)
    try:
        ctx.h2d(dbuf, filler)  # the device form's col (dbuf + 256) and val (dbuf + 512) are read back below

        def host(h=ctx.h, E=E, sz=ok_s, n=n, d=d, thr=1.0, rp=rp, col=col, val=val, cap=32, tot=tot):
            return ctx.L.icl_pairs_within(h, p(E), p(sz), n, d, thr, p(rp), p(col), p(val), cap, None if tot is None else ctypes.byref(tot))

        def dev(h=ctx.h, E=dbuf, sz=ok_s, n=n, d=d, thr=1.0, rp=rp, col=dbuf + 256, val=dbuf + 512, cap=32, tot=tot):
            return ctx.L.icl_pairs_within_dev(h, E, p(sz), n, d, thr, p(rp), col, val, cap, None if tot is None else ctypes.byref(tot))

        cases = dict(null_ctx=dict(h=None), null_E=dict(E=None), null_row_ptr=dict(rp=None), null_total=dict(tot=None), null_col=dict(col=None),
                     null_val=dict(val=None), null_both_with_cap=dict(col=None, val=None, cap=1), d0=dict(d=0), neg_n=dict(n=-1),
                     huge_n=dict(n=1 << 31, sz=None), grid_too_large=dict(n=10_000_000, sz=None), size_0=dict(sz=bad0), size_neg=dict(sz=badn), neg_cap=dict(cap=-1),
                     nan_threshold=dict(thr=float("nan")))
        for fn in (host, dev):
            for name, kw in cases.items():
                assert fn(**kw) == _lib.ICL_ERR_ARG, (fn.__name__, name)
                assert (rp == 77).all() and (col == 77).all() and (val == 77.0).all() and tot.value == -5, (fn.__name__, name)
        back = np.zeros(1024, np.uint8)
        ctx.sync()
        ctx.d2h(back, dbuf)
        assert (back == 0x4D).all()           # nothing reached the device buffers either
        # 78 125 tile rows are 3.05e9 tiles: more than one launch's grid (tri_tile_count), refused before anything is allocated or read
        assert host(n=10_000_000, sz=None) == _lib.ICL_ERR_ARG and b"tile grid" in ctx.L.icl_last_error(ctx.h) and tot.value == -5
        assert host() == _lib.ICL_OK and tot.value == 10 and rp.tolist() == [0, 0, 1, 3, 6, 10]
        assert col[:10].tolist() == [0, 0, 1, 0, 1, 2, 0, 1, 2, 3] and (col[10:] == 77).all() and (val[:10] == 0).all()
        for m in (0, 1):                      # n <= 1: ICL_OK and no pairs, with or without E
            rp[:], tot.value = 77, -5
            assert host(E=None, sz=None, n=m) == _lib.ICL_OK and tot.value == 0 and (rp[:m + 1] == 0).all() and (rp[m + 1:] == 77).all()
            assert ctx.last_pairs_stats() == {"tiles": 0, "hit_tiles": 0, "pairs": 0, "workspace_bytes": 0}
    finally:
        ctx.free(dbuf)
    with pytest.raises(_lib.ICLError) as ei:
        ctx.pairs_within(E, float("nan"))
    assert ei.value.code == _lib.ICL_ERR_ARG and "NaN" in str(ei.value)
