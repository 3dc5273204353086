"""Inputs and the checker of the icl_pairs_within tests (tests/test_pairs_within_cpu.py, tests/test_pairs_within_gpu.py).

The checker takes every pair's value from the oracle's ComputeInitialDistanceMatrix (oracle.initial_distance_matrix(E, sizes)),
thresholds its strict lower triangle in plain numpy (`<=` on float32: NaN fails, -0 equals +0) and lists the pairs in (i, j) order as a
CSR: a second statement of the rule, independent of imageclust_amd/csrc/pairs_select.h.  col and row_ptr must be equal, val must be
equal as uint32 bit patterns."""
import numpy as np

from tests.nearest_cases import MAXF, mixed_sizes, random_rows, tie_rows  # noqa: F401  (the shared inputs, re-exported)


def oracle_matrix(E, sizes=None):
    """-> float32[n][n]: the oracle's ComputeInitialDistanceMatrix of the rows with their sizes"""
    from oracle import oracle as O

    E = np.ascontiguousarray(E, np.float32)
    if len(E) == 0:
        return np.zeros((0, 0), np.float32)
    return np.asarray(O.initial_distance_matrix(E, None if sizes is None else np.asarray(sizes, np.int32)), np.float32)


def lower_values(V):
    """the strict lower triangle's values in (i, j) order"""
    i, j = np.tril_indices(len(V), -1)
    return np.asarray(V, np.float32)[i, j]


def select(V, threshold):
    """The pairs j < i of V (n x n) with V[i, j] <= threshold -> (row_ptr int64[n + 1], col int32[total], val float32[total])"""
    V = np.asarray(V, np.float32)
    n = len(V)
    i, j = np.tril_indices(n, -1)  # row by row, ascending j inside a row
    with np.errstate(invalid="ignore"):
        keep = V[i, j] <= np.float32(threshold)
    i, j = i[keep], j[keep]
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=n)[:n], out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), V[i, j].astype(np.float32)


def expected(E, threshold, sizes=None):
    return select(oracle_matrix(E, sizes), threshold)


def same(got, want):
    (gr, gc, gv), (wr, wc, wv) = got, want
    gv, wv = np.ascontiguousarray(gv, np.float32), np.ascontiguousarray(wv, np.float32)
    return bool(np.array_equal(np.asarray(gr, np.int64), wr) and gc.shape == wc.shape and np.array_equal(gc, wc)
                and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)))


def why(got, want):
    (gr, gc, gv), (wr, wc, wv) = got, want
    if not np.array_equal(np.asarray(gr, np.int64), wr):
        bad = np.flatnonzero(np.asarray(gr, np.int64) != wr) if len(gr) == len(wr) else [-1]
        return "row_ptr differs (got total %d, want %d); first at %d" % (gr[-1], wr[-1], bad[0])
    bad = np.flatnonzero((gc != wc) | (np.ascontiguousarray(gv, np.float32).view(np.uint32) != wv.view(np.uint32)))
    if not len(bad):
        return "equal"
    p = bad[0]
    return "%d entries differ; first at place %d (row %d): got (%d, %r), want (%d, %r)" % (
        len(bad), p, np.searchsorted(wr, p, side="right") - 1, gc[p], gv[p], wc[p], wv[p])


def tile_stats(V, threshold, tile=128):
    """What icl_last_pairs_stats must report for the matrix V: (tiles of the lower triangle, tiles that hold a listed pair, pairs j < i < n
    evaluated: the whole triangle once and the pairs of the tiles with a hit a second time when anything is listed)"""
    V = np.asarray(V, np.float32)
    n = len(V)
    T = (n + tile - 1) // tile
    with np.errstate(invalid="ignore"):
        H = np.tril(V <= np.float32(threshold), -1)
    hit = again = 0
    for ti in range(T):
        for tj in range(ti + 1):
            if H[ti * tile:(ti + 1) * tile, tj * tile:(tj + 1) * tile].any():
                nr, nc = min(tile, n - ti * tile), min(tile, n - tj * tile)
                hit += 1
                again += nr * (nr - 1) // 2 if ti == tj else nr * nc
    return T * (T + 1) // 2, hit, n * (n - 1) // 2 + again


def few_copies(n, d, seed, patterns=100, most=3):
    """n integer-valued rows drawn from `patterns` distinct patterns, each used at most `most` times, in shuffled order: every row has at
    most most - 1 exact duplicates, so a k-nearest self-join with k > most - 1 loses none of them"""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, (patterns, d)).astype(np.float32)
    assert n <= patterns * most and len(np.unique(base, axis=0)) == patterns
    use = np.repeat(np.arange(patterns), most)
    return base[rng.permutation(use)[:n]]
