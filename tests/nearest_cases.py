"""Inputs and the checker of the icl_nearest tests (tests/test_nearest_cpu.py, tests/test_nearest_gpu.py).

The checker takes every pair's value from the oracle's ComputeInitialDistanceMatrix over the rows of Q and E stacked with their sizes
(the block [0:nq, nq:]), applies the leave-out rules and orders each row with a STABLE sort by value over ascending j -- NaN last, as
numpy sorts -- in plain numpy: a second statement of the order rule, independent of imageclust_amd/csrc/nearest_select.h."""
import numpy as np

MAXF = np.float32(3.4028234663852886e38)


def oracle_values(Q, E, q_size=None, e_size=None):
    """-> float32[nq][n]: WardDistance of (Q[i], q_size[i]) and (E[j], e_size[j]) by the oracle"""
    from oracle import oracle as O

    Q, E = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(E, np.float32)
    nq, n = len(Q), len(E)
    if nq == 0 or n == 0:
        return np.zeros((nq, n), np.float32)
    sizes = None
    if q_size is not None or e_size is not None:
        sizes = np.concatenate([np.ones(nq, np.int32) if q_size is None else np.asarray(q_size, np.int32),
                                np.ones(n, np.int32) if e_size is None else np.asarray(e_size, np.int32)])
    return O.initial_distance_matrix(np.concatenate([Q, E]), sizes)[:nq, nq:].copy()


def select(V, k, q_size=None, e_size=None, max_size=0, exclude=None):
    """The k smallest remaining pairs of each row of V (nq x n) -> (idx int32[nq][k], val float32[nq][k])"""
    V = np.asarray(V, np.float32)
    nq, n = V.shape
    idx, val = np.full((nq, k), -1, np.int32), np.full((nq, k), MAXF, np.float32)
    for i in range(nq):
        keep = np.ones(n, bool)
        if exclude is not None and exclude[i] >= 0:
            keep[int(exclude[i])] = False
        if max_size > 0:
            sq = 1 if q_size is None else int(q_size[i])
            keep &= (sq + (np.ones(n, np.int64) if e_size is None else np.asarray(e_size, np.int64))) <= max_size
        js = np.flatnonzero(keep)
        js = js[np.argsort(V[i, js], kind="stable")][:k]
        idx[i, :len(js)] = js
        val[i, :len(js)] = V[i, js]
    return idx, val


def expected(Q, E, k, q_size=None, e_size=None, max_size=0, exclude=None):
    return select(oracle_values(Q, E, q_size, e_size), k, q_size, e_size, max_size, exclude)


def same(got, want):
    """idx equal; val equal as uint32 bit patterns, NaN compared by isnan"""
    (gi, gv), (wi, wv) = got, want
    gv, wv = np.ascontiguousarray(gv, np.float32), np.ascontiguousarray(wv, np.float32)
    if gi.shape != wi.shape or not np.array_equal(gi, wi):
        return False
    gn, wn = np.isnan(gv), np.isnan(wv)
    return bool(np.array_equal(gn, wn) and np.array_equal(gv.view(np.uint32)[~gn], wv.view(np.uint32)[~wn]))


def why(got, want):
    (gi, gv), (wi, wv) = got, want
    bad = np.argwhere((gi != wi) | ((gv.view(np.uint32) != wv.view(np.uint32)) & ~(np.isnan(gv) & np.isnan(wv))))
    if not len(bad):
        return "equal"
    i, p = bad[0]
    return "%d entries differ; first at row %d place %d: got (%d, %r), want (%d, %r)" % (len(bad), i, p, gi[i, p], gv[i, p], wi[i, p], wv[i, p])


def random_rows(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def tie_rows(n, d, seed, distinct=7):
    """integer-valued rows drawn from `distinct` patterns: many duplicate rows, so exact ties (and zeros) wherever they fall -- inside a
    tile, across tiles, across column splits.  Sums of small integers are exact in fp32: equal patterns give equal values."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, (distinct, d)).astype(np.float32)
    return base[rng.integers(0, distinct, n)]


def mixed_sizes(n, seed, lo=1, hi=9):
    return np.random.default_rng(seed).integers(lo, hi + 1, n).astype(np.int32)
