"""Inputs and the checker of the icl_pairs_between tests (tests/test_pairs_between_cpu.py, tests/test_pairs_between_gpu.py).

The checker takes every pair's value from tests.nearest_cases.oracle_values (the oracle's ComputeInitialDistanceMatrix over the stacked
rows, the block [0:nq, nq:]), states the rule a second time in plain numpy (`<=` on float32: NaN fails, -0 equals +0; column exclude[i]
of row i is left out) and lists the pairs in (i, j) order as a CSR over the queries: independent of imageclust_amd/csrc/pairs_select.h.
row_ptr and col must be equal, val must be equal as uint32 bit patterns."""
import numpy as np

from tests.nearest_cases import MAXF, mixed_sizes, oracle_values, random_rows, tie_rows  # noqa: F401  (the shared inputs, re-exported)
from tests.pairs_cases import few_copies, same, why  # noqa: F401  (the CSR comparison is the self-join's)


def select(V, threshold, exclude=None):
    """The pairs of V (nq x n) with V[i, j] <= threshold and j != exclude[i] -> (row_ptr int64[nq + 1], col int32[total], val float32[total])"""
    V = np.asarray(V, np.float32)
    nq, n = V.shape
    with np.errstate(invalid="ignore"):
        keep = V <= np.float32(threshold)
    if exclude is not None:
        ex = np.asarray(exclude, np.int64)
        rows = np.flatnonzero(ex >= 0)
        keep[rows, ex[rows]] = False
    i, j = np.nonzero(keep)  # row by row, ascending j inside a row
    row_ptr = np.zeros(nq + 1, np.int64)
    np.cumsum(np.bincount(i, minlength=nq)[:nq], out=row_ptr[1:])
    return row_ptr, j.astype(np.int32), V[i, j].astype(np.float32)


def expected(Q, L, threshold, q_size=None, l_size=None, exclude=None):
    return select(oracle_values(Q, L, q_size, l_size), threshold, exclude)


def tile_stats(V, threshold, exclude=None, tile=128, filled=None):
    """What icl_last_pairs_between_stats must report for the values V behind its split count: (tiles of the rectangle, tiles that hold a
    listed pair, pairs evaluated: the whole rectangle once and the pairs of the tiles with a hit a second time when the fill pass ran --
    filled; default: whenever anything is listed)"""
    V = np.asarray(V, np.float32)
    nq, n = V.shape
    rp, col, _ = select(V, threshold, exclude)
    H = np.zeros((nq, n), bool)
    H[np.repeat(np.arange(nq), np.diff(rp)), col] = True
    B, T = (nq + tile - 1) // tile, (n + tile - 1) // tile
    hit = again = 0
    for b in range(B):
        for t in range(T):
            if H[b * tile:(b + 1) * tile, t * tile:(t + 1) * tile].any():
                hit += 1
                again += min(tile, nq - b * tile) * min(tile, n - t * tile)
    if filled is None:
        filled = hit > 0
    return B * T, hit, nq * n + (again if filled else 0)


def between(V, lo_mask):
    """A threshold strictly between the planted pairs' values (lo_mask True) and every other value of V: the midpoint of the largest
    planted and the smallest other number, read from the oracle's values"""
    V = np.asarray(V, np.float32)
    lo, hi = V[lo_mask], V[~lo_mask]
    hi = hi[~np.isnan(hi)]
    assert len(lo) and len(hi) and lo.max() < hi.min(), "the planted pairs do not separate from the rest"
    return np.float32((np.float64(lo.max()) + np.float64(hi.min())) / 2)


def planted(nq, n, d, seed, kind="random"):
    """Q (nq x d) and L (n x d) of the given kind with every third query an exact copy of a library row -> (Q, L, plant: query -> row)"""
    rows = {"random": random_rows, "ties": tie_rows}[kind]
    Q, L = rows(nq, d, seed), rows(n, d, seed + 1)
    rng = np.random.default_rng(seed + 2)
    plant = {}
    for i in range(0, nq, 3):
        plant[i] = int(rng.integers(0, n))
        Q[i] = L[plant[i]]
    return Q, L, plant
