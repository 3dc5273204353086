"""Inputs and the checker of the icl_cluster_fit tests (tests/test_cluster_fit_cpu.py, tests/test_cluster_fit_gpu.py).

The checker takes every pair's value from the oracle (tests.nearest_cases.oracle_values, with a frozen cluster's item count), reads the
own cost off it, orders each row's alternatives with a STABLE sort by value over ascending j -- NaN last, as numpy sorts -- and finds
rep / worst with explicit loops: a second statement of the rules, independent of imageclust_amd/csrc/fit_select.h."""
import numpy as np

from tests import nearest_cases as NC

MAXF = NC.MAXF
FIELDS = ("own", "alt_idx", "alt_val", "listed", "rep", "worst")
K_ALTS = (0, 1, 10, 64)
# (nq, K, d): no alternative at all; the smallest with one; one cluster; two bands; two column tiles and the scalar loads; the wide loads
CASES = [(1, 1, 1), (2, 2, 3), (5, 1, 7), (130, 3, 5), (300, 129, 33), (257, 260, 64)]
SPLIT_CASE = (64, 700, 16)  # six column tiles: column_splits 1, 2, 3 and 7


def from_values(V, cluster_of, k_alt, q_size=None, c_size=None, max_size=0):
    """The expected result from the nq x K values V -> dict of FIELDS"""
    V = np.asarray(V, np.float32)
    nq, K = V.shape
    cof = np.asarray(cluster_of, np.int64).reshape(-1)
    cs = np.ones(K, np.int64) if c_size is None else np.asarray(c_size, np.int64)
    qs = np.ones(nq, np.int64) if q_size is None else np.asarray(q_size, np.int64)
    own = np.full(nq, MAXF, np.float32)
    idx, val = np.full((nq, k_alt), -1, np.int32), np.full((nq, k_alt), MAXF, np.float32)
    for i in range(nq):
        if cof[i] >= 0:
            own[i] = V[i, cof[i]]
        keep = cs > 0                                   # a frozen cluster is never offered
        if cof[i] >= 0:
            keep[cof[i]] = False                        # nor the row's own
        if max_size > 0:
            keep &= qs[i] + cs <= max_size              # nor one the row would push above max_size
        js = np.flatnonzero(keep)
        js = js[np.argsort(V[i, js], kind="stable")][:k_alt]
        idx[i, :len(js)] = js
        val[i, :len(js)] = V[i, js]
    listed, rep, worst = np.zeros(K, np.int32), np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    for i in range(nq):                                 # ascending i: a later row replaces an earlier one only when strictly better
        c = cof[i]
        if c < 0:
            continue
        listed[c] += 1
        v = own[i]
        if rep[c] < 0:
            rep[c] = worst[c] = i
            continue
        r, w = own[rep[c]], own[worst[c]]
        if (np.isnan(r) and not np.isnan(v)) or (not np.isnan(r) and not np.isnan(v) and v < r):
            rep[c] = i
        if (np.isnan(v) and not np.isnan(w)) or (not np.isnan(w) and not np.isnan(v) and v > w):
            worst[c] = i
    return dict(own=own, alt_idx=idx, alt_val=val, listed=listed, rep=rep, worst=worst)


def values(Q, C, q_size=None, c_size=None):
    """-> float32[nq][K] by the oracle; a frozen cluster (negative size) with its item count"""
    return NC.oracle_values(Q, C, q_size, None if c_size is None else np.abs(np.asarray(c_size, np.int32)))


def expected(Q, C, cluster_of, k_alt, q_size=None, c_size=None, max_size=0):
    return from_values(values(Q, C, q_size, c_size), cluster_of, k_alt, q_size, c_size, max_size)


def _bits_differ(g, w):
    g, w = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(w, np.float32)
    return (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))


def why(got, want):
    """"" when the two results are equal -- integers as they are, floats as uint32 bit patterns, NaN by isnan -- else the first difference"""
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        if g.shape != w.shape:
            return "%s: shape %s, want %s" % (f, g.shape, w.shape)
        bad = np.argwhere(_bits_differ(g, w) if w.dtype == np.float32 else g != w)
        if len(bad):
            at = tuple(int(x) for x in bad[0])
            return "%s: %d entries differ; first at %s: got %r, want %r" % (f, len(bad), at, g[at], w[at])
    return ""


def problem(nq, K, d, seed, plain=False):
    """A problem of the given shape with everything the rules can meet, as far as the shape has room for it: mixed sizes, frozen own
    clusters and frozen alternatives, a max_size that bans many pairs, rows of no cluster, a cluster nobody names, duplicate rows inside
    one cluster, duplicate centroids, one NaN row, +-Inf entries.  plain: finite rows, no frozen cluster, every row in a cluster.
    -> dict(Q, C, cluster_of, q_size, c_size, max_size)"""
    rng = np.random.default_rng(seed)
    Q, C = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((K, d)).astype(np.float32)
    qs, cs = rng.integers(1, 7, nq).astype(np.int32), rng.integers(1, 10, K).astype(np.int32)
    cof = rng.integers(0, K, nq).astype(np.int32) if K else np.full(nq, -1, np.int32)
    if plain:
        return dict(Q=Q, C=C, cluster_of=cof, q_size=qs, c_size=cs, max_size=12)
    if K >= 3:
        cof[cof == 1] = 0        # nobody names cluster 1
        cs[2::5] *= -1           # frozen: cluster 2 (named by some rows), 7, 12, ...
    if K >= 5:
        C[4], cs[4], cs[3] = C[3], 2, 2   # duplicate centroids of one size: equal values, the tie goes by j
    if K >= 2:
        C[K - 1, 0] = np.inf
    if nq >= 4 and K:
        cof[3::7] = -1
    if nq >= 8 and K:
        Q[7], qs[7], cof[7], cof[6] = Q[6], qs[6], max(int(cof[6]), 0), max(int(cof[6]), 0)   # a tie inside one cluster: the lower row
    if nq >= 6 and K:
        Q[4, d // 2] = np.nan    # own NaN: rep passes over row 4, worst takes it
        cof[4] = cof[5] = max(int(cof[5]), 0)
    if nq >= 3:
        Q[2, 0] = -np.inf
    return dict(Q=Q, C=C, cluster_of=cof, q_size=qs, c_size=cs, max_size=7)


def covers(P, want):
    """What a problem() of at least 8 rows and 5 clusters must contain, read off its expected result at k_alt = 64: "" or what is missing"""
    cof, cs = P["cluster_of"], P["c_size"]
    if not (want["rep"][1] == -1 and want["listed"][1] == 0):
        return "a cluster nobody names"
    if not (np.isnan(want["own"][4]) and want["worst"][cof[4]] == 4 and want["rep"][cof[4]] not in (4, -1)):
        return "a NaN row that worst takes and rep passes over"
    if not ((cof < 0).any() and (want["own"][cof < 0] == MAXF).all()):
        return "rows of no cluster"
    if not ((want["alt_idx"][:, -1] == -1) & (want["alt_idx"][:, 0] >= 0)).any():
        return "rows the ban leaves short"
    if not (cs[cof[cof >= 0]] < 0).any() or np.isin(want["alt_idx"], np.flatnonzero(cs < 0)).any():
        return "frozen own clusters that nobody is offered"
    if not (want["rep"][cof[6]] != 7 and want["own"][6].view(np.uint32) == want["own"][7].view(np.uint32)):
        return "a tie inside one cluster"
    if not np.isinf(want["alt_val"]).any():
        return "infinite values"
    both = (want["alt_idx"] == 3).any(1) & (want["alt_idx"] == 4).any(1)
    if not both.any() or not all(list(r).index(3) + 1 == list(r).index(4) for r in want["alt_idx"][both]):
        return "duplicate centroids listed side by side, the lower column first"
    return ""


def plant_own_column(res, cluster_of, V):
    """A copy of a result with fault 1: row 0's own cluster offered as its first alternative"""
    bad = {f: np.array(a, copy=True) for f, a in res.items()}
    bad["alt_idx"][0, 0], bad["alt_val"][0, 0] = cluster_of[0], V[0, cluster_of[0]]
    return bad


def plant_highest_index_tie(res, cluster_of):
    """A copy of a result with fault 2: ties for rep go to the HIGHEST row"""
    bad = {f: np.array(a, copy=True) for f, a in res.items()}
    own, cof = res["own"], np.asarray(cluster_of)
    for c in range(len(bad["rep"])):
        r = bad["rep"][c]
        if r >= 0:
            tied = np.flatnonzero((cof == c) & (own == own[r]))
            bad["rep"][c] = tied[-1]
    return bad
