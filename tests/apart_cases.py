"""What the constrained seeded-clustering tests share (test_cluster_apart_cpu.py, test_cluster_apart_gpu.py): the checker -- tests/
seeded_cases.run with the keep-apart relation B and its inheritance (DESIGN.md "Constrained seeded clustering") --, the state after t
merges of a log with the bans its clusters inherited, and the case lists.  A constrained problem is (C, seed_size, min_size, max_size,
k_target, apart_class, apart_pairs), as Context.cluster_many_apart takes it."""
import numpy as np

from oracle import oracle as O
from tests import seeded_cases as SC

OK, ERR_CONSTRAINT, ERR_UNSUPPORTED = SC.OK, SC.ERR_CONSTRAINT, SC.ERR_UNSUPPORTED
MAXF = SC.MAXF


def relation(m, apart_class=None, apart_pairs=None):
    """B at the start: m x m bool, symmetric, False on the diagonal."""
    B = np.zeros((m, m), bool)
    if apart_pairs is not None:
        for a, b in np.asarray(apart_pairs, np.int64).reshape(-1, 2):
            assert 0 <= a < m and 0 <= b < m and a != b
            B[a, b] = B[b, a] = True
    if apart_class is not None:
        cls = np.asarray(apart_class, np.int64).reshape(-1)
        assert len(cls) == m and (cls >= 0).all()
        B |= (cls[:, None] == cls[None, :]) & (cls[:, None] != 0)
        np.fill_diagonal(B, False)
    return B


def run(C, seed_size, min_size, max_size, k_target=0, apart_class=None, apart_pairs=None, inherit=True):
    """seeded_cases.run with B: the same dict.  inherit=False: a merged cluster is apart from nobody (what a kernel that bans only at
    the start computes) -- for the tests' own use."""
    C = np.ascontiguousarray(C, np.float32)
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m, d = C.shape
    assert len(ss) == m and (ss != 0).all()
    N = int(np.abs(ss).sum())
    fail = lambda st: dict(status=st, cluster_id=np.full(m, -1, np.int32), seed_rank=np.full(m, -1, np.int32), n_clusters=0,
                           log=np.zeros((0, 2), np.int32), C_out=np.zeros((m, d), np.float32), finals=[])
    if (ss > max_size).any() or m > SC.MAX_SEEDS:
        return fail(ERR_UNSUPPORTED)
    if k_target > 0:
        k = int(k_target)
    else:
        k, err = O.calc_optimal_clusters(N, min_size, max_size)
        if err is not None:
            return fail(ERR_CONSTRAINT)
    B = relation(m, apart_class, apart_pairs)
    cl = [[i, [i], int(abs(ss[i])), bool(ss[i] < 0), C[i].copy()] for i in range(m)]
    D = O.initial_distance_matrix(C, np.abs(ss).astype(np.int32)) if m else np.zeros((0, 0), np.float32)
    for i in range(m):
        if cl[i][3]:
            D[i, :] = MAXF
            D[:, i] = MAXF
    D[B] = MAXF
    log = []
    while len(cl) > k:
        i, j = O.find_closest(D)
        if i == -1 or j == -1:
            break
        if cl[i][2] + cl[j][2] > max_size:
            D[i, j] = D[j, i] = MAXF
            continue
        a, b = cl[i], cl[j]
        new = [m + len(log), a[1] + b[1], a[2] + b[2], False, O.merge_centroid(a[4], a[2], b[4], b[2])]
        log.append((a[0], b[0]))
        keep = [q for q in range(len(cl)) if q != i and q != j]
        nb = (B[i, keep] | B[j, keep]) if inherit else np.zeros(len(keep), bool)
        cl = [cl[q] for q in keep] + [new]
        D2 = np.zeros((len(cl), len(cl)), np.float32)
        B2 = np.zeros((len(cl), len(cl)), bool)
        D2[:-1, :-1] = D[np.ix_(keep, keep)]
        B2[:-1, :-1] = B[np.ix_(keep, keep)]
        B2[-1, :-1] = B2[:-1, -1] = nb
        for q, c in enumerate(cl[:-1]):
            D2[q, -1] = D2[-1, q] = MAXF if (c[3] or nb[q]) else O.ward_distance(c[4], c[2], new[4], new[2])
        D, B = D2, B2
    cid, rank, C_out = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros((m, d), np.float32)
    nc = 0
    for c in cl:
        C_out[c[1][0]] = c[4]
        if c[2] < min_size:
            continue
        for r, s in enumerate(c[1]):
            cid[s], rank[s] = nc, r
        nc += 1
    return dict(status=OK, cluster_id=cid, seed_rank=rank, n_clusters=nc, log=np.array(log, np.int32).reshape(-1, 2), C_out=C_out,
                finals=[(c[0], list(c[1]), c[2], c[4]) for c in cl])


def state_after(C, seed_size, log, t, apart_class=None, apart_pairs=None):
    """seeded_cases.state_after, and the bans the state's clusters hold: (C', seed_size', seeds', ids', pairs') -- pairs' lists (a, b),
    a < b, positions in the state's list, for every two clusters one of whose seeds is apart from one of the other's."""
    C2, ss2, seeds, ids = SC.state_after(C, seed_size, log, t)
    B = relation(len(np.asarray(seed_size).reshape(-1)), apart_class, apart_pairs)
    pairs = [(a, b) for b in range(len(seeds)) for a in range(b) if B[np.ix_(seeds[a], seeds[b])].any()]
    return C2, ss2, seeds, ids, np.array(pairs, np.int32).reshape(-1, 2)


def constrained(m, d, seed=None, ties=False):
    """The case of the issue's measurement over seeded_cases.mixed_problem(m, d): the seed pairs among the first quarter of the
    unconstrained log must stay apart, and class 1 lies on max(2, m // 8) random seeds -> the problem as cluster_many_apart takes it."""
    C, ss, mn, mx = SC.mixed_problem(m, d, 100 + m + d if seed is None else seed, ties=ties)
    base = SC.run(C, ss, mn, mx)["log"]
    pairs = np.array([(a, b) for a, b in base[:max(1, len(base) // 4)] if a < m and b < m], np.int32).reshape(-1, 2)
    cls = np.zeros(m, np.int32)
    cls[np.random.default_rng(7 + m + d).choice(m, max(2, m // 8), replace=False)] = 1
    return C, ss, mn, mx, 0, cls, pairs


def anchored(m, d, k_target=None):
    """"Put the leftovers somewhere": every unfrozen seed of at least min_size items is class 1 -- they take leftovers but not each
    other -- and k_target (default) is their number plus the frozen seeds."""
    C, ss, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
    cls = (ss >= mn).astype(np.int32)
    kt = max(1, int(cls.sum() + (ss < 0).sum())) if k_target is None else k_target
    return C, ss, mn, mx, kt, cls, None


KNOWN = (np.array([[0.0], [1.0], [2.1], [10.0]], np.float32), np.ones(4, np.int32), 1, 100, 1, None, np.array([[0, 2]], np.int32))
KNOWN_LOG = np.array([[1, 0], [3, 2]], np.int32)

CASES_M = (17, 64, 255, 256)   # the small route
CASES_MID = (300,)             # the mid route
CASES_D = (3, 8)               # (the dimensions at which the separation below was measured on the CPU)


def same_as_checker(r, ref, what):
    SC.same_as_checker(r, ref, what)
