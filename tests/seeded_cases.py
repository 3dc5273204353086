"""What the seeded-clustering tests share (test_cluster_seeded_cpu.py, test_cluster_seeded_gpu.py): the checker -- the reference's
loop (clustering.go:216-246) in Python over the oracle's primitives, started from any list of seed clusters -- the state after t
merges of a log, and the case lists.  A seed is (centroid row, size); a negative size marks a frozen seed (DESIGN.md "Seeded
clustering")."""
import numpy as np

from oracle import oracle as O
from tests import ward_cases as WC

OK, ERR_CONSTRAINT, ERR_UNSUPPORTED = 0, 2, 6
MAXF = np.float32(np.finfo(np.float32).max)
MAX_SEEDS = 2048


def run(C, seed_size, min_size, max_size, k_target=0):
    """The seeded problem on the CPU -> dict(status, cluster_id, seed_rank, n_clusters, log, C_out, finals); finals: the final list,
    (creation id, seed sequence, item count, centroid) per cluster, dropped ones included.  A failed problem has rows of -1."""
    C = np.ascontiguousarray(C, np.float32)
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m, d = C.shape
    assert len(ss) == m and (ss != 0).all()
    N = int(np.abs(ss).sum())
    fail = lambda st: dict(status=st, cluster_id=np.full(m, -1, np.int32), seed_rank=np.full(m, -1, np.int32), n_clusters=0,
                           log=np.zeros((0, 2), np.int32), C_out=np.zeros((m, d), np.float32), finals=[])
    if (ss > max_size).any() or m > MAX_SEEDS:
        return fail(ERR_UNSUPPORTED)
    if k_target > 0:
        k = int(k_target)
    else:
        k, err = O.calc_optimal_clusters(N, min_size, max_size)
        if err is not None:
            return fail(ERR_CONSTRAINT)
    # clusters: [creation id, seeds, items, frozen, centroid]
    cl = [[i, [i], int(abs(ss[i])), bool(ss[i] < 0), C[i].copy()] for i in range(m)]
    D = O.initial_distance_matrix(C, np.abs(ss).astype(np.int32)) if m else np.zeros((0, 0), np.float32)
    for i in range(m):
        if cl[i][3]:  # a frozen seed: every pair with it is banned from the start (:230-231)
            D[i, :] = MAXF
            D[:, i] = MAXF
    log = []
    while len(cl) > k:
        i, j = O.find_closest(D)
        if i == -1 or j == -1:
            break
        if cl[i][2] + cl[j][2] > max_size:  # :228-234
            D[i, j] = D[j, i] = MAXF
            continue
        a, b = cl[i], cl[j]
        new = [m + len(log), a[1] + b[1], a[2] + b[2], False, O.merge_centroid(a[4], a[2], b[4], b[2])]  # :37-40
        log.append((a[0], b[0]))
        keep = [q for q in range(len(cl)) if q != i and q != j]
        cl = [cl[q] for q in keep] + [new]
        D2 = np.zeros((len(cl), len(cl)), np.float32)
        D2[:-1, :-1] = D[np.ix_(keep, keep)]
        for q, c in enumerate(cl[:-1]):  # :76-96
            D2[q, -1] = D2[-1, q] = MAXF if c[3] else O.ward_distance(c[4], c[2], new[4], new[2])
        D = D2
    cid, rank, C_out = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros((m, d), np.float32)
    nc = 0
    for c in cl:
        C_out[c[1][0]] = c[4]
        if c[2] < min_size:  # :268-271
            continue
        for r, s in enumerate(c[1]):
            cid[s], rank[s] = nc, r
        nc += 1
    return dict(status=OK, cluster_id=cid, seed_rank=rank, n_clusters=nc, log=np.array(log, np.int32).reshape(-1, 2), C_out=C_out,
                finals=[(c[0], list(c[1]), c[2], c[4]) for c in cl])


def state_after(C, seed_size, log, t):
    """The cluster list after the first t merges of log, as a seeded problem: (C', seed_size', seeds', ids') in list order --
    surviving seeds in seed order, then the merged clusters in creation order; seeds': each cluster's seed sequence; ids': its
    creation id in the run the log comes from.  Centroids by MergeClusters (oracle), bit for bit the loop's."""
    C = np.ascontiguousarray(C, np.float32)
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m = len(ss)
    cl = {i: ([i], int(abs(ss[i])), bool(ss[i] < 0), C[i]) for i in range(m)}
    for u in range(t):
        a, b = cl.pop(int(log[u][0])), cl.pop(int(log[u][1]))
        cl[m + u] = (a[0] + b[0], a[1] + b[1], False, O.merge_centroid(a[3], a[1], b[3], b[1]))
    ids = sorted(cl)
    C2 = np.stack([cl[c][3] for c in ids]).astype(np.float32) if ids else np.zeros((0, C.shape[1]), np.float32)
    return C2, np.array([-cl[c][1] if cl[c][2] else cl[c][1] for c in ids], np.int32), [cl[c][0] for c in ids], ids


def resumed_log(log, t, ids, m):
    """What a run resumed from state_after(.., t) must log, in ITS creation ids: the rest of log with the state's clusters renumbered
    0 .. m' - 1 in list order and merge t + u of the first run as m' + u."""
    new = {old: i for i, old in enumerate(ids)}
    for u in range(len(log) - t):
        new[m + t + u] = len(ids) + u
    return np.array([(new[int(a)], new[int(b)]) for a, b in log[t:]], np.int32).reshape(-1, 2)


def cuts(n_merges):
    """after the first merge, at the middle, before the last merge"""
    return sorted({t for t in (1, n_merges // 2, n_merges - 1) if 0 < t < n_merges})


def centroids_from_log(C, seed_size, log):
    """C_out of a run with this log: the row of each final cluster's rank-0 seed holds its centroid, every other row is zero."""
    C2, _, seeds, _ = state_after(C, seed_size, log, len(log))
    out = np.zeros_like(np.ascontiguousarray(C, np.float32))
    for row, sq in zip(C2, seeds):
        out[sq[0]] = row
    return out


def small_singleton_cases(n_max=48):
    """tests/ward_cases.small_cases() of at most n_max rows: (name, E, min, max)"""
    return [c for c in WC.small_cases() if c[1].shape[0] <= n_max]


def mixed_problem(m, d, seed, max_size=9, min_size=3, frozen_every=5, ties=False):
    """m seeds of mixed sizes: sizes 1 .. 4 and max_size (every pair of such a seed is banned), every frozen_every-th seed frozen
    (one of them below min_size, one above max_size), duplicated centroids; ties=True: small-integer coordinates."""
    rng = np.random.default_rng(seed)
    C = WC.ties(m, d, seed, levels=3) if ties else WC.mog(m, d, seed, k=max(1, m // 6), sigma=0.3)
    if m >= 4:
        C[m // 2] = C[0]  # duplicates: a value of exactly 0, and equal values to order by id
        C[m - 1] = C[1]
    ss = rng.choice(np.array([1, 1, 1, 1, 2, 2, 3, 4, max_size], np.int32), m).astype(np.int32)  # (mostly small: merges stay possible)
    if m >= 3:
        ss[2] = max_size
    if frozen_every:
        fr = np.arange(m) % frozen_every == frozen_every - 1
        ss[fr] = -ss[fr]
        idx = np.flatnonzero(fr)
        if len(idx) >= 1:
            ss[idx[0]] = -1
        if len(idx) >= 2:
            ss[idx[1]] = -(max_size + 4)
    return np.ascontiguousarray(C, np.float32), ss, min_size, max_size


SHAPES_M = (0, 1, 2, 3, 17, 64, 255, 256)
SHAPES_D = (3, 8, 1037)
MID_SHAPES = ((257, 8), (300, 8), (300, 1037))


def same_as_checker(r, ref, what):
    """r: one result of Context.cluster_many_seeded(want_merges=True, want_centroids=True); ref: run()'s.  Bit-exact."""
    cid, rank, nc, st, log, C_out = r
    assert st == ref["status"], (what, st, ref["status"])
    assert np.array_equal(cid, ref["cluster_id"]) and np.array_equal(rank, ref["seed_rank"]) and nc == ref["n_clusters"], what
    assert np.array_equal(log, ref["log"]), what
    assert same_bits(C_out, ref["C_out"]), what


def same_bits(a, b):
    """Equal as uint32; where both hold a NaN its payload is left aside (which NaN an operation returns is the hardware's choice, not
    the reference's arithmetic: Go leaves it open too)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
