"""What the tests of icl_cluster_apart share (test_cluster_apart_large_cpu.py, test_cluster_apart_large_gpu.py; DESIGN.md "Constrained
seeded clustering, large N"): a checker with no cap on the seeds, the case lists and the comparisons.  The checker is tests/apart_cases.run's
rule -- the reference's loop over the oracle's primitives with the keep-apart relation B and its inheritance -- with D and B held ONCE, by
creation id, and updated in place: apart_cases.run refuses above 2 048 seeds and rebuilds both matrices per merge.  A dead cluster's row and
column hold MaxFloat32; creation ids order like the reference's positions (survivors keep their order, the merged cluster goes last), so
the first strict minimum in row-major order over this matrix is the one over the compacted matrix.  Problems, states and generators are
tests/apart_cases.py's and tests/seeded_cases.py's."""
import numpy as np

from oracle import oracle as O
from tests import apart_cases as AC
from tests import seeded_cases as SC

MAXF = SC.MAXF
# table word boundaries (31 .. 33, 63 .. 65), the 64-slot workgroup seam of the update kernel (64 / 65, 129, 255 .. 300), m <= 1
SHAPES_M = (1, 2, 17, 31, 32, 33, 63, 64, 65, 129, 255, 256, 300)
SHAPES_D = (3, 8, 1037)   # d % 4 != 0 twice, and more than one stage of the update kernel's pipeline
GRAPH_MERGES = 128        # 2 * GRAPH_STEPS of ward.hip: from this many merges asked for, the steps are replayed from a captured graph
WB_K = 16                 # ward.hip: from merge WB_K on a new cluster's row lies in recycled storage
ABOVE_CAP = (2100, 3)     # (m, d) above icl_cluster_many_apart's 2 048 seeds
ABOVE_CAP_MERGES = 200
ROWS_SINGLE_APART = 4     # include/imageclust.h ICL_ROWS_SINGLE_APART


def run(C, seed_size, min_size, max_size, k_target=0, apart_class=None, apart_pairs=None, inherit=True):
    """apart_cases.run with any number of seeds: the same dict, and "values": the picked pairs' Ward values in log order."""
    C = np.ascontiguousarray(C, np.float32)
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m, d = C.shape
    assert len(ss) == m and (ss != 0).all()
    N = int(np.abs(ss).sum())
    fail = lambda st: dict(status=st, cluster_id=np.full(m, -1, np.int32), seed_rank=np.full(m, -1, np.int32), n_clusters=0,
                           log=np.zeros((0, 2), np.int32), C_out=np.zeros((m, d), np.float32), finals=[], values=np.zeros(0, np.float32))
    if (ss > max_size).any():
        return fail(AC.ERR_UNSUPPORTED)
    if k_target > 0:
        k = int(k_target)
    else:
        k, err = O.calc_optimal_clusters(N, min_size, max_size)
        if err is not None:
            return fail(AC.ERR_CONSTRAINT)
    M = m + max(0, m - k)   # creation ids: the seeds, then one per merge asked for
    size = np.zeros(M, np.int64)
    size[:m] = np.abs(ss)
    frozen = np.zeros(M, bool)
    frozen[:m] = ss < 0
    cen = {i: C[i].copy() for i in range(m)}
    seeds = {i: [i] for i in range(m)}
    D = np.full((M, M), MAXF, np.float32)
    B = np.zeros((M, M), bool)
    if m:
        D[:m, :m] = O.initial_distance_matrix(C, np.abs(ss).astype(np.int32))
        B[:m, :m] = AC.relation(m, apart_class, apart_pairs)
    D[frozen, :] = MAXF
    D[:, frozen] = MAXF
    D[B] = MAXF
    live = np.zeros(M, bool)
    live[:m] = True
    log, values, made = [], [], m
    while int(live.sum()) > k:
        i, j = O.find_closest(D[:made])   # (rows below `made`: the ids that exist; the row pitch stays M)
        if i == -1 or j == -1:
            break
        if size[i] + size[j] > max_size:
            D[i, j] = D[j, i] = MAXF
            continue
        c = made
        values.append(D[i, j])
        log.append((i, j))
        size[c] = size[i] + size[j]
        cen[c] = O.merge_centroid(cen[i], int(size[i]), cen[j], int(size[j]))
        seeds[c] = seeds.pop(i) + seeds.pop(j)
        nb = (B[i] | B[j]) if inherit else np.zeros(M, bool)
        for q in (i, j):
            live[q] = False
            D[q, :] = MAXF
            D[:, q] = MAXF
            del cen[q]
        B[c, :] = nb
        B[:, c] = nb
        for q in np.flatnonzero(live):
            D[c, q] = D[q, c] = MAXF if (frozen[q] or nb[q]) else O.ward_distance(cen[q], int(size[q]), cen[c], int(size[c]))
        live[c] = True
        made += 1
    cid, rank, C_out = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros((m, d), np.float32)
    nc, finals = 0, []
    for c in np.flatnonzero(live):   # ascending creation id: surviving seeds in seed order, then the merged clusters in creation order
        c = int(c)
        finals.append((c, list(seeds[c]), int(size[c]), cen[c]))
        C_out[seeds[c][0]] = cen[c]
        if size[c] < min_size:
            continue
        for r, s in enumerate(seeds[c]):
            cid[s], rank[s] = nc, r
        nc += 1
    return dict(status=AC.OK, cluster_id=cid, seed_rank=rank, n_clusters=nc, log=np.array(log, np.int32).reshape(-1, 2), C_out=C_out,
                finals=finals, values=np.array(values, np.float32))


def same_run(a, b):
    """two results of run() / apart_cases.run(): what both hold is equal, floats as bits"""
    return (a["status"] == b["status"] and np.array_equal(a["cluster_id"], b["cluster_id"]) and np.array_equal(a["seed_rank"], b["seed_rank"])
            and a["n_clusters"] == b["n_clusters"] and np.array_equal(a["log"], b["log"]) and SC.same_bits(a["C_out"], b["C_out"])
            and [(f[0], f[1], f[2]) for f in a["finals"]] == [(f[0], f[1], f[2]) for f in b["finals"]]
            and all(SC.same_bits(x[3], y[3]) for x, y in zip(a["finals"], b["finals"])))


def large(ctx, job, **kw):
    """One constrained problem (C, seed_size, min, max, k_target, apart_class, apart_pairs) through Context.cluster_apart -> (cid, rank,
    nc, status, log, C_out)"""
    return ctx.cluster_apart(job[0], job[1], job[2], job[3], job[4], job[5], job[6], **kw)


def many(ctx, job, **kw):
    """The same problem through icl_cluster_many_apart (at most 2 048 seeds), the same tuple"""
    return ctx.cluster_many_apart([job], want_merges=True, want_centroids=True, **kw)[0]


def same_tuple(a, b, what):
    """two results of large() / many() / Context.cluster_seeded: everything equal, C_out as bits"""
    assert a[3] == b[3], (what, a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y), what
    assert np.array_equal(a[4], b[4]), what
    assert SC.same_bits(a[5], b[5]), what


def same_as_checker(r, ref, what, values=None):
    """r: a result of large(); ref: run()'s; values: Context.last_merge_values() behind the call.  Bit-exact."""
    SC.same_as_checker(r, ref, what)
    if values is not None:
        assert np.array_equal(np.asarray(values, np.float32).view(np.uint32), ref["values"].view(np.uint32)), what


def case(kind, m, d):
    """AC.constrained(m, d) / AC.anchored(m, d); a lone seed, which AC.constrained cannot draw two class members from, carries class 1"""
    if kind == "anchored":
        return AC.anchored(m, d)
    if m < 2:
        C, ss, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
        return C, ss, mn, mx, 0, np.ones(m, np.int32), None
    return AC.constrained(m, d)


def above_cap(kind):
    """The problems above icl_cluster_many_apart's cap: AC.constrained / AC.anchored's construction at m = 2 100, d = 3 with a k_target
    that asks for ABOVE_CAP_MERGES merges (AC.constrained itself takes its pairs from apart_cases' capped checker)."""
    m, d = ABOVE_CAP
    C, ss, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
    kt = m - ABOVE_CAP_MERGES
    if kind == "anchored":   # every unfrozen seed of at least min_size items is an anchor; the rest may go to them or to each other
        return C, ss, mn, mx, kt, (ss >= mn).astype(np.int32), None
    base = run(C, ss, mn, mx, kt)["log"]
    pairs = np.array([(a, b) for a, b in base[:max(1, len(base) // 4)] if a < m and b < m], np.int32).reshape(-1, 2)
    cls = np.zeros(m, np.int32)
    cls[np.random.default_rng(7 + m + d).choice(m, max(2, m // 8), replace=False)] = 1
    return C, ss, mn, mx, kt, cls, pairs


def engine_on(calls):
    """The stand-in engine of Clustering (tests/test_cluster_apart_cpu.engine_with) over the cap-free checker"""
    def engine(C, ss, mn, mx, kt, *extra):
        calls.append(extra)
        r = run(C, ss, mn, mx, kt, *extra)
        return r["cluster_id"], r["seed_rank"], r["n_clusters"], r["status"], r["log"], r["C_out"]
    return engine
