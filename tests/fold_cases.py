"""What the fold-centroid tests share (test_fold_centroids_cpu.py, test_fold_centroids_gpu.py, test_clustering_edit_*.py): the rule of
icl_fold_centroids restated in numpy float32 -- MergeClusters (clustering.go:29-47) folded over a member list in list order, one rounded
operation per line --, the planted mistakes the cases must tell from it, the case list, and the bit comparison.  (DESIGN.md "Editing a
held clustering".)"""
import numpy as np

STAGE, BATCH = 256, 8  # imageclust_amd/csrc/fold_plan.h: members staged in LDS at a time, rows loaded ahead of their chain steps
MISTAKES = ("sorted", "mean", "contracted", "weight1", "total_late", "total_in_f32")


def fold(E, row_ptr, member, size=None, mistake=None):
    """The rule, one group at a time -> (C float32[K][d], size_out int32[K]).  mistake: one of MISTAKES, a wrong kernel's arithmetic."""
    E = np.ascontiguousarray(E, np.float32)
    row_ptr, member = np.asarray(row_ptr, np.int64), np.asarray(member, np.int64)
    K, d = len(row_ptr) - 1, E.shape[1]
    C, total = np.zeros((K, d), np.float32), np.zeros(K, np.int32)
    with np.errstate(all="ignore"):
        for g in range(K):
            ms = member[row_ptr[g]:row_ptr[g + 1]]
            if len(ms) == 0:
                continue  # a row of +0.0, size 0
            if mistake == "sorted":
                ms = np.sort(ms)
            item = [int(size[m]) if size is not None else 1 for m in ms]
            if mistake == "mean":  # sum, then one division
                acc = np.float32(item[0]) * E[ms[0]] if len(ms) > 1 else E[ms[0]].copy()
                for m, s in zip(ms[1:], item[1:]):
                    acc = acc + np.float32(s) * E[m]
                C[g], total[g] = (acc / np.float32(sum(item)) if len(ms) > 1 else acc), sum(item)
                continue
            c, S = E[ms[0]].copy(), item[0]  # the first member: copied, not merged with anything
            for m, s in zip(ms[1:], item[1:]):
                fa = np.float32(S + s if mistake == "total_late" else S)
                fb = np.float32(1 if mistake == "weight1" else s)
                fs = np.float32(S) + np.float32(s) if mistake == "total_in_f32" else np.float32(S + s)
                if mistake == "contracted":  # products and sum in float64, rounded once
                    sm = (fa.astype(np.float64) * c.astype(np.float64) + fb.astype(np.float64) * E[m].astype(np.float64)).astype(np.float32)
                else:
                    pa = fa * c
                    pb = fb * E[m]
                    sm = pa + pb
                c = sm / fs
                S += s
            C[g], total[g] = c, S
    return C, total


def engine(E, row_ptr, member, size):
    """Clustering's fold_engine: the restatement standing in for Context.fold_centroids."""
    return fold(E, row_ptr, member, size)


def why(got, want):
    """None when (C, size_out) pairs are equal -- floats as uint32, a NaN against any NaN, sizes as integers -- else the first difference."""
    (gc, gs), (wc, ws) = got, want
    gc, wc = np.ascontiguousarray(gc, np.float32), np.ascontiguousarray(wc, np.float32)
    if gc.shape != wc.shape:
        return "shapes %s and %s" % (gc.shape, wc.shape)
    if not np.array_equal(np.asarray(gs, np.int64), np.asarray(ws, np.int64)):
        g = int(np.flatnonzero(np.asarray(gs, np.int64) != np.asarray(ws, np.int64))[0])
        return "size_out[%d] is %d, not %d" % (g, gs[g], ws[g])
    bad = (gc.view(np.uint32) != wc.view(np.uint32)) & ~(np.isnan(gc) & np.isnan(wc))
    if bad.any():
        g, k = np.argwhere(bad)[0]
        return "%d elements differ, first C[%d][%d]: %r (0x%08x), not %r (0x%08x)" % (int(bad.sum()), g, k, gc[g, k], gc.view(np.uint32)[g, k],
                                                                                     wc[g, k], wc.view(np.uint32)[g, k])
    return None


def csr(lengths, n, rng):
    """Groups of these lengths over rows drawn from [0, n) with repetition: rows come shuffled, some twice, some never."""
    row_ptr = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))]).astype(np.int64)
    return row_ptr, rng.integers(0, max(n, 1), int(row_ptr[-1])).astype(np.int32)


def rows(n, d, rng):
    return (rng.standard_normal((n, d)) * rng.choice([0.01, 1.0, 300.0], (n, 1))).astype(np.float32)


LENGTHS = list(range(18)) + [STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + BATCH + 1]  # 0 .. 17 holds BATCH - 1, BATCH, BATCH + 1
WIDTHS = (1, 3, 4, 8, 1037, 2048, 2052)  # 1 024 columns is the most one workgroup covers in the 16-byte form, 256 in the scalar form


def width_case(d, sized):
    rng = np.random.default_rng(1000 + d)
    n = 97
    E = rows(n, d, rng)
    row_ptr, member = csr(LENGTHS, n, rng)
    member[row_ptr[5]:row_ptr[5] + 2] = 7  # a row twice in one group ...
    member[row_ptr[9]] = 7                 # ... and in another
    size = rng.integers(1, 51, n).astype(np.int32) if sized else None
    return E, row_ptr, member, size


def special_case():
    """Rows holding NaN, +-Inf and -0.0; one-member groups must reproduce their row's bits (the sign of zero, the NaN's payload aside)."""
    rng = np.random.default_rng(7)
    E = rows(24, 8, rng)
    E[0, 1], E[1, 2], E[2, 3], E[3, :] = np.nan, np.inf, -np.inf, -0.0
    E[4, 0] = -0.0
    groups = [[0], [1], [2], [3], [4], [3, 3], [3, 4, 3], [0, 5, 6], [5, 1, 6], [6, 2, 1], [5, 3], [3, 5], [7, 8, 9, 10, 0, 11]]
    row_ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return E, row_ptr, np.array([i for g in groups for i in g], np.int32), None


def big_sizes_case():
    """Item counts around 2^24 + 1, where float(S) rounds: the total must be kept as an integer.  60 members: below INT32_MAX."""
    rng = np.random.default_rng(24)
    n, d = 80, 8
    E = rows(n, d, rng)
    size = ((1 << 24) + rng.integers(-3, 4, n)).astype(np.int32)
    size[60:] = rng.integers(1, 4, n - 60)  # rows 60 ..: small counts
    row_ptr, member = csr([60, 2, 3, 0, 17, 100], n, rng)
    member[:60] = rng.permutation(60)  # 60 counts of about 2^24: 1.0e9 items
    member[row_ptr[5]:] = rng.integers(60, n, 100)
    member[row_ptr[4]] = 61  # a small cluster first, large counts behind it
    return E, row_ptr, member, size


def long_case():
    rng = np.random.default_rng(5000)
    E = rows(211, 8, rng)
    row_ptr, member = csr([5000, 3], 211, rng)
    return E, row_ptr, member, None


def count_case(K, d=8):
    rng = np.random.default_rng(300 + K)
    n = 64
    E = rows(n, d, rng)
    row_ptr, member = csr(rng.integers(0, 21, K), n, rng)
    return E, row_ptr, member, rng.integers(1, 51, n).astype(np.int32)


def many_groups_case():
    """70 000 groups of 0 .. 3 members, d = 3: more workgroups than a grid dimension of 65 535 holds."""
    rng = np.random.default_rng(70000)
    E = rows(1000, 3, rng)
    row_ptr, member = csr(rng.integers(0, 4, 70000), 1000, rng)
    return E, row_ptr, member, None


def geometry(K, d, aligned, compute_units):
    """fold_plan.h's fold_geometry -> (vec, threads, chunks): the 16-byte form?, threads per workgroup, chunks of columns per group.
    tests/test_fold_centroids_cpu.py holds it against the header itself."""
    vec = bool(aligned and d % 4 == 0)
    owners = -(-d // (4 if vec else 1))
    want, threads = 4 * max(compute_units, 1), 256
    while threads > 64 and (owners <= threads // 2 or K * -(-owners // threads) < want):
        threads //= 2
    return vec, threads, -(-owners // threads)


# (name, K, d, sized): enough groups that the workgroups keep several waves on a device of 256 compute units -- 4 x 256 workgroups
# at 256 threads for K = 1 100, at 128 but not at 256 for K = 300 (K = 150 at d = 1037) -- so that the stage loop's barriers order different waves.
# d = 2052 (16-byte form) and d = 1037 (one column per thread) leave dead lanes in the last chunk, which must keep meeting the barriers.
WAVES = (("4 waves d=2048", 1100, 2048, True), ("4 waves d=2052", 1100, 2052, False), ("4 waves d=1037", 1100, 1037, True),
         ("2 waves d=2048", 300, 2048, False), ("2 waves d=2052", 300, 2052, True), ("2 waves d=1037", 150, 1037, False))


def waves_case(K, d, sized):
    """LENGTHS (0 .. 17, 255 / 256 / 257, 521: several LDS stages) shuffled among short groups"""
    rng = np.random.default_rng(K + d)
    n = 61
    E = rows(n, d, rng)
    lengths = rng.permutation(np.concatenate([LENGTHS, rng.integers(0, 6, K - len(LENGTHS))]))
    row_ptr, member = csr(lengths, n, rng)
    return E, row_ptr, member, rng.integers(1, 51, n).astype(np.int32) if sized else None


def cases(big=True):
    """[(name, E, row_ptr, member, size), ...]; big=False leaves out the 70 000-group case and the many-group cases of WAVES."""
    out = [("d=%d %s" % (d, "sized" if sized else "unsized"),) + width_case(d, sized) for d in WIDTHS for sized in (False, True)]
    out.append(("special rows",) + special_case())
    out.append(("sizes around 2^24",) + big_sizes_case())
    out.append(("one group of 5000",) + long_case())
    out += [("K=%d" % K,) + count_case(K) for K in (0, 1, 2, 300)]
    if big:
        out.append(("K=70000",) + many_groups_case())
        out += [(name,) + waves_case(K, d, sized) for name, K, d, sized in WAVES]
    return out


# ---- stand-ins for the engines a Clustering state calls, and what the edit tests compare -------------------------------------------
MAXF = np.float32(np.finfo(np.float32).max)


def _ward_row(X, sx, y, sy):
    """WardDistance (clustering.go:136-157) of each row of X (item counts sx) against y (sy items): differences, products and the
    sum each rounded, in k order, then (float(sa * sb) / float(sa + sb)) * s."""
    s = np.zeros(len(X), np.float32)
    for k in range(X.shape[1]):
        df = X[:, k] - y[k]
        s = s + df * df
    return ((sx * sy).astype(np.float32) / (sx + sy).astype(np.float32)) * s


def seeded_engine(C, seed_size, min_size, max_size, k_target=0):
    """Clustering's `engine` for unfrozen seeds: the reference's loop (clustering.go:216-246) from existing clusters, the answer of
    tests/seeded_cases.run -- (cluster_id, seed_rank, n_clusters, status, merges, C_out) -- without its cap on the seeds and without a
    Python loop over the clusters per merge: the matrix keeps one slot per creation id (list order IS creation order: removal keeps
    the order and the new cluster goes last), a pair lives in the row of its higher id, and each row remembers its first minimum, so
    FindClosestClusters' row-major first minimum is the first row of smallest minimum."""
    from oracle import oracle as O

    C = np.ascontiguousarray(C, np.float32)
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m, d = C.shape
    assert (ss > 0).all(), "no frozen seeds here"
    fail = lambda st: (np.full(m, -1, np.int32), np.full(m, -1, np.int32), 0, st, np.zeros((0, 2), np.int32), np.zeros((m, d), np.float32))
    if (ss > max_size).any():
        return fail(6)  # ICL_ERR_UNSUPPORTED
    if k_target > 0:
        k = int(k_target)
    else:
        k, err = O.calc_optimal_clusters(int(ss.sum()), min_size, max_size)
        if err is not None:
            return fail(2)  # ICL_ERR_CONSTRAINT
    cap = max(m + max(m - k, 0), 1)
    cen, size, alive = np.zeros((cap, d), np.float32), np.zeros(cap, np.int64), np.zeros(cap, bool)
    cen[:m], size[:m], alive[:m] = C, ss, True
    D = np.full((cap, cap), MAXF, np.float32)
    if m:
        D0 = O.initial_distance_matrix(C, ss.astype(np.int32)).copy()
        D0[np.triu_indices(m)] = MAXF
        D[:m, :m] = D0
    rmin, rarg = D.min(axis=1), D.argmin(axis=1)
    seeds, log, live, nxt = {i: [i] for i in range(m)}, [], m, m
    with np.errstate(all="ignore"):
        while live > k:
            i = int(np.argmin(rmin))
            if not rmin[i] < MAXF:
                break
            j = int(rarg[i])
            if size[i] + size[j] > max_size:  # :228-234
                D[i, j] = MAXF
                rmin[i], rarg[i] = D[i].min(), D[i].argmin()
                continue
            new, nxt = nxt, nxt + 1
            sa, sb = size[i], size[j]
            cen[new] = (np.float32(sa) * cen[i] + np.float32(sb) * cen[j]) / np.float32(sa + sb)  # :37-40
            size[new], seeds[new] = sa + sb, seeds.pop(i) + seeds.pop(j)
            log.append((i, j))
            for x in (i, j):
                alive[x], rmin[x] = False, MAXF
                D[x, :] = MAXF
                D[:, x] = MAXF
            for r in np.flatnonzero(alive & ((rarg == i) | (rarg == j))):
                rmin[r], rarg[r] = D[r].min(), D[r].argmin()
            act = np.flatnonzero(alive)
            D[new, act] = _ward_row(cen[act], size[act], cen[new], size[new])  # :76-96
            alive[new] = True
            rmin[new], rarg[new] = D[new].min(), D[new].argmin()
            live -= 1
    cid, rank, C_out, nc = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros((m, d), np.float32), 0
    for c in sorted(seeds):
        C_out[seeds[c][0]] = cen[c]
        if size[c] < min_size:  # :268-271
            continue
        for r, s in enumerate(seeds[c]):
            cid[s], rank[s] = nc, r
        nc += 1
    return cid, rank, nc, 0, np.array(log, np.int32).reshape(-1, 2), C_out


def snapshot(state):
    """Everything a Clustering state holds, comparable with ==: clusters (members, centroid bits, frozen, id), embeddings, apart groups."""
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()
    return ([(list(c.Members), bits(c.Centroid), bool(c.Frozen), int(c.Id)) for c in state.clusters],
            [(k, bits(v)) for k, v in state.embeddings.items()], [list(g) for g in state.apart])
