"""numpy-float32 restatement of FAST mode FROM SEEDS (icl_cluster_seeded_fast): the DEFINITION the engine is held to, bit for bit.

tests/lw_numpy.py defines FAST mode on singletons; this file starts the same loop from m seed clusters with sizes of their own:

  admission   icl_cluster_seeded's (ward_seed_admit): N = sum |s|, k = k_target when above 0 else CalculateOptimalClusters(N), T = max(0, m - k)
              merges asked for; a frozen seed (s < 0) has the EFFECTIVE size kmax = max_size clamped to [1, N], every other seed its item count; an
              unfrozen seed above max_size is ICL_ERR_UNSUPPORTED;
  initial     V0(i, j) = clamp0(fl(ward_scale(|s_i|, |s_j|) * fl(2 * D~(i, j)))) for i > j, D~ the stand-alone matrix of icl_distance_mfma_dev on the
              seed centroids and ward_scale = fl(f32(si * sj) / f32(si + sj)) on the REAL item counts (ward_value.h);
  loop        lw_numpy's three rules -- selection, new row, clamp / NaN -- on the effective sizes: a pair whose effective sizes sum above max_size is
              never a candidate (every pair of a frozen seed), a new row is computed only for the live x with sx + sa + sb <= max_size, and the loop
              ends early when no candidate is left;
  final list  ward_final_list with the real item counts: surviving seeds in seed order, then merged clusters in creation order, clusters below
              min_size ITEMS dropped; seed_rank counts seeds, a's before b's;
  C_out       MergeClusters' centroid along the log with the real item counts (centroids_from_log), at the row of each final cluster's rank-0 seed;
              a never-merged seed keeps its input row, every other row is zero.

Not an identity: a run cut after t merges and resumed from its clusters rebuilds V0 from centroids, where the uncut run carried Lance-Williams values
forward.  tests/test_lw_seeded_restatement_cpu.py checks this file; tests/test_seeded_fast_gpu.py holds the engine to it.
"""
import numpy as np

from tests.lw_numpy import clamp0, lw_row
from tests.ward_numpy import MAXF, calc_k

F = np.float32
OK, ERR_CONSTRAINT, ERR_UNSUPPORTED = 0, 2, 6


def ward_scale(si, sj):
    """fl(f32(si * sj) / f32(si + sj)) on arrays of item counts (ward_value.h, ward_scale's factor)."""
    si, sj = np.asarray(si, np.int64), np.asarray(sj, np.int64)
    return ((si * sj).astype(F) / (si + sj).astype(F)).astype(F)


def sized_matrix(D, seed_size):
    """V0 of the docstring for every pair (the full square; callers read i > j) from the stand-alone matrix D~ (lower triangle) and the seed sizes
    (sign ignored).  What icl_distance_mfma_seeded_dev stores."""
    D = np.asarray(D, F)
    it = np.abs(np.asarray(seed_size, np.int64).reshape(-1))
    with np.errstate(all="ignore"):
        return clamp0(ward_scale(it[:, None], it[None, :]) * (F(2) * D).astype(F))


def admit(seed_size, min_size, max_size, k_target=0):
    """ward_seed_admit -> (status, N, k, kmax, eff); eff is None for a refused problem."""
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    N = int(np.abs(ss).sum())
    if N >= 1 << 30 or (ss > max_size).any():
        return ERR_UNSUPPORTED, N, 0, 1, None
    if k_target > 0:
        k = int(k_target)
    else:
        k = calc_k(N, min_size, max_size)
        if k is None:
            return ERR_CONSTRAINT, N, 0, 1, None
    kmax = min(max(int(max_size), 1), max(N, 1))
    return OK, N, k, kmax, np.where(ss < 0, kmax, ss).astype(np.int64)


def final_list(seed_size, min_size, log):
    """ward_final_list with real item counts -> (cluster_id[m], seed_rank[m], n_clusters, finals); finals: (creation id, seed sequence, items) per
    final cluster in list order, dropped ones included."""
    ss = np.abs(np.asarray(seed_size, np.int64).reshape(-1))
    m = len(ss)
    seq = {i: [i] for i in range(m)}
    items = {i: int(ss[i]) for i in range(m)}
    for t, (a, b) in enumerate(np.asarray(log).reshape(-1, 2)):
        seq[m + t] = seq.pop(int(a)) + seq.pop(int(b))
        items[m + t] = items.pop(int(a)) + items.pop(int(b))
    cid, rank, nc, finals = np.full(m, -1, np.int32), np.full(m, -1, np.int32), 0, []
    for c in sorted(seq):
        finals.append((c, seq[c], items[c]))
        if items[c] < min_size:
            continue
        for r, s in enumerate(seq[c]):
            cid[s], rank[s] = nc, r
        nc += 1
    return cid, rank, nc, finals


def merge_centroid(ca, sa, cb, sb):
    """ward_merge_elem on rows: fl(fl(fl(f32(sa) a) + fl(f32(sb) b)) / f32(sa + sb))."""
    with np.errstate(all="ignore"):
        pa = (F(sa) * np.asarray(ca, F)).astype(F)
        pb = (F(sb) * np.asarray(cb, F)).astype(F)
        return ((pa + pb).astype(F) / F(sa + sb)).astype(F)


def centroids_from_log(C, seed_size, log):
    """C_out of a call with this log (the docstring's rule)."""
    C = np.ascontiguousarray(C, F)
    ss = np.abs(np.asarray(seed_size, np.int64).reshape(-1))
    m = len(ss)
    cen = {i: C[i] for i in range(m)}
    items = {i: int(ss[i]) for i in range(m)}
    first = {i: i for i in range(m)}
    for t, (a, b) in enumerate(np.asarray(log).reshape(-1, 2)):
        a, b = int(a), int(b)
        cen[m + t] = merge_centroid(cen[a], items[a], cen[b], items[b])
        items[m + t] = items[a] + items[b]
        first[m + t] = first[a]
        for q in (a, b):
            del cen[q], items[q], first[q]
    out = np.zeros_like(C)
    for c in cen:
        out[first[c]] = cen[c]
    return out


def cluster_lw_seeded(D, seed_size, min_size, max_size, k_target=0):
    """D: m x m, lower triangle = icl_distance_mfma_dev's matrix of the seed centroids.  -> dict(status, cluster_id, seed_rank, n_clusters, log[T, 2],
    values[T]); a refused problem has rows of -1 and an empty log."""
    ss = np.asarray(seed_size, np.int64).reshape(-1)
    m = len(ss)
    assert (ss != 0).all() and np.asarray(D).shape == (m, m)
    status, N, k, kmax, eff = admit(ss, min_size, max_size, k_target)
    if status != OK:
        return dict(status=status, cluster_id=np.full(m, -1, np.int32), seed_rank=np.full(m, -1, np.int32), n_clusters=0,
                    log=np.zeros((0, 2), np.int32), values=np.zeros(0, F))
    T = max(0, m - k)
    M = m + T
    V = np.full((M, M), np.nan, F)   # stored values, V[i, j] for creation ids i > j
    K = np.full((M, M), np.inf, F)   # the candidates: V where the pair is live, fits kmax and is < MaxFloat32, +inf elsewhere
    size = np.zeros(M, np.int64)     # EFFECTIVE sizes
    size[:m] = eff
    live = np.zeros(M, bool)
    live[:m] = True
    V[:m, :m] = sized_matrix(D, ss)
    fits = (size[:m, None] + size[None, :m]) <= kmax
    K[:m, :m] = np.where(np.tri(m, m, -1, dtype=bool) & fits & (V[:m, :m] < MAXF), V[:m, :m], F(np.inf))
    log, values = [], []
    for t in range(T):
        flat = int(np.argmin(K))     # row-major first minimum: smallest value, then smallest i, then smallest j
        i, j = divmod(flat, M)
        dab = K[i, j]
        if not dab < MAXF:
            break                    # no mergeable pair is left
        c = m + t
        sa, sb = int(size[i]), int(size[j])
        log.append((i, j))
        values.append(dab)
        live[i] = live[j] = False
        K[i, :] = K[:, i] = K[j, :] = K[:, j] = np.inf
        xs = np.flatnonzero(live & (size + sa + sb <= kmax))
        size[c] = sa + sb
        live[c] = True
        if len(xs):
            v = lw_row(V[np.maximum(i, xs), np.minimum(i, xs)], V[np.maximum(j, xs), np.minimum(j, xs)], dab, sa, sb, size[xs])
            V[c, xs] = v
            K[c, xs] = np.where(v < MAXF, v, F(np.inf))
    log = np.array(log, np.int32).reshape(-1, 2)
    cid, rank, nc, _ = final_list(ss, min_size, log)
    return dict(status=OK, cluster_id=cid, seed_rank=rank, n_clusters=nc, log=log, values=np.array(values, F))
