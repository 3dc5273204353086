"""numpy-float32 restatement of FAST mode (ICL_UPDATE_LW): the DEFINITION the engine's Lance-Williams merge loop is held to, bit for bit.

FAST mode is not comparable with clustering.go (GEMM-form initial distances, Lance-Williams rows instead of centroid recomputes), but it is fully
determined by three rules on the matrix D~ that dist_mfma_kernel produces:

  selection   the reference's: first strict minimum in (row, column) order of creation ids among the pairs of live clusters whose sizes fit
              max_size (a static mask: sizes only grow) and whose value is < MaxFloat32 -- a NaN is never a candidate;
  new row     d(c,x) = ((f32(sa+sx) d(a,x) + f32(sb+sx) d(b,x)) - f32(sx) d(a,b)) / f32(sa+sb+sx), every product, sum, difference and quotient
              rounded to fp32 on its own (ward.hip is compiled with -ffp-contract=off), computed only for the live x with sx + sa + sb <= max_size;
  clamp       every entry, initial or new, that is negative or -0 is +0; a NaN stays a NaN.

Same creation-id formulation as tests/ward_numpy.py: static ids, the merge t creates id n + t, members(c) = members(i) + members(j) for the pick
(i > j).  tests/test_lw_restatement_cpu.py checks this file against the exact oracle and against a literal dictionary version of the rules.
"""
import numpy as np

from tests.ward_numpy import MAXF, calc_k

F = np.float32


def clamp0(v):
    """Negative or -0 -> +0; NaN stays NaN."""
    v = np.asarray(v, F)
    return np.where(v > 0, v, np.where(np.isnan(v), v, F(0))).astype(F)


def lw_row(dax, dbx, dab, sa, sb, sx):
    """ward_lw_value of ward.hip on arrays: each operation is one fp32 rounding, in the kernel's order."""
    sx = np.asarray(sx)
    with np.errstate(all="ignore"):
        p1 = (sa + sx).astype(F) * np.asarray(dax, F)
        p2 = (sb + sx).astype(F) * np.asarray(dbx, F)
        p3 = sx.astype(F) * F(dab)
        v = ((p1 + p2) - p3) / (sa + sb + sx).astype(F)
    return clamp0(v)


def cluster_lw(D0, min_size, max_size):
    """D0: n x n, lower triangle = the RAW initial matrix (the clamp is applied here).  -> (cid, rank, n_clusters, merges[T,2], values[T]) or None."""
    D0 = np.asarray(D0, F)
    n = D0.shape[0]
    k = calc_k(n, min_size, max_size)
    if k is None:
        return None
    T = n - k
    M = n + T
    V = np.full((M, M), np.nan, F)       # stored values, V[i, j] for creation ids i > j
    K = np.full((M, M), np.inf, F)       # the candidates: V where the pair is live, fits max_size and is < MaxFloat32, +inf elsewhere
    size = np.zeros(M, np.int64)
    size[:n] = 1
    live = np.zeros(M, bool)
    live[:n] = True
    members = {i: [i] for i in range(n)}
    V[:n, :n] = clamp0(D0)
    tri = np.tri(n, n, -1, dtype=bool)
    K[:n, :n] = np.where(tri & (2 <= max_size) & (V[:n, :n] < MAXF), V[:n, :n], F(np.inf))
    merges, values = [], []
    for t in range(T):
        flat = int(np.argmin(K))         # row-major first minimum: smallest value, then smallest i, then smallest j
        i, j = divmod(flat, M)
        dab = K[i, j]
        if not dab < MAXF:
            break                        # no mergeable pair is left
        c = n + t
        sa, sb = int(size[i]), int(size[j])
        merges.append((i, j))
        values.append(dab)
        live[i] = live[j] = False
        K[i, :] = K[:, i] = K[j, :] = K[:, j] = np.inf
        xs = np.flatnonzero(live & (size + sa + sb <= max_size))
        size[c] = sa + sb
        members[c] = members.pop(i) + members.pop(j)
        live[c] = True
        if len(xs):
            v = lw_row(V[np.maximum(i, xs), np.minimum(i, xs)], V[np.maximum(j, xs), np.minimum(j, xs)], dab, sa, sb, size[xs])
            V[c, xs] = v
            K[c, xs] = np.where(v < MAXF, v, F(np.inf))
    cid = np.full(n, -1, np.int32)
    rank = np.full(n, -1, np.int32)
    nid = 0
    for c in np.flatnonzero(live):       # live clusters in creation-id order, the ones below min_size dropped
        if size[c] < min_size:
            continue
        for r, m in enumerate(members[int(c)]):
            cid[m] = nid
            rank[m] = r
        nid += 1
    return cid, rank, nid, np.array(merges, np.int32).reshape(-1, 2), np.array(values, F)
