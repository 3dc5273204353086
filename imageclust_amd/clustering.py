"""Host-side mirror of /root/reference/internal/clustering/clustering.go over the HIP engine.

Same exported names, argument meaning and error behaviour as the Go package, so the parity tests read like
tests of the reference.  Every arithmetic result comes from libimageclust_hip.so through its C-ABI
(include/imageclust.h); the functions that only re-arrange lists (NewCluster, RemoveClusters,
RemoveRowsAndColumns) are plain data-structure code exactly as in the Go file.  There is no CPU fallback:
without the built library (or without a gfx950 device) these functions raise.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib

_default_ctx: Optional[_lib.Context] = None


def default_context() -> _lib.Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = _lib.Context(0)
    return _default_ctx


def set_default_context(ctx: Optional[_lib.Context]):
    global _default_ctx
    _default_ctx = ctx


@dataclass
class Cluster:
    """clustering.go:11-15"""
    Indices: List[int] = field(default_factory=list)
    Size: int = 0
    Centroid: np.ndarray = None


def NewCluster(index: int, embedding) -> Cluster:
    """clustering.go:18-26: singleton with a COPY of the embedding."""
    return Cluster(Indices=[int(index)], Size=1, Centroid=np.array(embedding, dtype=np.float32, copy=True))


def MergeClusters(a: Cluster, b: Cluster, ctx: Optional[_lib.Context] = None) -> Cluster:
    """clustering.go:29-47: members a++b, centroid (float(sa)*Ca + float(sb)*Cb)/float(sa+sb) on the GPU."""
    ctx = ctx or default_context()
    return Cluster(Indices=list(a.Indices) + list(b.Indices), Size=a.Size + b.Size,
                   Centroid=ctx.merge_centroid(a.Centroid, a.Size, b.Centroid, b.Size))


def RemoveClusters(clusters: List[Cluster], i: int, j: int) -> List[Cluster]:
    """clustering.go:51-58: order-preserving removal of positions i and j."""
    if i > j:
        i, j = j, i
    return clusters[:i] + clusters[i + 1:j] + clusters[j + 1:]


def ComputeInitialDistanceMatrix(clusters: List[Cluster], ctx: Optional[_lib.Context] = None) -> np.ndarray:
    """clustering.go:61-73 -> n x n fp32, symmetric, zero diagonal (exact Ward tile kernel)."""
    ctx = ctx or default_context()
    n = len(clusters)
    if n == 0:
        return np.zeros((0, 0), np.float32)
    C = np.stack([np.asarray(c.Centroid, np.float32) for c in clusters])
    sizes = np.array([c.Size for c in clusters], np.int32)
    return ctx.ward_distance_matrix(C, sizes)


def RemoveRowsAndColumns(matrix: np.ndarray, i: int, j: int) -> np.ndarray:
    """clustering.go:100-116"""
    keep = [k for k in range(matrix.shape[0]) if k != i and k != j]
    return matrix[np.ix_(keep, keep)]


def WardDistance(a: Cluster, b: Cluster, ctx: Optional[_lib.Context] = None) -> np.float32:
    """clustering.go:136-145 for one pair (a 2x2 call of the distance tile)."""
    return ComputeInitialDistanceMatrix([a, b], ctx)[1, 0]


def UpdateDistanceMatrix(distanceMatrix: np.ndarray, clusters: List[Cluster], newCluster: Cluster, removedIdx1: int,
                         removedIdx2: int, ctx: Optional[_lib.Context] = None) -> np.ndarray:
    """clustering.go:76-96: drop two rows/columns, append the new cluster's row/column computed from centroids
    (icl_update_distance_matrix).  `clusters` is the list AFTER removal and append (newCluster last), as at
    clustering.go:244; newCluster is accepted for signature parity and must be clusters[-1]."""
    ctx = ctx or default_context()
    C = np.stack([np.asarray(c.Centroid, np.float32) for c in clusters])
    sizes = np.array([c.Size for c in clusters], np.int32)
    return ctx.update_distance_matrix(np.asarray(distanceMatrix, np.float32), C, sizes, removedIdx1, removedIdx2)


def DotFloat32(a, b) -> np.float32:
    """clustering.go:148-157: in-order fp32 dot product, product rounded then sum rounded; panics on length mismatch."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    if a.shape != b.shape:
        raise ValueError("vectors must be the same length")  # clustering.go:150 panics
    s = np.float32(0)
    for p in (a * b).astype(np.float32):
        s = np.float32(s + p)
    return s


def FindClosestClusters(distanceMatrix, ctx: Optional[_lib.Context] = None) -> Tuple[int, int]:
    """clustering.go:119-133 -> (i, j) with i > j, or (-1, -1)."""
    ctx = ctx or default_context()
    D = np.asarray(distanceMatrix, np.float32)
    if D.ndim != 2 or D.shape[0] == 0:
        return -1, -1
    return ctx.find_closest(D)


def CalculateOptimalClusters(totalItems: int, minSize: int, maxSize: int):
    """clustering.go:168-186 -> (nClusters, err) with err None on success."""
    k, rc = _lib.calc_optimal_clusters(totalItems, minSize, maxSize)
    if rc is not None:
        if totalItems < minSize:
            return 0, "total items (%d) less than minimum cluster size (%d)" % (totalItems, minSize)
        return 0, ("cannot satisfy cluster size constraints with total items (%d), minSize (%d), and maxSize (%d)"
                   % (totalItems, minSize, maxSize))
    return k, None


def PerformClusteringWithConstraints(embeddings, productReferenceIDs: List[str], minSize: int, maxSize: int,
                                     ctx: Optional[_lib.Context] = None,
                                     update: int = _lib.UPDATE_EXACT) -> Tuple[Optional[Dict[int, List[str]]], bool]:
    """clustering.go:198-284 -> (map cluster id -> member ids, ok).  (None, False) on impossible constraints."""
    ctx = ctx or default_context()
    E = np.asarray(embeddings, np.float32)
    if E.ndim != 2:
        E = E.reshape(len(embeddings), -1)
    try:
        cid, rank, _ = ctx.cluster(E, minSize, maxSize, update)
    except _lib.ICLError as e:
        if e.code == _lib.ICL_ERR_CONSTRAINT:
            return None, False
        raise
    return clusters_as_map(cid, rank, productReferenceIDs), True


def PerformClusteringWithConstraintsMany(jobs, ctx: Optional[_lib.Context] = None) -> List[Tuple[Optional[Dict[int, List[str]]], bool]]:
    """Many PerformClusteringWithConstraints calls in one (icl_cluster_many, exact mode): jobs = [(embeddings, productReferenceIDs,
    minSize, maxSize), ...] -> [(map, ok), ...], each entry what PerformClusteringWithConstraints returns for that job."""
    ctx = ctx or default_context()
    probs = []
    for emb, _, mn, mx in jobs:
        E = np.asarray(emb, np.float32)
        if E.ndim != 2:
            E = E.reshape(len(emb), -1)
        probs.append((E, mn, mx))
    out = []
    for (_, ids, _, _), (cid, rank, _, st) in zip(jobs, ctx.cluster_many(probs)):
        if st == _lib.ICL_ERR_CONSTRAINT:
            out.append((None, False))
        elif st != _lib.ICL_OK:
            raise _lib.ICLError(st, "icl_cluster_many: a problem failed with code %d" % st)
        else:
            out.append((clusters_as_map(cid, rank, ids), True))
    return out


MANY_SEEDED_MAX = 2048  # icl_cluster_many_seeded's cap on a problem's seeds; above it the seeded call of the large-N engine runs


def _constrained(apart_class, apart_pairs) -> bool:
    """Whether the two optional lists hold a constraint at all."""
    return (apart_class is not None and bool(np.asarray(apart_class).any())) or (apart_pairs is not None and len(apart_pairs) > 0)


def _seeded_call(ctx, C, sizes, minSize, maxSize, k_target, apart_class=None, apart_pairs=None, update: int = _lib.UPDATE_EXACT):
    """One seeded problem -> (cluster_id, seed_rank, n_clusters, status, merges, C_out): icl_cluster_many_seeded up to its cap,
    icl_cluster_seeded (ward.hip's exact pipeline, no cap) above.  With a keep-apart constraint: icl_cluster_many_apart up to the same
    cap, icl_cluster_apart (ward.hip's one-merge-per-step exact loop, no cap) above -- ICLError(ICL_ERR_UNSUPPORTED) where the handle
    has no such call.  An unconstrained problem never takes a constrained call, whatever the two cost.  update=UPDATE_LW (FAST mode):
    icl_cluster_seeded_fast at every seed count -- ward_many.hip has no FAST route --, and a constraint raises ICLError(ICL_ERR_UNSUPPORTED)."""
    if update == _lib.UPDATE_LW:
        if _constrained(apart_class, apart_pairs):
            raise _lib.ICLError(_lib.ICL_ERR_UNSUPPORTED, "FAST mode (UPDATE_LW) keeps no keep-apart constraints")
        return ctx.cluster_seeded(C, sizes, minSize, maxSize, k_target, want_centroids=True, update=_lib.UPDATE_LW)
    if _constrained(apart_class, apart_pairs):
        if len(sizes) > MANY_SEEDED_MAX:
            large = getattr(ctx, "cluster_apart", None)
            if large is None:  # a handle without the large-N constrained call (a _lib.Group: group contexts are not covered)
                raise _lib.ICLError(_lib.ICL_ERR_UNSUPPORTED, "%d seeds with keep-apart constraints: icl_cluster_many_apart holds at most %d and "
                                    "this handle has no icl_cluster_apart" % (len(sizes), MANY_SEEDED_MAX))
            return large(C, sizes, minSize, maxSize, k_target, apart_class, apart_pairs, want_centroids=True)
        return ctx.cluster_many_apart([(C, sizes, minSize, maxSize, k_target, apart_class, apart_pairs)], want_merges=True, want_centroids=True)[0]
    if len(sizes) > MANY_SEEDED_MAX:
        return ctx.cluster_seeded(C, sizes, minSize, maxSize, k_target, want_centroids=True)
    return ctx.cluster_many_seeded([(C, sizes, minSize, maxSize, k_target)], want_merges=True, want_centroids=True)[0]


def PerformClusteringSeeded(centroids, sizes, minSize: int, maxSize: int, k_target: int = 0, ctx: Optional[_lib.Context] = None,
                            apart_pairs=None, apart_class=None, update: int = _lib.UPDATE_EXACT):
    """The loop of clustering.go:216-246 started from existing clusters (icl_cluster_many_seeded, one problem; icl_cluster_seeded above
    2 048 seeds): centroids[i] and
    sizes[i] describe seed cluster i, a negative size a frozen one that is never merged; k_target > 0 is the number of clusters to stop
    at, else CalculateOptimalClusters of the item total decides -> ((cluster_id, seed_rank, n_clusters, merges, C_out), True) at seed
    granularity -- C_out[i] is the centroid of the final cluster whose first seed is i, zero for every other seed -- or (None, False)
    on impossible constraints.  apart_pairs ((i, j) seed indices) and apart_class (one int per seed, 0: none; the seeds of one non-zero
    class) name seeds that must never share a cluster (icl_cluster_many_apart: a merged cluster inherits the bans of both parents;
    icl_cluster_apart above 2 048 seeds); the loop may then end before k clusters are reached.  update=UPDATE_LW runs the problem in
    FAST mode (icl_cluster_seeded_fast, any seed count; DESIGN.md "Seeded clustering in FAST mode"): the default is the exact pipeline."""
    ctx = ctx or default_context()
    C = np.asarray(centroids, np.float32)
    if C.ndim != 2:
        C = C.reshape(len(sizes), -1)
    cid, rank, nc, st, mg, co = _seeded_call(ctx, C, sizes, minSize, maxSize, k_target, apart_class, apart_pairs, update)
    if st == _lib.ICL_ERR_CONSTRAINT:
        return None, False
    if st != _lib.ICL_OK:
        raise _lib.ICLError(st, ctx.last_error())
    return (cid, rank, nc, mg, co), True


def NearestClusters(queries, q_sizes, centroids, sizes, k: int, maxSize: int = 0, ctx: Optional[_lib.Context] = None):
    """For each query cluster (centroid queries[i], q_sizes[i] items; None: singletons) the up to k clusters of (centroids, sizes) that are
    closest in the loop's own cost (icl_nearest): WardDistance of clustering.go:136-157 bit for bit, ascending by (value, index).  maxSize > 0
    leaves out the pairs the loop would ban (:228) -> (idx int32[nq][k], val float32[nq][k]); a short row ends in idx -1, val MaxFloat32."""
    ctx = ctx or default_context()
    return ctx.nearest(queries, centroids, k, q_size=q_sizes, e_size=sizes, max_size=maxSize)


def ClusterFit(queries, q_sizes, cluster_of, centroids, sizes, k: int = 1, maxSize: int = 0, ctx: Optional[_lib.Context] = None):
    """For each clustered row (centroid queries[i], q_sizes[i] items; None: singletons) its cost against its own cluster cluster_of[i] of
    (centroids, sizes) and the up to k other clusters that would take it (icl_cluster_fit): WardDistance of clustering.go:136-157 bit for
    bit throughout.  A negative size is a frozen cluster: measured as an own cluster, never offered; maxSize > 0 leaves out the pairs the
    loop would ban (:228) -> dict(own, alt_idx, alt_val, listed, rep, worst), as Context.cluster_fit."""
    ctx = ctx or default_context()
    return ctx.cluster_fit(queries, cluster_of, centroids, k, q_size=q_sizes, c_size=sizes, max_size=maxSize)


def FoldCentroids(embeddings, groups, sizes=None, ctx: Optional[_lib.Context] = None):
    """The centroid of each cluster given as a list of row indices (icl_fold_centroids): what the reference holds after merging the
    listed rows one at a time in list order (MergeClusters, clustering.go:29-47, bit for bit; sizes: the rows' item counts, None:
    singletons) -> (centroids float32[len(groups)][d], item totals int32[len(groups)]).  An empty list gives a row of +0.0 and 0."""
    ctx = ctx or default_context()
    E = np.asarray(embeddings, np.float32)
    if E.ndim != 2:
        E = E.reshape(len(embeddings), -1)
    row_ptr, member = _lib.groups_as_csr(groups)
    return ctx.fold_centroids(E, row_ptr, member, size=sizes)


def _final_seed_lists(m: int, merges) -> List[List[int]]:
    """The final list of a seeded run over m seeds from its merge log, each cluster as its seed sequence: surviving seeds in seed order,
    then merged clusters in creation order, a's seeds before b's."""
    seq = {i: [i] for i in range(m)}
    for t, (a, b) in enumerate(np.asarray(merges).reshape(-1, 2)):
        seq[m + t] = seq.pop(int(a)) + seq.pop(int(b))
    return [seq[c] for c in sorted(seq)]


def NearDuplicates(embeddings, ids, k: int, threshold: float, ctx: Optional[_lib.Context] = None) -> List[Tuple[str, str, float]]:
    """Pairs of images whose WardDistance as singletons is at most threshold, from a self-join of the embeddings (icl_nearest with
    exclude[i] = i, the k nearest of every image) -> [(id_a, id_b, value), ...], a before b in `ids`, each pair once, ordered by position.
    An image with more than k neighbours under the threshold reports its k nearest; a pair is reported when either side lists it.
    DuplicatePairs is the complete call: every pair under the threshold, however many partners an image has."""
    ctx = ctx or default_context()
    E = np.asarray(embeddings, np.float32)
    if E.ndim != 2:
        E = E.reshape(len(ids), -1)
    if len(E) != len(ids):
        raise ValueError("%d embeddings for %d ids" % (len(E), len(ids)))
    if len(E) == 0:
        return []
    idx, val = ctx.nearest(E, E, k, exclude=np.arange(len(E), dtype=np.int64))
    found: Dict[Tuple[int, int], float] = {}
    for i in range(len(E)):
        for j, v in zip(idx[i], val[i]):
            if j >= 0 and v <= threshold:  # (NaN fails the comparison)
                found.setdefault((min(i, int(j)), max(i, int(j))), float(v))
    return [(ids[a], ids[b], v) for (a, b), v in sorted(found.items())]


def _pairs_csr(embeddings, ids, threshold, ctx, engine):
    """The embeddings as a matrix and their complete pair list (icl_pairs_within; `engine(E, threshold) -> (row_ptr, col, val)` stands in
    for the GPU call in tests)."""
    E = np.asarray(embeddings, np.float32)
    if E.ndim != 2:
        E = E.reshape(len(ids), -1)
    if len(E) != len(ids):
        raise ValueError("%d embeddings for %d ids" % (len(E), len(ids)))
    if len(E) == 0:
        return E, (np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    if engine is not None:
        return E, engine(E, threshold)
    return E, (ctx or default_context()).pairs_within(E, threshold)


def DuplicatePairs(embeddings, ids, threshold: float, ctx: Optional[_lib.Context] = None, engine=None) -> List[Tuple[str, str, float]]:
    """EVERY pair of images whose WardDistance as singletons is at most threshold (icl_pairs_within: exact values, no cap on an image's
    partners, no distance matrix) -> [(id_a, id_b, value), ...], a before b in `ids`, each pair once, ordered by position: NearDuplicates'
    shape, but complete.  NaN values are never reported."""
    _, (row_ptr, col, val) = _pairs_csr(embeddings, ids, threshold, ctx, engine)
    found = []
    for i in range(len(row_ptr) - 1):
        for p in range(int(row_ptr[i]), int(row_ptr[i + 1])):
            found.append((int(col[p]), i, float(val[p])))
    found.sort(key=lambda t: (t[0], t[1]))
    return [(ids[a], ids[b], v) for a, b, v in found]


def DuplicateGroups(embeddings, ids, threshold: float, ctx: Optional[_lib.Context] = None, engine=None) -> List[List[str]]:
    """The connected components of DuplicatePairs' graph with at least two members (icl_pair_groups) -> [[id, ...], ...]: members in
    position order, groups ordered by their first member."""
    _, (row_ptr, col, _) = _pairs_csr(embeddings, ids, threshold, ctx, engine)
    group, _ = _lib.pair_groups(row_ptr, col)
    members: Dict[int, List[str]] = {}
    for i, g in enumerate(group):
        members.setdefault(int(g), []).append(ids[i])
    return [m for _, m in sorted(members.items()) if len(m) >= 2]


def _rows_of(embeddings, ids):
    E = np.asarray(embeddings, np.float32)
    if E.ndim != 2:
        E = E.reshape(len(ids), -1)
    if len(E) != len(ids):
        raise ValueError("%d embeddings for %d ids" % (len(E), len(ids)))
    return E


def _between_csr(Q, L, threshold, ctx, engine):
    """The complete pair list of the rows of Q against the rows of L (icl_pairs_between; `engine(Q, L, threshold) -> (row_ptr, col, val)`
    stands in for the GPU call in tests)."""
    if len(Q) == 0 or len(L) == 0:
        return np.zeros(len(Q) + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if engine is not None:
        return engine(Q, L, threshold)
    return (ctx or default_context()).pairs_between(Q, L, threshold)


def DuplicatesOf(new_embeddings, new_ids, embeddings, ids, threshold: float, ctx: Optional[_lib.Context] = None,
                 engine=None) -> List[Tuple[str, str, float]]:
    """EVERY pair (new image, held image) whose WardDistance as singletons is at most threshold (icl_pairs_between: exact values, no cap
    on an image's partners, no distance matrix, the held images never compared with each other) -> [(new_id, id, value), ...], ordered
    by the new image's position and then by the held image's.  NaN values are never reported."""
    Q, L = _rows_of(new_embeddings, new_ids), _rows_of(embeddings, ids)
    row_ptr, col, val = _between_csr(Q, L, threshold, ctx, engine)
    return [(new_ids[i], ids[int(col[p])], float(val[p])) for i in range(len(Q)) for p in range(int(row_ptr[i]), int(row_ptr[i + 1]))]


@dataclass
class HeldCluster:
    """A cluster a Clustering state holds between calls: member ids in the reference's order, the centroid as the loop left it (after
    an edit: the fold of MergeClusters over the members in list order), the frozen flag, and its id in as_map() (-1: below minSize, so the reference's report drops it -- the state keeps it)."""
    Members: List[str]
    Centroid: np.ndarray
    Frozen: bool = False
    Id: int = -1


class Clustering:
    """A clustering that can go on: the final clusters of a run -- the dropped ones included -- are kept with sizes and centroids, and
    recluster() resumes the reference's loop from them (DESIGN.md "Seeded clustering").  Keys name clusters by any of their members' ids.

        state = Clustering.start(embeddings, ids, 3, 6)     # what PerformClusteringWithConstraints computes, kept
        state.add(more_embeddings, more_ids)                # new images join as singletons
        state.freeze(["img_4"])                             # the cluster holding img_4 stays as it is
        state.keep_apart(["img_1", "img_9"])                # these two never share a cluster again (DESIGN.md "Constrained seeded clustering")
        state.recluster()
        state.absorb_leftovers()                            # the images of dropped clusters join the kept clusters where they may
        state.as_map()

    `engine` replaces the GPU call in tests: engine(C, seed_size, minSize, maxSize, k_target) -> (cluster_id, seed_rank, n_clusters,
    status, merges, C_out), called with two more arguments, (..., apart_class, apart_pairs), only when a constraint exists; `nearest_engine` likewise for nearest(): nearest_engine(Q, E, k, q_size, e_size, max_size) -> (idx, val); and
    `fit_engine` for fit(), representatives() and misfits(): fit_engine(Q, cluster_of, C, k_alt, q_size, c_size, max_size) -> the dict of
    Context.cluster_fit; `between_engine` and `pairs_engine` for duplicates_of() and add(skip_duplicates=): between_engine(Q, L, threshold)
    and pairs_engine(E, threshold) -> (row_ptr, col, val), as Context.pairs_between and Context.pairs_within; `fold_engine` for the edits
    below: fold_engine(E, row_ptr, member, size) -> (C, size_out), as Context.fold_centroids.

    A held clustering can be edited (DESIGN.md "Editing a held clustering"): remove(ids) deletes images, move(ids, to_key) puts images
    into another cluster, Clustering.from_partition(...) adopts a partition computed elsewhere, oversized() lists the clusters above
    maxSize and split(keys) divides clusters with the state's own engine.  An edited cluster's centroid is the fold of MergeClusters over
    its members in list order (icl_fold_centroids); a cluster no edit touched keeps the centroid the loop left it, so a state may hold
    both kinds.

    update=UPDATE_LW keeps the state in FAST mode: every recluster() is icl_cluster_seeded_fast, whatever the number of clusters held, and a
    state with keep_apart constraints raises ICLError(ICL_ERR_UNSUPPORTED) there.  A FAST state cut and resumed is not the uncut FAST run."""

    def __init__(self, minSize: int, maxSize: int, ctx: Optional[_lib.Context] = None, engine=None, nearest_engine=None, fit_engine=None,
                 between_engine=None, pairs_engine=None, update: int = _lib.UPDATE_EXACT, fold_engine=None):
        self.minSize, self.maxSize = int(minSize), int(maxSize)
        self.update = int(update)
        self.ctx, self.engine, self.nearest_engine, self.fit_engine = ctx, engine, nearest_engine, fit_engine
        self.between_engine, self.pairs_engine, self.fold_engine = between_engine, pairs_engine, fold_engine
        self.clusters: List[HeldCluster] = []
        self.embeddings: Dict[str, np.ndarray] = {}
        self.ok = True
        self.last_merges = np.zeros((0, 2), np.int32)
        self.apart: List[List[str]] = []  # keep_apart's groups of image ids: the clusters holding the ids of one group are mutually apart

    @classmethod
    def start(cls, embeddings, ids, minSize: int, maxSize: int, ctx: Optional[_lib.Context] = None, engine=None, nearest_engine=None,
              fit_engine=None, between_engine=None, pairs_engine=None, update: int = _lib.UPDATE_EXACT, fold_engine=None) -> "Clustering":
        """A seeded run from singletons: the clusters of PerformClusteringWithConstraints(embeddings, ids, minSize, maxSize); .ok is
        False (and every image is still a singleton) when the constraints cannot be met."""
        state = cls(minSize, maxSize, ctx, engine, nearest_engine, fit_engine, between_engine, pairs_engine, update, fold_engine)
        state.add(embeddings, ids)
        state.recluster()
        return state

    @classmethod
    def from_partition(cls, embeddings, ids, groups, minSize: int, maxSize: int, ctx: Optional[_lib.Context] = None, engine=None,
                       nearest_engine=None, fit_engine=None, between_engine=None, pairs_engine=None, update: int = _lib.UPDATE_EXACT,
                       fold_engine=None) -> "Clustering":
        """A state from a partition it did not compute (a user's albums, a clustering saved as id lists): `groups` is a list of
        non-empty id lists, each id at most once; the ids in no group follow as singletons, in `ids` order.  No clustering runs: every
        centroid is the fold of MergeClusters over the cluster's members in list order (one icl_fold_centroids call; a one-member
        cluster holds its row's bits).  A group above maxSize is held as it is -- oversized() lists it, split() divides it, and
        recluster() refuses the state while it is there.  ValueError for an empty group, an unknown id or an id listed twice."""
        ids = list(ids)
        E = _rows_of(embeddings, ids)
        at = {k: i for i, k in enumerate(ids)}
        if len(at) != len(ids):
            raise ValueError("from_partition: an id is listed twice")
        groups = [list(g) for g in groups]
        seen = set()
        for g in groups:
            if not g:
                raise ValueError("from_partition: an empty group")
            for k in g:
                if k not in at or k in seen:
                    raise ValueError("from_partition: id %r is %s" % (k, "in two groups or twice in one" if k in at else "unknown"))
                seen.add(k)
        lists = groups + [[k] for k in ids if k not in seen]
        state = cls(minSize, maxSize, ctx, engine, nearest_engine, fit_engine, between_engine, pairs_engine, update, fold_engine)
        C = state._fold_rows(E, [[at[k] for k in g] for g in lists])
        state.embeddings = {k: np.array(E[i], np.float32, copy=True) for i, k in enumerate(ids)}
        state.clusters = [HeldCluster(g, np.array(C[j], np.float32, copy=True)) for j, g in enumerate(lists)]
        state._renumber()
        return state

    def _fold_rows(self, E, groups) -> np.ndarray:
        """The centroids of the clusters given as lists of rows of E, singletons throughout (icl_fold_centroids; `fold_engine(E, row_ptr,
        member, size) -> (C, size_out)` stands in for the GPU call in tests)."""
        row_ptr, member = _lib.groups_as_csr(groups)
        if self.fold_engine is not None:
            return np.asarray(self.fold_engine(E, row_ptr, member, None)[0], np.float32)
        return (self.ctx or default_context()).fold_centroids(E, row_ptr, member)[0]

    def _fold_members(self, lists: List[List[str]]) -> List[np.ndarray]:
        """The centroids of clusters given as member id lists, all in one fold call over the rows they name."""
        if not lists:
            return []
        rows = list(dict.fromkeys(k for g in lists for k in g))
        at = {k: i for i, k in enumerate(rows)}
        E = np.stack([self.embeddings[k] for k in rows]).astype(np.float32)
        C = self._fold_rows(E, [[at[k] for k in g] for g in lists])
        return [np.array(C[j], np.float32, copy=True) for j in range(len(lists))]

    def _renumber(self):
        """The report's ids (clustering.go:265-280; keep_together's rule): dense over the clusters of at least minSize items, in held
        order, -1 otherwise."""
        kept = 0
        for c in self.clusters:
            c.Id = -1
            if len(c.Members) >= self.minSize:
                c.Id, kept = kept, kept + 1

    def _where(self, keys, what: str) -> Dict[str, int]:
        """id -> position of its cluster, after checking that every key is held and listed once (ValueError otherwise)."""
        where = {k: i for i, c in enumerate(self.clusters) for k in c.Members}
        seen = set()
        for k in keys:
            if k not in where or k in seen:
                raise ValueError("%s: id %r is %s" % (what, k, "listed twice" if k in where else "not held"))
            seen.add(k)
        return where

    def remove(self, ids):
        """The images leave the state: embeddings, member lists and the keep_apart groups (a group left with fewer than two ids is
        dropped).  A cluster that lost members gets the fold of MergeClusters over what remains, as singletons in member order (all
        rebuilt clusters in one icl_fold_centroids call); an emptied cluster disappears; a frozen cluster stays frozen.  ValueError,
        with the state as it was, for an id that is not held or is listed twice."""
        ids = list(ids)
        where = self._where(ids, "remove")
        gone, touched = set(ids), sorted({where[k] for k in ids})
        left = {i: [k for k in self.clusters[i].Members if k not in gone] for i in touched}
        rebuilt = [i for i in touched if left[i]]
        cen = dict(zip(rebuilt, self._fold_members([left[i] for i in rebuilt])))
        held = []
        for i, c in enumerate(self.clusters):
            if i not in left:
                held.append(c)
            elif left[i]:
                held.append(HeldCluster(left[i], cen[i], c.Frozen))
        self.clusters = held
        for k in ids:
            del self.embeddings[k]
        self.apart = [g for g in ([k for k in grp if k not in gone] for grp in self.apart) if len(g) >= 2]
        self._renumber()

    def move(self, ids, to_key=None):
        """The images change cluster: all are taken out first, then appended, in the order given, to the cluster holding to_key; with
        to_key=None each becomes a singleton at the end, its centroid a copy of its embedding (as add() leaves it).  Every cluster that
        lost or gained members gets the fold of MergeClusters over its new member list (one icl_fold_centroids call); a cluster left
        empty disappears.  ValueError, with the state as it was, when an id is not held or listed twice, an id is already in the
        target, a source or the target is frozen, the target would exceed maxSize, or two ids of one keep_apart group would share it."""
        ids = list(ids)
        where = self._where(ids, "move")
        target = None
        if to_key is not None:
            if to_key not in where:
                raise ValueError("move: id %r is not held" % (to_key,))
            target = where[to_key]
            if self.clusters[target].Frozen:
                raise ValueError("move: the target cluster is frozen")
            if any(where[k] == target for k in ids):
                raise ValueError("move: an id is already in the target cluster")
        if any(self.clusters[where[k]].Frozen for k in ids):
            raise ValueError("move: a source cluster is frozen")
        if not ids:
            return  # nobody moves: the target keeps the centroid it holds
        gone, touched = set(ids), sorted({where[k] for k in ids})
        left = {i: [k for k in self.clusters[i].Members if k not in gone] for i in touched}
        if target is not None:
            left[target] = list(self.clusters[target].Members) + ids
            if len(left[target]) > self.maxSize:
                raise ValueError("move: %d items, above maxSize (%d)" % (len(left[target]), self.maxSize))
            inside = set(left[target])
            if any(sum(k in inside for k in grp) >= 2 for grp in self.apart):
                raise ValueError("move: a keep-apart constraint holds between two of these images")
        rebuilt = [i for i in sorted(left) if left[i]]
        cen = dict(zip(rebuilt, self._fold_members([left[i] for i in rebuilt])))
        held = []
        for i, c in enumerate(self.clusters):
            if i not in left:
                held.append(c)
            elif left[i]:
                held.append(HeldCluster(left[i], cen[i], c.Frozen))
        if target is None:
            held += [HeldCluster([k], self.embeddings[k].copy()) for k in ids]
        self.clusters = held
        self._renumber()

    def oversized(self) -> List[str]:
        """The clusters above maxSize (from_partition may hold some), by their first members' ids.  recluster() raises
        ICLError(ICL_ERR_UNSUPPORTED) while there is one; split() divides them."""
        return [c.Members[0] for c in self.clusters if len(c.Members) > self.maxSize]

    def split(self, keys, k_target: int = 0):
        """Each unfrozen cluster of at least 2 members holding one of these ids is divided, in held order: the state's own engine and mode
        run the reference's loop on the members' embeddings alone -- singletons, minSize 1, the state's maxSize, no constraints -- and the
        parts (the sub-run's final list: a's members before b's, centroids as the loop left them) take the cluster's place, unfrozen.
        This is the reference's splitCluster (clustering.go:295-349) made reachable.  k_target = 0 stops where it does, at
        CalculateOptimalClusters(n, 1, maxSize) = (ceil(n / maxSize) + n) / 2 parts (:303) -- a little over n / 2 of them, since a minimum
        of 1 puts the upper end of the range at n; ceil(n / maxSize) is the usual choice for "as few parts as maxSize allows".  ValueError, with the state as it was, for an
        id that is not held, a frozen cluster, or a sub-run that cannot meet its constraints."""
        keys = list(dict.fromkeys(keys))
        where = self._where(keys, "split")
        at = sorted({where[k] for k in keys})
        if any(self.clusters[i].Frozen for i in at):
            raise ValueError("split: a cluster holding one of these ids is frozen")
        parts = {}
        for i in at:
            members = self.clusters[i].Members
            if len(members) < 2:
                continue
            C = np.stack([self.embeddings[k] for k in members]).astype(np.float32)
            ss = np.ones(len(members), np.int32)
            if self.engine is not None:
                _, _, _, st, mg, co = self.engine(C, ss, 1, self.maxSize, k_target)
            else:
                _, _, _, st, mg, co = _seeded_call(self.ctx or default_context(), C, ss, 1, self.maxSize, k_target, update=self.update)
            if st == _lib.ICL_ERR_CONSTRAINT:
                raise ValueError("split: the cluster of %r cannot be divided under these constraints" % (members[0],))
            if st != _lib.ICL_OK:
                raise _lib.ICLError(st, "split: the sub-run failed with code %d" % st)
            parts[i] = [HeldCluster([members[s] for s in seq], np.array(co[seq[0]], np.float32, copy=True)) for seq in _final_seed_lists(len(members), mg)]
        self.clusters = [p for i, c in enumerate(self.clusters) for p in parts.get(i, [c])]
        self._renumber()

    def _duplicate_lists(self, E, threshold):
        """Per row of E: ([(held position, value), ...] over self.embeddings in the order they were added -- icl_pairs_between --,
        [(earlier row of E, value), ...] -- icl_pairs_within on E, whose row i lists exactly the j < i), and the held ids by position."""
        held = list(self.embeddings)
        if len(E) == 0:
            return [], held
        L = np.stack([self.embeddings[k] for k in held]).astype(np.float32) if held else np.zeros((0, E.shape[1]), np.float32)
        hp, hc, hv = _between_csr(E, L, threshold, self.ctx, self.between_engine)
        if self.pairs_engine is not None:
            bp, bc, bv = self.pairs_engine(E, threshold)
        else:
            bp, bc, bv = (self.ctx or default_context()).pairs_within(E, threshold)
        return [([(int(hc[p]), float(hv[p])) for p in range(int(hp[i]), int(hp[i + 1]))],
                 [(int(bc[p]), float(bv[p])) for p in range(int(bp[i]), int(bp[i + 1]))]) for i in range(len(E))], held

    def duplicates_of(self, embeddings, ids, threshold: float) -> List[List[Tuple[str, float]]]:
        """For each incoming image, every image it duplicates (WardDistance as singletons at most threshold, exact and complete): its
        partners among all held images, in the order they were added (icl_pairs_between: the held images are never compared with each
        other), then its partners at earlier positions of the same batch (icl_pairs_within on the batch) -> one list of (id, value) per
        incoming image.  The state is not changed."""
        ids = list(ids)
        lists, held = self._duplicate_lists(_rows_of(embeddings, ids), threshold)
        return [[(held[j], v) for j, v in h] + [(ids[j], v) for j, v in b] for h, b in lists]

    def add(self, embeddings, ids, skip_duplicates: Optional[float] = None):
        """New images, each a singleton seed behind the clusters held so far.  With skip_duplicates = a threshold, an incoming image that
        has any partner under it (duplicates_of) among the held images or at an earlier position of the batch -- skipped or not -- is not
        added, and the method returns [(skipped id, partner id, value), ...] in batch order: the partner named is the held partner added
        first if there is one, otherwise the earliest batch partner.  With None nothing is compared and nothing is returned."""
        E = _rows_of(embeddings, ids)
        skipped = []
        if skip_duplicates is not None:
            ids = list(ids)
            clash = [k for k in ids if k in self.embeddings]
            if clash or len(set(ids)) != len(ids):
                raise ValueError("id %r is already clustered" % (clash[0],) if clash else "an id is listed twice")
            lists, held = self._duplicate_lists(E, skip_duplicates)
            keep = []
            for i, (h, b) in enumerate(lists):
                if h or b:
                    skipped.append((ids[i], held[h[0][0]], h[0][1]) if h else (ids[i], ids[b[0][0]], b[0][1]))
                else:
                    keep.append(i)
            E, ids = E[keep], [ids[i] for i in keep]
        for row, key in zip(E, ids):
            if key in self.embeddings:
                raise ValueError("id %r is already clustered" % (key,))
            self.embeddings[key] = np.array(row, np.float32, copy=True)
            self.clusters.append(HeldCluster([key], self.embeddings[key].copy()))
        return skipped if skip_duplicates is not None else None

    def _holding(self, keys) -> List[int]:
        where = {k: i for i, c in enumerate(self.clusters) for k in c.Members}
        return sorted({where[k] for k in keys})

    def freeze(self, keys):
        for i in self._holding(keys):
            self.clusters[i].Frozen = True

    def unfreeze(self, keys):
        for i in self._holding(keys):
            self.clusters[i].Frozen = False

    def dissolve(self, keys):
        """The clusters holding these ids fall apart: their members become singleton seeds again, in member order, at the end."""
        gone = self._holding(keys)
        freed = [k for i in gone for k in self.clusters[i].Members]
        self.clusters = [c for i, c in enumerate(self.clusters) if i not in set(gone)]
        self.clusters += [HeldCluster([k], self.embeddings[k].copy()) for k in freed]

    def keep_apart(self, keys):
        """The clusters holding these ids are mutually apart from now on: no recluster() merges two of them, nor clusters that swallowed
        them.  Held per image id, so it survives merges and dissolve().  ValueError when two of the ids already share a cluster.  The
        state may hold any number of clusters (icl_cluster_many_apart up to 2 048, icl_cluster_apart on the large-N engine above)."""
        keys = list(dict.fromkeys(keys))
        where = {k: i for i, c in enumerate(self.clusters) for k in c.Members}
        at = [where[k] for k in keys]
        if len(set(at)) != len(at):
            raise ValueError("keep_apart: two of these ids already share a cluster")
        if len(keys) >= 2:
            self.apart.append(keys)

    def _apart_pairs(self, clusters=None) -> List[Tuple[int, int]]:
        """The keep-apart relation over the held clusters: sorted (a, b), a < b, positions in self.clusters."""
        where = {k: i for i, c in enumerate(self.clusters if clusters is None else clusters) for k in c.Members}
        found = set()
        for group in self.apart:
            at = sorted({where[k] for k in group if k in where})
            found.update((a, b) for x, a in enumerate(at) for b in at[x + 1:])
        return sorted(found)

    def keep_together(self, keys):
        """The clusters holding these ids become one, now, on the host: merged in held order with MergeClusters' rule (clustering.go:
        31-40: a's members then b's, centroid (float(sa) Ca + float(sb) Cb) / float(sa + sb), each operation rounded to fp32), the new
        cluster in the first one's place, frozen if any part was.  ValueError, with the state as it was, when a keep-apart constraint
        forbids it or the cluster would hold more than maxSize items."""
        at = self._holding(keys)
        if len(at) < 2:
            return
        if any(a in at and b in at for a, b in self._apart_pairs()):
            raise ValueError("keep_together: a keep-apart constraint holds between two of these clusters")
        if sum(len(self.clusters[i].Members) for i in at) > self.maxSize:
            raise ValueError("keep_together: %d items, above maxSize (%d)" % (sum(len(self.clusters[i].Members) for i in at), self.maxSize))
        first = self.clusters[at[0]]
        members, cen, frozen = list(first.Members), np.array(first.Centroid, np.float32, copy=True), first.Frozen
        for i in at[1:]:
            c = self.clusters[i]
            sa, sb = len(members), len(c.Members)
            cen = ((np.float32(sa) * cen + np.float32(sb) * np.asarray(c.Centroid, np.float32)) / np.float32(sa + sb)).astype(np.float32)
            members, frozen = members + list(c.Members), frozen or c.Frozen
        self.clusters[at[0]] = HeldCluster(members, cen, frozen)
        self.clusters = [c for i, c in enumerate(self.clusters) if i not in set(at[1:])]
        kept = 0  # the report's ids (clustering.go:265-280): dense over the clusters of at least minSize items, in held order
        for c in self.clusters:
            c.Id = -1
            if len(c.Members) >= self.minSize:
                c.Id, kept = kept, kept + 1

    def absorb_leftovers(self) -> List[str]:
        """"Put the leftovers somewhere": the loop resumed with every kept, unfrozen cluster (at least minSize items) allowed to take
        the dropped clusters' images but not another kept cluster -- class 1 of icl_cluster_many_apart, of icl_cluster_apart above
        2 048 held clusters -- and k_target = the kept and
        the frozen clusters.  Returns the ids still unplaced: those no kept cluster could take (sizes, keep_apart, frozen)."""
        kept = [len(c.Members) >= self.minSize and not c.Frozen for c in self.clusters]
        k = sum(kept) + sum(c.Frozen for c in self.clusters)
        if k < len(self.clusters):
            self.recluster(max(1, k), _anchor=np.array(kept, np.int32))
        return [key for c in self.clusters if len(c.Members) < self.minSize for key in c.Members]

    def constraints(self) -> Dict[str, list]:
        """What is held: the keep_apart groups (image ids), the cluster pairs they stand for now (first members' ids), the frozen
        clusters (first members' ids)."""
        return {"apart": [list(g) for g in self.apart],
                "apart_clusters": [(self.clusters[a].Members[0], self.clusters[b].Members[0]) for a, b in self._apart_pairs()],
                "frozen": [c.Members[0] for c in self.clusters if c.Frozen]}

    def seeds(self):
        """The seeded problem the state stands for: (centroids m x d, seed_size m; negative: frozen)."""
        d = len(next(iter(self.embeddings.values()))) if self.embeddings else 0
        C = np.stack([c.Centroid for c in self.clusters]).astype(np.float32) if self.clusters else np.zeros((0, d), np.float32)
        ss = np.array([-len(c.Members) if c.Frozen else len(c.Members) for c in self.clusters], np.int32)
        return C, ss

    def recluster(self, k_target: int = 0, _anchor=None) -> bool:
        """Resume the loop from the clusters held, keep_apart's constraints respected at any number of clusters (_seeded_call picks
        the engine).  False, with the state as it was, when the constraints cannot be met.  (_anchor: absorb_leftovers' class per cluster.)"""
        C, ss = self.seeds()
        pairs = np.array(self._apart_pairs(), np.int32).reshape(-1, 2)
        extra = (_anchor, pairs) if _constrained(_anchor, pairs) else ()
        if extra and self.update == _lib.UPDATE_LW:
            raise _lib.ICLError(_lib.ICL_ERR_UNSUPPORTED, "FAST mode (UPDATE_LW) keeps no keep-apart constraints")
        if self.engine is not None:
            cid, rank, nc, st, mg, co = self.engine(C, ss, self.minSize, self.maxSize, k_target, *extra)
        else:
            ctx = self.ctx or default_context()
            cid, rank, nc, st, mg, co = _seeded_call(ctx, C, ss, self.minSize, self.maxSize, k_target, *extra, update=self.update)
        self.ok = st == _lib.ICL_OK
        if st == _lib.ICL_ERR_CONSTRAINT:
            return False
        if st != _lib.ICL_OK:
            raise _lib.ICLError(st, "seeded clustering: the problem failed with code %d" % st)
        # the final list from the merge log: surviving seeds in seed order, then merged clusters in creation order, a's seeds before b's
        held = []
        for seq in _final_seed_lists(len(self.clusters), mg):
            first = seq[0]
            # an image's rank: the items of the seeds before its own, plus its place in its own seed
            members = [k for s in seq for k in self.clusters[s].Members]
            held.append(HeldCluster(members, np.array(co[first], np.float32, copy=True), len(seq) == 1 and self.clusters[first].Frozen, int(cid[first])))
        self.clusters = held
        self.last_merges = np.asarray(mg, np.int32).reshape(-1, 2).copy()
        return True

    def nearest(self, embeddings, k: int) -> List[List[Tuple[str, float]]]:
        """Where add() + recluster() could put new images: for each embedding, taken as a singleton, the up to k held clusters that could
        take it, nearest first, as (the cluster's first member's id, WardDistance).  Frozen clusters are left out, and so are clusters
        a new item would push above maxSize (icl_nearest's max_size rule).  The state is not changed."""
        Q = np.asarray(embeddings, np.float32)
        if Q.ndim != 2:
            Q = Q.reshape(len(embeddings), -1)
        cand = [c for c in self.clusters if not c.Frozen]
        if not cand or len(Q) == 0:
            return [[] for _ in range(len(Q))]
        E = np.stack([c.Centroid for c in cand]).astype(np.float32)
        es = np.array([len(c.Members) for c in cand], np.int32)
        qs = np.ones(len(Q), np.int32)
        if self.nearest_engine is not None:
            idx, val = self.nearest_engine(Q, E, k, qs, es, self.maxSize)
        else:
            idx, val = (self.ctx or default_context()).nearest(Q, E, k, q_size=qs, e_size=es, max_size=self.maxSize)
        return [[(cand[int(j)].Members[0], float(v)) for j, v in zip(ri, rv) if j >= 0] for ri, rv in zip(idx, val)]

    def _fit_call(self, k: int):
        """icl_cluster_fit over every held image as a singleton and every held cluster -> (image ids in row order, the call's dict)."""
        ids = [key for c in self.clusters for key in c.Members]
        if not ids:
            return ids, None
        Q = np.stack([self.embeddings[key] for key in ids]).astype(np.float32)
        cof = np.array([ci for ci, c in enumerate(self.clusters) for _ in c.Members], np.int32)
        C, cs = self.seeds()
        qs = np.ones(len(ids), np.int32)
        if self.fit_engine is not None:
            return ids, self.fit_engine(Q, cof, C, k, qs, cs, self.maxSize)
        return ids, (self.ctx or default_context()).cluster_fit(Q, cof, C, k, q_size=qs, c_size=cs, max_size=self.maxSize)

    def fit(self, k: int = 1) -> Dict[str, Tuple[float, List[Tuple[str, float]]]]:
        """How well each held image sits where it is: id -> (WardDistance of the image, as a singleton, to its own cluster, [(first
        member's id of another cluster, WardDistance), ...] nearest first, at most k).  Both are the loop's own cost in the same
        arithmetic.  Frozen clusters are left out of the alternatives, and so are clusters a further item would push above maxSize; an
        image's own cluster is measured whether frozen or full.  The state is not changed."""
        ids, r = self._fit_call(k)
        if r is None:
            return {}
        return {key: (float(r["own"][i]), [(self.clusters[int(j)].Members[0], float(v)) for j, v in zip(r["alt_idx"][i], r["alt_val"][i]) if j >= 0])
                for i, key in enumerate(ids)}

    def representatives(self) -> Dict[str, str]:
        """The cover image of each held cluster: first member's id -> the id of the member of smallest cost to the cluster's centroid
        (ties: the earliest member)."""
        ids, r = self._fit_call(0)
        if r is None:
            return {}
        return {c.Members[0]: ids[int(r["rep"][ci])] for ci, c in enumerate(self.clusters)}

    def misfits(self) -> List[str]:
        """The images another cluster would take at a lower cost than their own cluster's: ids whose first alternative costs less than
        their own cost (an exact comparison: one arithmetic), largest gain first, ties in member order."""
        found = [(own - alts[0][1], key) for key, (own, alts) in self.fit(1).items() if alts and alts[0][1] < own]
        return [key for _, key in sorted(found, key=lambda t: -t[0])]

    def as_map(self) -> Dict[int, List[str]]:
        """The reference's map[int][]string (clustering.go:265-280): the kept clusters."""
        return {c.Id: list(c.Members) for c in self.clusters if c.Id >= 0}

    def assignments(self) -> Dict[str, Tuple[int, int]]:
        """id -> (cluster id or -1, rank in the cluster's member list or -1)"""
        return {k: ((c.Id, r) if c.Id >= 0 else (-1, -1)) for c in self.clusters for r, k in enumerate(c.Members)}


def clusters_as_map(cluster_id, member_rank, ids) -> Dict[int, List[str]]:
    """Canonical (cluster_id, member_rank) -> map[int][]string of clustering.go:265-280."""
    out: Dict[int, List[str]] = {}
    order = np.lexsort((member_rank, cluster_id))
    for i in order:
        c = int(cluster_id[i])
        if c >= 0:
            out.setdefault(c, []).append(ids[i])
    return out



# ---- dendrogram export -----------------------------------------------------------------------
def LastDendrogram(n: int, ctx: Optional[_lib.Context] = None) -> np.ndarray:
    """The merge tree of the last PerformClusteringWithConstraints / cluster call as a scipy-style linkage matrix
    Z[t] = [id_a, id_b, ward_distance, size]: singleton i has id i, the cluster created by merge t has id n+t (the
    engine's creation ids are exactly that convention).  The reference stops at k clusters (clustering.go:220), so Z has
    n-k rows: a forest cut at the size constraints, not a full tree.  Heights are the values FindClosestClusters
    returned (clustering.go:123-131), i.e. WardDistance of the merged pair (:84) -- not scipy's sqrt(2*d) scale."""
    ctx = ctx or default_context()
    m = ctx.last_merges().astype(np.int64)
    v = ctx.last_merge_values().astype(np.float64)
    size = np.ones(n + len(m), np.int64)
    Z = np.zeros((len(m), 4), np.float64)
    for t, (a, b) in enumerate(m):
        size[n + t] = size[a] + size[b]
        Z[t] = (a, b, v[t], size[n + t])
    return Z


def ExportDendrogram(path: str, Z: np.ndarray, ids: Optional[List[str]] = None):
    """Writes the linkage matrix (and the item ids) as JSON: {"n", "ids", "merges": [[a, b, height, size], ...]}."""
    import json

    n = int(len(ids)) if ids is not None else int(Z[:, :2].max() + 2 - len(Z)) if len(Z) else 0
    with open(path, "w") as f:
        json.dump({"n": n, "ids": list(ids) if ids is not None else None,
                   "merges": [[int(r[0]), int(r[1]), float(r[2]), int(r[3])] for r in Z]}, f)
