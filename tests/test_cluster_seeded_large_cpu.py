"""icl_cluster_seeded without a GPU: the ABI (header, exports, ctypes table), the argument check, and the Python state's routing between
icl_cluster_many_seeded (up to 2 048 seeds) and icl_cluster_seeded (above) with a stub in place of the context."""
import ctypes
import os
import re

import numpy as np

from tests import seeded_cases as SC
from tests import seeded_large_cases as LC
from tests import ward_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("icl_cluster_seeded", "icl_cluster_seeded_dev")


def test_new_symbols_in_header_exports_and_ctypes_table():
    from imageclust_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "imageclust.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(icl_[a-z0-9_]+)\s*\(", src))
    bound = {s[0]: s for s in _lib.SYMBOLS}
    raw = ctypes.CDLL(_lib.SO_PATH)
    L = _lib.load()
    for name in NEW:
        assert name in declared, "%s is not declared in include/imageclust.h" % name
        assert hasattr(raw, name), "the library does not export %s" % name
        assert name in bound and len(bound[name][2]) == 12, "ctypes table: %s" % name
        assert getattr(L, name).restype is ctypes.c_int
    # (ctx, C, m, d, seed_size, min, max, k_target, cluster_id, seed_rank, n_clusters, C_out) in both
    assert bound[NEW[0]][2] == bound[NEW[1]][2]


def test_bad_arguments_are_refused_without_a_gpu():
    """A null context fails before any device call, whatever else is passed: ICL_ERR_ARG and nothing written."""
    from imageclust_amd import _lib

    L = _lib.load()
    C = np.ones((3, 2), np.float32)
    ss = np.ones(3, np.int32)
    for name in NEW:
        fn = getattr(L, name)
        cid, rank, co = np.full(3, 777, np.int32), np.full(3, 777, np.int32), np.full((3, 2), 777.0, np.float32)
        nc = ctypes.c_int32(777)
        assert fn(None, C.ctypes.data, 3, 2, ss.ctypes.data, 1, 2, 0, cid.ctypes.data, rank.ctypes.data, ctypes.byref(nc), co.ctypes.data) == _lib.ICL_ERR_ARG
        assert fn(None, None, 3, 2, None, 1, 2, 0, None, None, None, None) == _lib.ICL_ERR_ARG
        assert fn(None, None, -1, -1, None, 1, 2, 0, None, None, None, None) == _lib.ICL_ERR_ARG
        assert (cid == 777).all() and (rank == 777).all() and nc.value == 777 and (co == 777.0).all()


class StubContext:
    """Stands where a _lib.Context would: records which seeded call the state takes and answers with a valid result made on the host --
    `merges` merges of neighbouring seeds (tests/seeded_large_cases.fake_pair_log), ids by icl_seeded_assign_ids, centroids by the oracle."""

    def __init__(self, merges):
        self.merges, self.calls = merges, []

    def _answer(self, C, ss, mn):
        from imageclust_amd import _lib

        log = LC.fake_pair_log(len(ss), min(self.merges, len(ss) // 2))
        cid, rank, nc = _lib.seeded_assign_ids(ss, mn, log)
        return cid, rank, nc, 0, log, SC.centroids_from_log(C, ss, log)

    def cluster_seeded(self, C, ss, mn, mx, k_target=0, want_centroids=True, dev=False):
        self.calls.append(("large", len(ss), k_target))
        return self._answer(C, ss, mn)

    def cluster_many_seeded(self, problems, want_merges=False, want_centroids=False, raise_on_error=False, dev=False):
        assert want_merges and want_centroids and len(problems) == 1
        C, ss, mn, mx, kt = problems[0]
        self.calls.append(("many", len(ss), kt))
        return [self._answer(C, ss, mn)]


def test_state_routes_by_seed_count_and_keeps_2100_members():
    from imageclust_amd import clustering

    assert clustering.MANY_SEEDED_MAX == SC.MAX_SEEDS == 2048
    n = 2100
    E = WC.mog(n, 4, 7)
    ids = ["img_%d" % i for i in range(n)]
    stub = StubContext(merges=40)
    st = clustering.Clustering.start(E, ids, 1, 6, ctx=stub)
    assert st.ok and stub.calls == [("large", n, 0)]  # above the cap: the large-N engine's call
    assert len(st.clusters) == n - 40
    assert sorted(k for c in st.clusters for k in c.Members) == sorted(ids)  # every member is still held, once
    # the final list: surviving seeds in seed order, then the merged clusters in creation order, a's members before b's
    assert [c.Members for c in st.clusters[-40:]] == [[ids[2 * t + 1], ids[2 * t]] for t in range(40)]
    assert st.clusters[0].Members == [ids[80]] and np.array_equal(st.clusters[0].Centroid, E[80])
    from oracle import oracle as O

    assert SC.same_bits(st.clusters[-40].Centroid, O.merge_centroid(E[1], 1, E[0], 1))
    assert st.as_map() == {i: list(c.Members) for i, c in enumerate(st.clusters)}  # min_size 1: nothing dropped, dense ids in list order
    # 2 060 clusters held: still above the cap; k_target travels
    st.freeze([ids[80]])
    stub.merges = 0
    assert st.recluster(k_target=2000) and stub.calls[-1] == ("large", n - 40, 2000)
    assert st.seeds()[1][0] == -1 and st.clusters[0].Frozen
    # exactly at the cap and one above it
    for m, route in ((2048, "many"), (2049, "large")):
        stub2 = StubContext(merges=0)
        s2 = clustering.Clustering(1, 6, ctx=stub2)
        s2.add(E[:m], ids[:m])
        assert s2.recluster() and stub2.calls == [(route, m, 0)]
        (cid, rank, nc, mg, co), ok = clustering.PerformClusteringSeeded(E[:m], np.ones(m, np.int32), 1, 6, ctx=stub2)
        assert ok and nc == m and stub2.calls[-1] == (route, m, 0) and np.array_equal(co, E[:m])
