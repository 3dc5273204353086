"""Seeded clustering without a GPU (DESIGN.md "Seeded clustering"): the checker of tests/seeded_cases.py against the oracle, the
restart identity on the checker, the host-only id rule icl_seeded_assign_ids against the checker's final lists, and the bookkeeping of
clustering.Clustering with the checker as its engine."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import seeded_cases as SC
from tests import ward_cases as WC


@pytest.fixture(scope="module")
def singleton_runs():
    """(name, E, min, max, checker's run from all-ones seeds) for the small cases of at most 48 rows"""
    return [(name, E, mn, mx, SC.run(E, np.ones(len(E), np.int32), mn, mx)) for name, E, mn, mx in SC.small_singleton_cases()]


def test_checker_from_singletons_is_the_oracle(singleton_runs):
    assert len(singleton_runs) >= 25
    for name, E, mn, mx, r in singleton_runs:
        ref = O.cluster(E, mn, mx, want_log=True)
        if not ref["ok"]:
            assert r["status"] == SC.ERR_CONSTRAINT, name
            continue
        assert r["status"] == SC.OK, name
        assert np.array_equal(r["log"], ref["log"][:, 2:4].astype(np.int32)), name
        assert np.array_equal(r["cluster_id"], ref["cluster_id"]) and np.array_equal(r["seed_rank"], ref["member_rank"]), name
        assert r["n_clusters"] == ref["n_clusters"], name


def test_split_and_resume_is_the_same_run(singleton_runs):
    """A run cut after t merges and resumed from that state logs the rest of the run and ends with the same centroids, bit for bit.
    The bans made before the cut are not carried over."""
    runs = 0
    for name, E, mn, mx, r in singleton_runs:
        if r["status"] != SC.OK:
            continue
        m, log = len(E), r["log"]
        for t in SC.cuts(len(log)):
            C2, ss2, seeds2, ids = SC.state_after(E, np.ones(m, np.int32), log, t)
            r2 = SC.run(C2, ss2, mn, mx, k_target=len(ids) - (len(log) - t))
            assert r2["status"] == SC.OK, (name, t)
            assert np.array_equal(r2["log"], SC.resumed_log(log, t, ids, m)), (name, t)
            # the same final clusters: members through the state's seed sequences, centroids as uint32
            fin = {tuple(s for q in f[1] for s in seeds2[q]): f[3] for f in r2["finals"]}
            ref = {tuple(f[1]): f[3] for f in r["finals"]}
            assert fin.keys() == ref.keys(), (name, t)
            for key in ref:
                assert np.array_equal(fin[key].view(np.uint32), ref[key].view(np.uint32)), (name, t)
            runs += 1
    assert runs >= 60


def _mixed_cases():
    out = []
    for m, d, seed in [(2, 3, 0), (3, 8, 1), (17, 3, 2), (40, 8, 3), (33, 5, 4)]:
        for ties in (False, True):
            out.append(("mixed_%d_%d_%d" % (m, d, ties), SC.mixed_problem(m, d, seed, ties=ties), 0))
    C, ss, mn, mx = SC.mixed_problem(30, 4, 9)
    out.append(("k_below", (C, ss, mn, mx), 4))
    out.append(("k_above", (C, ss, mn, mx), 99))
    out.append(("k_one", (C, np.abs(ss).clip(1, 2).astype(np.int32), 1, 1000), 1))
    out.append(("all_frozen", (C, -np.abs(ss), mn, mx), 2))
    out.append(("min_drops_real_sizes", (C[:6], np.array([1, 2, -2, 3, -7, 1], np.int32), 3, 3), 6))
    return out


def test_seeded_assign_ids_equals_the_checker(singleton_runs):
    """icl_seeded_assign_ids: the final-list rule at seed granularity, from (sizes, min_size, merge log) alone: the drop rule counts
    ITEMS, frozen seeds below min_size are dropped like any other, m = 0 and m = 1 work."""
    from imageclust_amd import _lib

    probs = [(name, (E, np.ones(len(E), np.int32), mn, mx), 0) for name, E, mn, mx, _ in singleton_runs] + _mixed_cases()
    checked = 0
    for name, (C, ss, mn, mx), kt in probs:
        r = SC.run(C, ss, mn, mx, kt)
        if r["status"] != SC.OK:
            continue
        cid, rank, nc = _lib.seeded_assign_ids(ss, mn, r["log"])
        assert np.array_equal(cid, r["cluster_id"]) and np.array_equal(rank, r["seed_rank"]) and nc == r["n_clusters"], name
        checked += 1
    assert checked >= 35
    # dropped by item count, not by seed count: a lone seed of 3 items is kept at min_size 3, two merged seeds of 1 item are not
    cid, rank, nc = _lib.seeded_assign_ids([3, 1, 1, -1], 3, [(2, 1)])
    assert cid.tolist() == [0, -1, -1, -1] and rank.tolist() == [0, -1, -1, -1] and nc == 1
    cid, rank, nc = _lib.seeded_assign_ids([1, 1, 2, -5], 3, [(2, 0), (4, 1)])  # Merge(Merge(2, 0), 1): seeds 2, 0, 1
    assert cid.tolist() == [1, 1, 1, 0] and rank.tolist() == [1, 2, 0, 0] and nc == 2
    cid, rank, nc = _lib.seeded_assign_ids([], 1, [])
    assert len(cid) == 0 and len(rank) == 0 and nc == 0
    assert [x.tolist() if hasattr(x, "tolist") else x for x in _lib.seeded_assign_ids([4], 5, [])] == [[-1], [-1], 0]
    assert [x.tolist() if hasattr(x, "tolist") else x for x in _lib.seeded_assign_ids([-4], 4, [])] == [[0], [0], 1]
    for bad in ([(1, 1)], [(2, 0)], [(1, 0), (1, 2)], [(-1, 0)]):  # a log that names a cluster that is not there
        with pytest.raises(_lib.ICLError) as ei:
            _lib.seeded_assign_ids([1, 1], 1, bad)
        assert ei.value.code == _lib.ICL_ERR_ARG
    with pytest.raises(_lib.ICLError) as ei:
        _lib.seeded_assign_ids([1, 0], 1, [])
    assert ei.value.code == _lib.ICL_ERR_ARG


def _checker_engine(calls):
    def engine(C, ss, mn, mx, kt):
        calls.append((C.copy(), ss.copy(), kt))
        r = SC.run(C, ss, mn, mx, kt)
        return r["cluster_id"], r["seed_rank"], r["n_clusters"], r["status"], r["log"], r["C_out"]

    return engine


def test_clustering_state_bookkeeping():
    from imageclust_amd import clustering

    E = WC.mog(27, 6, 5, k=4, sigma=0.2)
    ids = ["img_%d" % i for i in range(27)]
    calls = []
    st = clustering.Clustering.start(E[:20], ids[:20], 3, 6, engine=_checker_engine(calls))
    ref = O.cluster(E[:20], 3, 6)
    assert st.ok and st.as_map() == O.clusters_as_map(ref["cluster_id"], ref["member_rank"], ids[:20])
    assert sorted(k for c in st.clusters for k in c.Members) == sorted(ids[:20])  # dropped clusters are kept in the state
    held = [(list(c.Members), c.Centroid.copy()) for c in st.clusters]

    st.add(E[20:], ids[20:])
    frozen_key = st.clusters[0].Members[-1]
    st.freeze([frozen_key])
    C, ss = st.seeds()
    assert len(ss) == len(held) + 7 and ss[0] == -len(held[0][0]) and (ss[1:] > 0).all() and (ss[-7:] == 1).all()
    assert np.array_equal(C[:len(held)], np.stack([h[1] for h in held])) and np.array_equal(C[-7:], E[20:])
    members = [list(c.Members) for c in st.clusters]
    assert st.recluster()
    r = SC.run(C, ss, 3, 6)
    # rank expansion: the members of a final cluster are its seeds' members, seed after seed
    want = {}
    for fid, seq, items, cen in r["finals"]:
        if items >= 3:
            want[len(want)] = [k for s in seq for k in members[s]]
    assert st.as_map() == want
    assert st.clusters[0].Frozen and st.clusters[0].Members == held[0][0]  # the frozen cluster came through untouched, first in the list
    assert np.array_equal(st.clusters[0].Centroid, held[0][1])
    for c, (fid, seq, items, cen) in zip(st.clusters, r["finals"]):
        assert np.array_equal(c.Centroid.view(np.uint32), cen.view(np.uint32)) and len(c.Members) == items
    asg = st.assignments()
    for cid, mem in want.items():
        assert [asg[k] for k in mem] == [(cid, q) for q in range(len(mem))]

    st.unfreeze([frozen_key])
    assert not st.clusters[0].Frozen
    # dissolve: the members come back as singleton seeds with their own embeddings, behind the clusters that stay
    victim = list(st.clusters[1].Members)
    n_before = len(st.clusters)
    st.dissolve([victim[0]])
    C, ss = st.seeds()
    assert len(st.clusters) == n_before - 1 + len(victim) and [c.Members for c in st.clusters[-len(victim):]] == [[k] for k in victim]
    assert np.array_equal(C[-len(victim):], np.stack([E[ids.index(k)] for k in victim]))
    assert st.recluster(k_target=5) and calls[-1][2] == 5 and len(st.clusters) >= 5
    with pytest.raises(ValueError):
        st.add(E[:1], ids[:1])
    # impossible constraints: start() reports it and keeps the singletons
    bad = clustering.Clustering.start(E[:2], ids[:2], 3, 6, engine=_checker_engine([]))
    assert not bad.ok and bad.as_map() == {} and len(bad.clusters) == 2
