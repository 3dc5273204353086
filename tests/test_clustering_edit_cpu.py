"""Editing a held clustering without a GPU (DESIGN.md "Editing a held clustering"): Clustering.remove / move / from_partition /
oversized / split and workflow.RunMore(remove_ids=) with the checkers standing in for the GPU calls -- tests/seeded_cases.run for the
seeded loop, tests/fold_cases.fold for icl_fold_centroids."""
import copy
import types

import numpy as np
import pytest

from imageclust_amd import _lib, clustering as CL, workflow as WF
from tests import fold_cases as FC
from tests import seeded_cases as SC
from tests import ward_cases as WC

N, D, MIN, MAX = 40, 8, 3, 6


def seeded(C, ss, mn, mx, kt, *extra):
    assert not extra, "no constraint reaches the engine in these tests"
    r = SC.run(C, ss, mn, mx, kt)
    return r["cluster_id"], r["seed_rank"], r["n_clusters"], r["status"], r["log"], r["C_out"]


class Folds:
    """The numpy fold as fold_engine, counting its calls"""

    def __init__(self):
        self.calls = []

    def __call__(self, E, row_ptr, member, size):
        self.calls.append((len(row_ptr) - 1, len(member)))
        return FC.fold(E, row_ptr, member, size)


def problem():
    return WC.mog(N, D, 11, k=6, sigma=0.3), ["i%d" % i for i in range(N)]


def started(folds=None):
    E, ids = problem()
    return CL.Clustering.start(E, ids, MIN, MAX, engine=seeded, fold_engine=folds or Folds()), E, ids


def fold_of(state, members):
    E = np.stack([state.embeddings[k] for k in members])
    return FC.fold(E, [0, len(members)], np.arange(len(members)))[0][0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def ids_follow_the_rule(state):
    kept = [c for c in state.clusters if len(c.Members) >= state.minSize]
    return [c.Id for c in kept] == list(range(len(kept))) and all(c.Id == -1 for c in state.clusters if len(c.Members) < state.minSize)


def test_the_fast_stand_in_is_the_seeded_checker():
    """tests/fold_cases.seeded_engine (what the GPU edit tests use above 2 048 seeds) against tests/seeded_cases.run"""
    for m, d, seed in ((0, 3, 1), (1, 3, 2), (17, 3, 3), (64, 8, 4), (120, 8, 5)):
        C = WC.ties(m, d, seed, levels=3) if seed % 2 else WC.mog(m, d, seed, k=max(1, m // 6), sigma=0.3)
        ss = np.random.default_rng(seed).choice(np.array([1, 1, 1, 2, 3, 6], np.int32), m).astype(np.int32)
        for kt in (0, max(1, m // 3)):
            r = SC.run(C, ss, MIN, MAX, kt)
            SC.same_as_checker(FC.seeded_engine(C, ss, MIN, MAX, kt), r, (m, d, kt))
    assert FC.seeded_engine(np.zeros((2, 3), np.float32), np.array([1, 7], np.int32), MIN, MAX)[3] == SC.ERR_UNSUPPORTED
    assert FC.seeded_engine(np.zeros((2, 3), np.float32), np.array([1, 1], np.int32), MIN, MAX)[3] == SC.ERR_CONSTRAINT


# ---- remove -----------------------------------------------------------------------------------------------------------------------
def test_remove_singletons_then_recluster_is_the_run_without_them():
    E, ids = problem()
    folds = Folds()
    st = CL.Clustering(MIN, MAX, engine=seeded, fold_engine=folds)
    st.add(E, ids)
    st.remove([ids[5], ids[11], ids[39]])
    assert folds.calls == []  # nothing is left to rebuild
    assert st.recluster()
    keep = [i for i in range(N) if i not in (5, 11, 39)]
    ref = CL.Clustering.start(E[keep], [ids[i] for i in keep], MIN, MAX, engine=seeded)
    assert FC.snapshot(st) == FC.snapshot(ref)


def test_remove_rebuilds_by_the_fold_in_one_call():
    folds = Folds()
    st, E, ids = started(folds)
    before = copy.deepcopy(st.clusters)
    big = [c for c in st.clusters if len(c.Members) >= 3][:2]
    gone = [big[0].Members[1], big[1].Members[0], big[1].Members[2]]
    st.remove(gone)
    assert folds.calls == [(2, len(big[0].Members) + len(big[1].Members) - 3)]
    assert all(k not in st.embeddings for k in gone) and len(st.embeddings) == N - 3
    for old in before:
        left = [k for k in old.Members if k not in gone]
        now = next(c for c in st.clusters if c.Members == left)
        if len(left) == len(old.Members):
            assert bits(now.Centroid) == bits(old.Centroid)  # untouched: the centroid the loop left
        else:
            assert bits(now.Centroid) == bits(fold_of(st, left))
    assert [c.Members for c in st.clusters] == [[k for k in o.Members if k not in gone] for o in before]
    assert ids_follow_the_rule(st)


def test_remove_the_last_member_and_from_a_frozen_cluster():
    st, E, ids = started()
    victim, frozen = st.clusters[0], st.clusters[1]
    st.freeze([frozen.Members[0]])
    n = len(st.clusters)
    st.remove(list(victim.Members) + [frozen.Members[0]])
    assert len(st.clusters) == n - 1 and all(c.Members != victim.Members for c in st.clusters)
    now = st.clusters[0]
    assert now.Frozen and now.Members == frozen.Members[1:] and bits(now.Centroid) == bits(fold_of(st, now.Members))
    assert ids_follow_the_rule(st)
    st.remove(list(now.Members))  # a frozen cluster can be deleted whole
    assert not any(c.Frozen for c in st.clusters)
    st.remove(list(st.embeddings))
    assert st.clusters == [] and st.embeddings == {} and st.as_map() == {}


def test_remove_prunes_the_apart_groups():
    E, ids = problem()
    st = CL.Clustering(MIN, MAX, engine=seeded, fold_engine=Folds())
    st.add(E, ids)
    st.keep_apart(ids[:3])
    st.keep_apart(ids[3:5])
    st.remove([ids[0], ids[3]])
    assert st.apart == [[ids[1], ids[2]]]
    assert st.constraints()["apart_clusters"] == [(ids[1], ids[2])]


def test_remove_refusals_leave_the_state_alone():
    st, E, ids = started()
    st.keep_apart([ids[0], next(k for c in st.clusters if ids[0] not in c.Members for k in c.Members)])
    before = FC.snapshot(st)
    for bad in (["nobody"], [ids[2], ids[2]], [ids[1], "nobody"]):
        with pytest.raises(ValueError):
            st.remove(bad)
        assert FC.snapshot(st) == before

    def broken(*a):
        raise _lib.ICLError(_lib.ICL_ERR_HIP, "the fold failed")

    st.fold_engine = broken
    with pytest.raises(_lib.ICLError):
        st.remove([st.clusters[0].Members[0]])
    assert FC.snapshot(st) == before


# ---- move -------------------------------------------------------------------------------------------------------------------------
def two_with_room(st):
    """(a source cluster of at least 2, a target with room for 2 more)"""
    tgt = next(c for c in st.clusters if 2 <= len(c.Members) <= MAX - 2)
    src = next(c for c in st.clusters if c is not tgt and len(c.Members) >= 2)
    return src, tgt


def test_move_rebuilds_target_and_sources():
    folds = Folds()
    st, E, ids = started(folds)
    src, tgt = two_with_room(st)
    other = next(c for c in st.clusters if c is not src and c is not tgt and len(c.Members) >= 1)
    moved = [src.Members[1], other.Members[0]]
    want_t, want_s, want_o = tgt.Members + moved, [k for k in src.Members if k != moved[0]], other.Members[1:]
    untouched = [(list(c.Members), bits(c.Centroid)) for c in st.clusters if c not in (src, tgt, other)]
    pos = st.clusters.index(tgt) - (1 if not want_o and st.clusters.index(other) < st.clusters.index(tgt) else 0)
    st.move(moved, tgt.Members[0])
    assert len(folds.calls) == 1 and folds.calls[0][0] == 2 + bool(want_o)
    assert st.clusters[pos].Members == want_t  # appended in the order given, the cluster in its place
    for want in (want_t, want_s, want_o):
        if want:
            now = next(c for c in st.clusters if c.Members == want)
            assert bits(now.Centroid) == bits(fold_of(st, want))
    assert [(list(c.Members), bits(c.Centroid)) for c in st.clusters if c.Members not in (want_t, want_s, want_o)] == untouched
    assert ids_follow_the_rule(st) and len(st.embeddings) == N


def test_move_to_no_cluster_makes_singletons_at_the_end():
    folds = Folds()
    st, E, ids = started(folds)
    src = next(c for c in st.clusters if len(c.Members) >= 3)
    moved = [src.Members[2], src.Members[0]]
    left = [k for k in src.Members if k not in moved]
    n = len(st.clusters)
    st.move(moved)
    assert len(st.clusters) == n + 2 and [c.Members for c in st.clusters[-2:]] == [[moved[0]], [moved[1]]]
    assert all(bits(c.Centroid) == bits(st.embeddings[c.Members[0]]) and not c.Frozen for c in st.clusters[-2:])
    now = next(c for c in st.clusters if c.Members == left)
    assert bits(now.Centroid) == bits(fold_of(st, left)) and folds.calls == [(1, len(left))]
    assert ids_follow_the_rule(st)
    st.move([st.clusters[-1].Members[0]])  # a singleton moved to no cluster: it goes to the end, nothing to fold
    assert st.clusters[-1].Members == [moved[1]] and len(st.clusters) == n + 2 and len(folds.calls) == 1


def test_move_refusals_leave_the_state_alone():
    st, E, ids = started()
    src, tgt = two_with_room(st)
    full = next(c for c in st.clusters if c is not src and len(c.Members) >= MAX - 1)
    a, b = src.Members[0], src.Members[1]
    icy = next(c for c in st.clusters if c not in (src, tgt, full))
    st.freeze([icy.Members[0]])
    st.keep_apart([a, tgt.Members[0]])
    st.keep_apart([b, next(k for c in st.clusters if c not in (src, tgt) for k in c.Members)])
    before = FC.snapshot(st)
    refused = [(["nobody"], tgt.Members[0]), ([a, a], tgt.Members[0]), ([b], "nobody"), ([tgt.Members[1]], tgt.Members[0]),
               ([icy.Members[0]], tgt.Members[0]), ([icy.Members[0]], None), ([b], icy.Members[0]),
               ([k for c in st.clusters if c not in (full, icy) for k in c.Members][:MAX], full.Members[0]),
               ([a], tgt.Members[0]), ([b, a], tgt.Members[1])]
    for moved, key in refused:
        with pytest.raises(ValueError):
            st.move(moved, key)
        assert FC.snapshot(st) == before, (moved, key)
    folds = st.fold_engine
    st.move([], tgt.Members[0])  # nobody moves: no fold call, and the target keeps the centroid the loop left it
    st.move([])
    assert FC.snapshot(st) == before and folds.calls == []
    st.move([b], tgt.Members[0])  # b's keep-apart partner is elsewhere: allowed
    assert next(c for c in st.clusters if b in c.Members).Members[-1] == b


# ---- from_partition, oversized ------------------------------------------------------------------------------------------------------
def test_from_partition_of_singletons_resumes_as_start():
    E, ids = problem()
    folds = Folds()
    st = CL.Clustering.from_partition(E, ids, [], MIN, MAX, engine=seeded, fold_engine=folds)
    assert folds.calls == [(N, N)] and [c.Members for c in st.clusters] == [[k] for k in ids]
    assert all(bits(c.Centroid) == bits(E[i]) and c.Id == -1 for i, c in enumerate(st.clusters))
    assert st.recluster()
    assert FC.snapshot(st) == FC.snapshot(CL.Clustering.start(E, ids, MIN, MAX, engine=seeded))


def test_from_partition_adopts_a_finished_run_and_goes_on():
    ref, E, ids = started()
    groups = [list(c.Members) for c in ref.clusters if len(c.Members) >= 2]
    folds = Folds()
    st = CL.Clustering.from_partition(E, ids, groups, MIN, MAX, engine=seeded, fold_engine=folds)
    singles = [k for k in ids if not any(k in g for g in groups)]
    assert [c.Members for c in st.clusters] == groups + [[k] for k in singles] and len(folds.calls) == 1
    assert all(bits(c.Centroid) == bits(fold_of(st, c.Members)) for c in st.clusters)
    assert st.as_map() == {i: g for i, g in enumerate(g for g in groups if len(g) >= MIN)} and ids_follow_the_rule(st)
    more = WC.mog(7, D, 12, k=2, sigma=0.3)
    st.add(more, ["n%d" % i for i in range(7)])
    C, ss = st.seeds()
    held = [list(c.Members) for c in st.clusters]
    assert st.recluster()
    r = SC.run(C, ss, MIN, MAX)  # the seeded problem the adopted state stands for
    assert [c.Members for c in st.clusters] == [[k for s in f[1] for k in held[s]] for f in r["finals"]]
    assert all(bits(c.Centroid) == bits(f[3]) for c, f in zip(st.clusters, r["finals"]))
    with pytest.raises(ValueError):
        CL.Clustering.from_partition(E, ids, [[ids[0]], []], MIN, MAX, fold_engine=folds)
    with pytest.raises(ValueError):
        CL.Clustering.from_partition(E, ids, [[ids[0], ids[1]], [ids[1]]], MIN, MAX, fold_engine=folds)
    with pytest.raises(ValueError):
        CL.Clustering.from_partition(E, ids, [["nobody"]], MIN, MAX, fold_engine=folds)
    with pytest.raises(ValueError):
        CL.Clustering.from_partition(E[:2], [ids[0], ids[0]], [], MIN, MAX, fold_engine=folds)


def test_an_oversized_group_is_held_listed_and_refused():
    E, ids = problem()
    st = CL.Clustering.from_partition(E, ids, [ids[3:5], ids[10:24], ids[30:37]], MIN, MAX, engine=seeded, fold_engine=Folds())
    assert st.clusters[1].Members == ids[10:24] and bits(st.clusters[1].Centroid) == bits(fold_of(st, ids[10:24]))
    assert st.oversized() == [ids[10], ids[30]]
    before = FC.snapshot(st)
    with pytest.raises(_lib.ICLError) as ei:
        st.recluster()
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED and FC.snapshot(st) == before


# ---- split --------------------------------------------------------------------------------------------------------------------------
def oversized_state():
    E, ids = problem()
    return CL.Clustering.from_partition(E, ids, [ids[3:5], ids[10:24], ids[30:37]], MIN, MAX, engine=seeded, fold_engine=Folds()), E, ids


@pytest.mark.parametrize("k_target", [0, 3, 5])
def test_split_is_the_seeded_run_on_the_members(k_target):
    st, E, ids = oversized_state()
    others = [(list(c.Members), bits(c.Centroid)) for c in st.clusters]
    st.split([ids[12]], k_target)
    r = SC.run(E[10:24], np.ones(14, np.int32), 1, MAX, k_target)  # PerformClusteringSeeded on the members, minSize 1
    assert r["status"] == SC.OK
    want = [([ids[10 + s] for s in f[1]], bits(f[3])) for f in r["finals"]]
    if k_target:
        assert len(want) == k_target
    else:
        # splitCluster's own choice (clustering.go:303): (ceil(14 / 6) + 14) / 2 parts, a little over n / 2
        assert len(want) == CL.CalculateOptimalClusters(14, 1, MAX)[0] == 8
    got = [(list(c.Members), bits(c.Centroid)) for c in st.clusters]
    assert got == others[:1] + want + others[2:]  # the parts in the cluster's place
    assert not any(c.Frozen for c in st.clusters) and ids_follow_the_rule(st)
    assert st.oversized() == [ids[30]]


def test_split_of_several_clusters_and_resume():
    st, E, ids = oversized_state()
    st.split([ids[30], ids[11], ids[12], ids[0]], k_target=3)  # two oversized clusters, one named twice, and a singleton (left as it is)
    assert st.oversized() == [] and st.clusters[0].Members == ids[3:5]
    assert sorted(k for c in st.clusters for k in c.Members) == sorted(ids) and ids_follow_the_rule(st)
    assert len(st.clusters) == 1 + 3 + 3 + (N - 2 - 14 - 7)
    assert st.recluster() and sorted(k for c in st.clusters for k in c.Members) == sorted(ids)


def test_split_refusals_leave_the_state_alone():
    st, E, ids = oversized_state()
    st.freeze([ids[31]])
    before = FC.snapshot(st)
    with pytest.raises(ValueError):
        st.split([ids[12], ids[30]])  # the second cluster is frozen: nothing is split
    with pytest.raises(ValueError):
        st.split(["nobody"])
    assert FC.snapshot(st) == before
    st.engine = lambda C, ss, mn, mx, kt: (None, None, 0, _lib.ICL_ERR_CONSTRAINT, None, None)
    with pytest.raises(ValueError):
        st.split([ids[12]])
    st.engine = lambda C, ss, mn, mx, kt: (None, None, 0, _lib.ICL_ERR_HIP, None, None)
    with pytest.raises(_lib.ICLError):
        st.split([ids[12]])
    assert FC.snapshot(st) == before


# ---- workflow.RunMore(remove_ids=) ----------------------------------------------------------------------------------------------------
def test_run_more_removes_before_it_adds():
    E, ids = problem()
    new_rows = WC.mog(4, D - 2, 13, k=2, sigma=0.3)

    class Net:
        ctx = types.SimpleNamespace(embed_files=lambda paths, head, prec, threads: (new_rows.copy(), np.zeros(len(paths), np.int32)))

        def Empty(self):
            return False

    app = types.SimpleNamespace(Net=Net(), Head=0)
    new = (["n%d.jpg" % i for i in range(4)], ["n%d" % i for i in range(4)], [["x"]] * 4, {"x": 0, "y": 1})
    lab = np.concatenate([new_rows, np.tile(np.array([[1.0, 0.0]], np.float32), (4, 1))], axis=1)

    def state():
        return CL.Clustering.start(E, ids, MIN, MAX, engine=seeded, fold_engine=Folds())

    st, ref = state(), state()
    out = WF.RunMore(app, st, new, remove_ids=[ids[2], ids[20]])
    ref.remove([ids[2], ids[20]])
    ref.add(lab, new[1])
    assert ref.recluster()
    assert out == (ref.as_map(), True) and FC.snapshot(st) == FC.snapshot(ref)
    st, ref = state(), state()
    assert WF.RunMore(app, st, new) == WF.RunMore(app, ref, new, remove_ids=None) and FC.snapshot(st) == FC.snapshot(ref)
    before = FC.snapshot(st)
    with pytest.raises(ValueError):
        WF.RunMore(app, st, (new[0], ["m%d" % i for i in range(4)], new[2], new[3]), remove_ids=["nobody"])
    assert FC.snapshot(st) == before
