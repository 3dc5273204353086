"""Constrained seeded clustering without a GPU (DESIGN.md "Constrained seeded clustering"): the checker of tests/apart_cases.py against
tests/seeded_cases.run and a hand-derived answer, that its cases tell a kernel that inherits bans from one that does not,
imageclust_amd/csrc/apart_bits.h in a stand-alone program under the address and undefined-behaviour sanitizers, and
Clustering.keep_apart / keep_together / absorb_leftovers with the checker standing in for the GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import apart_cases as AC
from tests import seeded_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["random tables", "word edges", "refusals"]
LIMIT_S = 300


def same(a, b):
    return (a["status"] == b["status"] and np.array_equal(a["cluster_id"], b["cluster_id"]) and np.array_equal(a["seed_rank"], b["seed_rank"])
            and a["n_clusters"] == b["n_clusters"] and np.array_equal(a["log"], b["log"]) and SC.same_bits(a["C_out"], b["C_out"]))


@pytest.mark.parametrize("d", (3, 8))
def test_no_constraints_is_the_seeded_checker(d):
    for m in SC.SHAPES_M:
        C, ss, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
        for kt in (0, max(1, m // 4)):
            ref = SC.run(C, ss, mn, mx, kt)
            assert same(AC.run(C, ss, mn, mx, kt), ref), (m, d, kt)
            assert same(AC.run(C, ss, mn, mx, kt, np.zeros(m, np.int32), np.zeros((0, 2), np.int32)), ref), (m, d, kt)


def test_known_answer():
    """Singletons at 0, 1, 2.1, 10 with (0, 2) apart: merge (1, 0) -> 4, which inherits the ban with 2; d(4, 3) = 2/3 * 90.25 is above
    d(2, 3) = 31.205, so (3, 2) -> 5, which inherits the ban with 4; nothing is left to merge: 2 merges of the 3 asked.  Without
    inheritance the second merge is (4, 2) at 2/3 * 2.56."""
    r = AC.run(*AC.KNOWN)
    assert r["status"] == AC.OK and np.array_equal(r["log"], AC.KNOWN_LOG) and len(r["finals"]) == 2
    assert np.array_equal(r["cluster_id"], [0, 0, 1, 1]) and np.array_equal(r["seed_rank"], [1, 0, 1, 0])   # Merge(a, b): a's seeds first
    assert SC.same_bits(r["C_out"], np.array([[0.0], [0.5], [0.0], [np.float32(12.1) / np.float32(2)]], np.float32))
    loose = AC.run(*AC.KNOWN, inherit=False)
    assert loose["log"].tolist() == [[1, 0], [4, 2], [5, 3]]
    assert SC.run(*AC.KNOWN[:5])["log"].tolist()[0] == [1, 0]


def test_the_cases_separate_inheritance():
    """At least three quarters of the cases with five merges or more differ from the unconstrained log, and as many from the log of a
    checker that bans at the start only (measured: 10 of 10 and 9 of 10 with m = 300 included; the anchored runs end for want of pairs)."""
    n = diff = dinh = early = 0
    for m in AC.CASES_M + AC.CASES_MID:
        for d in AC.CASES_D:
            job = AC.constrained(m, d)
            a, plain, loose = AC.run(*job), SC.run(*job[:5]), AC.run(*job, inherit=False)
            if len(plain["log"]) < 5:
                continue
            n += 1
            diff += not np.array_equal(a["log"], plain["log"])
            dinh += not np.array_equal(a["log"], loose["log"])
            anc = AC.anchored(m, d)
            r = AC.run(*anc)
            early += len(r["finals"]) > anc[4]
            cls = anc[5]   # no final cluster holds two anchors
            assert all(sum(int(cls[s]) for s in f[1]) <= 1 for f in r["finals"]), (m, d)
            for f in a["finals"]:   # ... and no final cluster holds an apart pair
                B = AC.relation(m, job[5], job[6])
                assert not B[np.ix_(f[1], f[1])].any(), (m, d)
    assert n >= 8 and 4 * diff >= 3 * n and 4 * dinh >= 3 * n and 4 * early >= 3 * n, (n, diff, dinh, early)


def test_cut_and_resume_is_the_same_run():
    for m, d in ((17, 3), (64, 8)):
        job = AC.constrained(m, d)
        full = AC.run(*job)
        k = m - len(full["log"])  # (what the full run stopped at; the item total and so CalculateOptimalClusters' k stay, too)
        for t in SC.cuts(len(full["log"])):
            C2, ss2, seeds2, ids, pairs2 = AC.state_after(job[0], job[1], full["log"], t, job[5], job[6])
            r = AC.run(C2, ss2, job[2], job[3], len(ids) - (len(full["log"]) - t), None, pairs2)
            assert np.array_equal(r["log"], SC.resumed_log(full["log"], t, ids, m)), (m, d, t, k)


# ---- the same host code under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("apart_bits") / "apart_bits")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "apart_bits_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_bit_rows_and_refusals_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


# ---- the Python layer, with the checker standing in for the GPU ---------------------------------------------------------------
def engine_with(calls):
    def engine(C, ss, mn, mx, kt, *extra):
        calls.append(extra)
        r = AC.run(C, ss, mn, mx, kt, *extra)
        return r["cluster_id"], r["seed_rank"], r["n_clusters"], r["status"], r["log"], r["C_out"]
    return engine


def five_argument_engine(C, ss, mn, mx, kt):
    r = SC.run(C, ss, mn, mx, kt)
    return r["cluster_id"], r["seed_rank"], r["n_clusters"], r["status"], r["log"], r["C_out"]


def test_keep_apart_and_keep_together_through_the_stand_in():
    from imageclust_amd import clustering as CL
    from tests import ward_cases as WC

    E = WC.mog(40, 6, 11, k=5, sigma=0.25)
    ids = ["i%d" % i for i in range(40)]
    plain = CL.Clustering.start(E, ids, 3, 6, engine=five_argument_engine)   # an unconstrained state never passes the two extra arguments
    calls = []
    st = CL.Clustering.start(E, ids, 3, 6, engine=engine_with(calls))
    assert calls == [()] and st.as_map() == plain.as_map() and st.constraints() == {"apart": [], "apart_clusters": [], "frozen": []}
    big = next(c for c in st.clusters if len(c.Members) >= 3)
    a, b, c = big.Members[:3]
    with pytest.raises(ValueError):
        st.keep_apart([a, b])   # they share a cluster
    st.dissolve([a])
    st.keep_apart([a, b, c])
    st.keep_apart([a])          # a group of one holds nothing
    assert st.constraints()["apart"] == [[a, b, c]] and len(st.constraints()["apart_clusters"]) == 3
    seeds_before = st.seeds()
    members = [list(h.Members) for h in st.clusters]
    pairs = st._apart_pairs()
    assert st.recluster()
    assert len(calls) == 2 and calls[1][0] is None and calls[1][1].tolist() == [list(p) for p in pairs]
    ref = AC.run(seeds_before[0], seeds_before[1], 3, 6, 0, None, pairs)
    assert np.array_equal(st.last_merges, ref["log"])
    assert [h.Members for h in st.clusters] == [[k for s in f[1] for k in members[s]] for f in ref["finals"]]
    where = {k: i for i, h in enumerate(st.clusters) for k in h.Members}
    assert len({where[a], where[b], where[c]}) == 3           # held per image id: it survived the merges
    assert not np.array_equal(ref["log"], SC.run(seeds_before[0], seeds_before[1], 3, 6)["log"])   # (and it changed the run)

    # keep_together: MergeClusters' rule on the host, refusals leave the state as it was
    before = [(list(h.Members), h.Centroid.copy()) for h in st.clusters]
    with pytest.raises(ValueError, match="keep-apart"):
        st.keep_together([a, b])
    full = [h for h in st.clusters if len(h.Members) >= 4][:2]
    with pytest.raises(ValueError, match="maxSize"):
        st.keep_together([full[0].Members[0], full[1].Members[0]])
    assert [(list(h.Members), h.Centroid.tolist()) for h in st.clusters] == [(m, c.tolist()) for m, c in before]
    size = lambda i: len(st.clusters[i].Members)
    lone = min((where[k] for k in (a, b, c)), key=size)   # the smallest of the three and the first cluster that may take it
    mate = next(i for i in range(len(st.clusters)) if i != lone and size(i) + size(lone) <= 6 and (min(i, lone), max(i, lone)) not in st._apart_pairs())
    x, y = sorted((lone, mate))
    hx, hy, n_before = st.clusters[x], st.clusters[y], len(st.clusters)
    st.keep_together([hy.Members[0], hx.Members[0]])
    got = st.clusters[x]
    assert got.Members == hx.Members + hy.Members and len(st.clusters) == n_before - 1
    assert SC.same_bits(got.Centroid, O.merge_centroid(hx.Centroid, len(hx.Members), hy.Centroid, len(hy.Members)))
    assert sorted(st.as_map()) == list(range(len(st.as_map()))) and all(len(v) >= 3 for v in st.as_map().values())
    assert len({k: i for i, h in enumerate(st.clusters) for k in h.Members}) == 40
    st.keep_together([a])   # one cluster: nothing to do
    assert len(st.clusters) == n_before - 1


def test_absorb_leftovers_through_the_stand_in():
    from imageclust_amd import clustering as CL
    from tests import ward_cases as WC

    E = WC.mog(50, 5, 3, k=6, sigma=0.4)
    ids = ["p%d" % i for i in range(50)]
    calls = []
    st = CL.Clustering.start(E, ids, 4, 6, engine=engine_with(calls))
    st.add(WC.mog(7, 5, 4, k=2, sigma=0.4), ["q%d" % i for i in range(7)])    # leftovers: new singletons ...
    kept = [list(h.Members) for h in st.clusters if len(h.Members) >= 4]
    loose = [k for h in st.clusters if len(h.Members) < 4 for k in h.Members]
    assert len(kept) >= 3 and len(loose) >= 7
    frozen_key = kept[0][0]
    st.freeze([frozen_key])
    seeds_before, members = st.seeds(), [list(h.Members) for h in st.clusters]
    left = st.absorb_leftovers()
    cls, pairs = calls[-1]
    assert pairs.shape == (0, 2) and cls.tolist() == [int(len(m) >= 4 and m[0] != frozen_key) for m in members]
    ref = AC.run(seeds_before[0], seeds_before[1], 4, 6, len(kept), cls, None)
    assert np.array_equal(st.last_merges, ref["log"]) and len(ref["log"]) > 0
    where = {k: i for i, h in enumerate(st.clusters) for k in h.Members}
    assert len({where[m[0]] for m in kept}) == len(kept)         # no two formerly kept clusters share a cluster
    for m in kept:
        assert len({where[k] for k in m}) == 1                   # ... and each is whole
    assert st.clusters[where[frozen_key]].Members == kept[0]     # the frozen one took nothing
    assert sorted(left) == sorted(k for h in st.clusters if len(h.Members) < 4 for k in h.Members)
    assert set(left) <= set(loose) and len(left) < len(loose)
    n_calls = len(calls)
    full = CL.Clustering.start(E[:12], ids[:12], 1, 6, engine=engine_with(calls))
    assert full.absorb_leftovers() == [] and len(calls) == n_calls + 1      # nothing is dropped: no further call


def test_perform_clustering_seeded_refuses_constraints_above_the_cap():
    from imageclust_amd import _lib
    from imageclust_amd import clustering as CL

    m = CL.MANY_SEEDED_MAX + 1
    with pytest.raises(_lib.ICLError) as ei:
        CL.PerformClusteringSeeded(np.zeros((m, 1), np.float32), np.ones(m, np.int32), 1, 4, ctx=object(), apart_pairs=[(0, 1)])
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
