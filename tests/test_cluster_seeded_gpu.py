"""icl_cluster_many_seeded (imageclust_amd/csrc/ward_many.hip, DESIGN.md "Seeded clustering"): the clustering loop started from
existing clusters.  Bar: cluster ids, seed ranks, cluster count, status, merge log and C_out (as uint32) equal the checker's
(tests/seeded_cases.py: the reference's loop over the oracle's primitives) and, from all-ones seeds, icl_cluster_many's, BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

from tests import seeded_cases as SC
from tests import ward_cases as WC
from tests.many_cases import same_results, serving_problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def seeded(ctx, probs, **kw):
    return ctx.cluster_many_seeded(probs, want_merges=True, want_centroids=True, **kw)


def ones(E):
    return np.ones(len(E), np.int32)


def shape_problems(m, d):
    """mixed sizes, frozen seeds, seeds at max_size, duplicates; then exact ties with a k_target that asks for more merges than the
    sizes allow (the loop ends for want of pairs); k_target above m; everything merges into one cluster; the same with the frozen seeds
    kept and a max_size far above the item total (only the frozen flag stands between those seeds and a merge)"""
    C1, s1, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
    C2, s2, _, _ = SC.mixed_problem(m, d, 200 + m + d, ties=True)
    return [(C1, s1, mn, mx, 0), (C2, s2, mn, mx, max(1, m // 4)), (C1, s1, mn, mx, m + 3), (C1, np.abs(s1).clip(1, 2).astype(np.int32), 1, 40, 1),
            (C1, (np.sign(s1) * np.abs(s1).clip(1, 2)).astype(np.int32), 1, 1000000, 1)]


@pytest.fixture(scope="module")
def all_ones(ctx):
    """(problems as icl_cluster_many takes them, its results, the seeded call's results from all-ones seeds): the small cases, then
    200 request-shape problems"""
    probs = [(E, mn, mx) for _, E, mn, mx in WC.small_cases()] + serving_problems(200, 20261019, dup_every=37)
    many = ctx.cluster_many(probs, want_merges=True)
    got = seeded(ctx, [(E, ones(E), mn, mx) for E, mn, mx in probs])
    return probs, many, got


def test_all_ones_equals_cluster_many(all_ones):
    probs, many, got = all_ones
    for p, (pr, a, b) in enumerate(zip(probs, many, got)):
        same_results(a, b[:5], p)
        if a[3] == 0:
            assert SC.same_bits(b[5], SC.centroids_from_log(pr[0], ones(pr[0]), a[4])), p
        else:
            assert not b[5].any(), p


def test_resume_reproduces_the_rest_of_the_log(ctx, all_ones):
    """States cut after the first merge, at the middle and before the last merge, seeded back with k_target: the rest of the log (ids
    mapped as in the checker) and the same final centroids.  ties600 and mog_333 resume on the mid route."""
    probs, many, _ = all_ones
    jobs, want = [], []
    for p in list(range(len(WC.small_cases()))) + list(range(len(probs) - 12, len(probs))):
        (E, mn, mx), log = probs[p], many[p][4]
        if many[p][3] != 0:
            continue
        for t in SC.cuts(len(log)):
            C2, ss2, seeds2, ids = SC.state_after(E, ones(E), log, t)
            jobs.append((C2, ss2, mn, mx, len(ids) - (len(log) - t)))
            log2 = SC.resumed_log(log, t, ids, len(E))
            want.append((p, t, log2, SC.centroids_from_log(C2, ss2, log2), SC.centroids_from_log(E, ones(E), log), seeds2))
    assert len(jobs) >= 100
    for r, (p, t, log2, cen2, full, seeds2) in zip(seeded(ctx, jobs), want):
        assert r[3] == 0 and np.array_equal(r[4], log2), (p, t)
        assert SC.same_bits(r[5], cen2), (p, t)
        # ... and those centroids are the uncut run's: the resumed cluster whose first seed is q starts with the uncut run's item seeds2[q][0]
        for q in np.flatnonzero(r[1] == 0):
            assert SC.same_bits(r[5][q], full[seeds2[q][0]]), (p, t, q)


@pytest.mark.parametrize("d", SC.SHAPES_D)
def test_mixed_seeds_equal_the_checker(ctx, d):
    jobs = [j for m in SC.SHAPES_M for j in shape_problems(m, d)]
    jobs.append((np.zeros((0, d), np.float32), np.zeros(0, np.int32), 1, 2, 1))
    res = seeded(ctx, jobs)
    merged = 0
    for q, (j, r) in enumerate(zip(jobs, res)):
        ref = SC.run(*j)
        SC.same_as_checker(r, ref, (d, q, len(j[1])))
        merged += len(ref["log"])
    assert merged > 300


@pytest.mark.parametrize("m,d", SC.MID_SHAPES)
def test_mid_route_equals_the_checker(ctx, m, d):
    jobs = shape_problems(m, d)[:2]
    res = seeded(ctx, jobs)
    assert ctx.last_many_stats()["mid"] == len(jobs) and ctx.last_many_stats()["small"] == 0
    for q, (j, r) in enumerate(zip(jobs, res)):
        ref = SC.run(*j)
        assert len(ref["log"]) > m // 8
        SC.same_as_checker(r, ref, (m, d, q))


def test_result_does_not_depend_on_the_batch(ctx):
    from imageclust_amd import _lib

    jobs = [j for m, d in [(17, 3), (64, 8), (40, 1037), (255, 8), (300, 8), (3, 8)] for j in shape_problems(m, d)[:2]]
    plain = [(E, ones(E), mn, mx) for E, mn, mx in serving_problems(6, 5)]  # unseeded-shape problems in between
    base = seeded(ctx, jobs)
    mixed = jobs + plain
    perm = np.random.default_rng(2).permutation(len(mixed))
    shuf = seeded(ctx, [mixed[i] for i in perm])
    for pos, i in enumerate(perm):
        if i < len(jobs):
            same_results(base[i], shuf[pos], i)
    for i in range(len(jobs)):
        alone = seeded(ctx, [jobs[i]])[0]
        same_results(base[i], alone, i)
        st = ctx.last_many_stats()  # a lone problem stays on its one-workgroup route, whatever the mid-route policy
        assert st["large"] == 0 and st["small"] + st["mid"] <= 1
    ctx.set_many_options(_lib.MANY_MID_OFF)
    try:
        off = seeded(ctx, jobs)
    finally:
        ctx.set_many_options(_lib.MANY_MID_AUTO)
    for i, (a, b) in enumerate(zip(base, off)):
        same_results(a, b, i)


def test_failed_problems_and_bad_arguments(ctx):
    from imageclust_amd import _lib

    good = shape_problems(33, 8)[0]
    big = np.array(good[1], copy=True)
    big[0] = good[3] + 1  # a seed above max_size that is not frozen
    jobs = [good, (good[0], big, good[2], good[3], 0), shape_problems(64, 3)[1],
            (np.zeros((2049, 1), np.float32), np.ones(2049, np.int32), 1, 4, 0), shape_problems(17, 8)[0],
            (good[0][:2], np.array([1, 1], np.int32), 3, 6, 0), shape_problems(40, 8)[1]]
    res = seeded(ctx, jobs)
    assert [r[3] for r in res] == [0, _lib.ICL_ERR_UNSUPPORTED, 0, _lib.ICL_ERR_UNSUPPORTED, 0, _lib.ICL_ERR_CONSTRAINT, 0]
    for q, (j, r) in enumerate(zip(jobs, res)):
        if r[3] == 0:
            same_results(r, seeded(ctx, [j])[0], q)  # the neighbours of a failed problem are untouched
        else:
            assert (r[0] == -1).all() and (r[1] == -1).all() and r[2] == 0 and len(r[4]) == 0 and not r[5].any(), q
    with pytest.raises(_lib.ICLError) as ei:
        ctx.cluster_many_seeded(jobs, raise_on_error=True)
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED and "problem 1:" in str(ei.value)

    # argument errors: ICL_ERR_ARG, nothing written
    pk = _lib.pack_many([(j[0], j[2], j[3]) for j in (good, jobs[2])])
    ss = np.concatenate([good[1], jobs[2][1]]).astype(np.int32)
    L, h = ctx.L, ctx.h
    arr = lambda a: a.ctypes.data

    def call(nprob=2, E=True, e_len=None, m=None, seed=ss, cid=True):
        outs = [np.full(200, 777, np.int32) for _ in range(6)]
        co = np.full(pk["E"].size, 777.0, np.float32)
        rc = L.icl_cluster_many_seeded(h, nprob, arr(pk["E"]) if E else None, pk["E"].size if e_len is None else e_len, arr(pk["e_off"]),
                                       arr(pk["n"] if m is None else m), arr(pk["d"]), arr(seed) if seed is not None else None,
                                       arr(pk["min_size"]), arr(pk["max_size"]), None, arr(outs[0]) if cid else None, arr(outs[1]),
                                       arr(outs[2]), arr(outs[3]), arr(outs[4]), arr(outs[5]), arr(co))
        return rc, all((o == 777).all() for o in outs) and bool((co == 777.0).all())

    assert call() == (0, False)  # the well-formed call writes
    zero = ss.copy()
    zero[40] = 0
    assert call(seed=zero) == (_lib.ICL_ERR_ARG, True)
    assert call(seed=None) == (_lib.ICL_ERR_ARG, True)
    assert call(nprob=-1) == (_lib.ICL_ERR_ARG, True)
    assert call(E=False) == (_lib.ICL_ERR_ARG, True)
    assert call(cid=False) == (_lib.ICL_ERR_ARG, True)
    assert call(e_len=pk["E"].size - 1) == (_lib.ICL_ERR_ARG, True)
    assert call(m=np.array([33, -1], np.int32)) == (_lib.ICL_ERR_ARG, True)
    assert L.icl_cluster_many_seeded(h, 0, None, 0, *([None] * 14)) == 0


def test_dev_equals_host(ctx):
    jobs = [j for m, d in [(17, 3), (64, 8), (64, 1037), (256, 8), (257, 8), (1, 8)] for j in shape_problems(m, d)[:2]]
    host = seeded(ctx, jobs)
    dev = seeded(ctx, jobs, dev=True)
    for q, (a, b) in enumerate(zip(host, dev)):
        same_results(a, b, q)


def test_clustering_state_on_the_gpu(ctx):
    """Clustering.start -> add -> freeze -> recluster on 20 + 7 rows equals the checker."""
    from imageclust_amd import clustering

    E = WC.mog(27, 6, 5, k=4, sigma=0.2)
    ids = ["img_%d" % i for i in range(27)]
    st = clustering.Clustering.start(E[:20], ids[:20], 3, 6, ctx=ctx)
    assert st.ok and (st.as_map(), True) == clustering.PerformClusteringWithConstraints(E[:20], ids[:20], 3, 6, ctx=ctx)
    st.add(E[20:], ids[20:])
    st.freeze([st.clusters[0].Members[0]])
    Cs, ss = st.seeds()
    members = [list(c.Members) for c in st.clusters]
    assert st.recluster()
    ref = SC.run(Cs, ss, 3, 6)
    assert len(ref["log"]) > 0 and np.array_equal(st.last_merges, ref["log"])
    assert [c.Members for c in st.clusters] == [[k for s in f[1] for k in members[s]] for f in ref["finals"]]
    for c, f in zip(st.clusters, ref["finals"]):
        assert SC.same_bits(c.Centroid, f[3])
    (cid, rank, nc, mg, co), ok = clustering.PerformClusteringSeeded(Cs, ss, 3, 6, ctx=ctx)
    assert ok and np.array_equal(cid, ref["cluster_id"]) and np.array_equal(rank, ref["seed_rank"]) and nc == ref["n_clusters"]
    assert st.as_map() == {i: [k for s in f[1] for k in members[s]] for i, f in enumerate(f for f in ref["finals"] if f[2] >= 3)}
