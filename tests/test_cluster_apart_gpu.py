"""icl_cluster_many_apart (imageclust_amd/csrc/ward_many.hip, DESIGN.md "Constrained seeded clustering"): the seeded loop with a
keep-apart relation that merged clusters inherit.  Bar: cluster ids, seed ranks, cluster count, status, merge log and C_out (as uint32)
equal the checker's (tests/apart_cases.py) and, with no constraint, icl_cluster_many_seeded's, BIT-EXACT.  These routes are exact:
ctx.last_ward_bound_violations is not involved."""
import numpy as np
import pytest

from tests import apart_cases as AC
from tests import seeded_cases as SC
from tests.many_cases import same_results
from tests.test_cluster_seeded_gpu import shape_problems

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def apart(ctx, probs, **kw):
    return ctx.cluster_many_apart(probs, want_merges=True, want_centroids=True, **kw)


def bare(job):
    """a seeded problem as cluster_many_apart takes it, with no constraint"""
    return tuple(job[:5]) + (None, None)


@pytest.fixture(scope="module")
def cases():
    """(name, problem, the checker's result): the case list on both routes, the ties variant, the known answer, the anchored runs"""
    jobs = [("constrained %d x %d" % (m, d), AC.constrained(m, d)) for m in AC.CASES_M + AC.CASES_MID for d in AC.CASES_D]
    jobs += [("ties %d x %d" % (m, 8), AC.constrained(m, 8, seed=200 + m, ties=True)) for m in (64, 256, 300)]
    jobs += [("anchored %d x %d" % (m, 8), AC.anchored(m, 8)) for m in (64, 300)]
    jobs.append(("known answer", AC.KNOWN))
    return [(name, j, AC.run(*j)) for name, j in jobs]


@pytest.mark.parametrize("d", SC.SHAPES_D)
def test_no_constraints_equals_cluster_many_seeded(ctx, d):
    jobs = [j for m in SC.SHAPES_M for j in shape_problems(m, d)]
    want = ctx.cluster_many_seeded(jobs, want_merges=True, want_centroids=True)
    got = apart(ctx, [bare(j) for j in jobs])
    zeros = apart(ctx, [tuple(j[:5]) + (np.zeros(len(j[1]), np.int32), np.zeros((0, 2), np.int32)) for j in jobs])
    for q, (a, b, c) in enumerate(zip(want, got, zeros)):
        same_results(a[:5], b[:5], q)
        same_results(a[:5], c[:5], q)
        assert SC.same_bits(a[5], b[5]) and SC.same_bits(a[5], c[5]), q
    assert sum(len(a[4]) for a in want) > 300


@pytest.mark.parametrize("m,d", ((257, 8), (300, 8)))
def test_no_constraints_on_the_mid_route(ctx, m, d):
    jobs = shape_problems(m, d)[:2]
    want = ctx.cluster_many_seeded(jobs, want_merges=True, want_centroids=True)
    got = apart(ctx, [bare(j) for j in jobs])
    assert ctx.last_many_stats()["mid"] == len(jobs) and ctx.last_many_stats()["small"] == 0
    for q, (a, b) in enumerate(zip(want, got)):
        assert len(a[4]) > m // 8
        same_results(a[:5], b[:5], q)
        assert SC.same_bits(a[5], b[5]), q


def test_constrained_equals_the_checker(ctx, cases):
    res = apart(ctx, [j for _, j, _ in cases])
    st = ctx.last_many_stats()
    assert st["mid"] == sum(len(j[1]) > 256 for _, j, _ in cases) and st["large"] == 0
    for (name, j, ref), r in zip(cases, res):
        AC.same_as_checker(r, ref, name)
        if name.startswith("constrained") and len(ref["log"]) >= 5:   # (the case does constrain: tests/test_cluster_apart_cpu.py counts them)
            assert len(j[6]) > 0
    known = res[-1]
    assert np.array_equal(known[4], AC.KNOWN_LOG) and known[2] == 2


def test_anchored_run_ends_for_want_of_pairs(ctx):
    """k_target 1 asks for m - 1 merges; the anchors never merge with each other, so fewer are made"""
    jobs = [AC.anchored(m, 8, k_target=1) for m in (64, 300)]
    for j, r in zip(jobs, apart(ctx, jobs)):
        m = len(j[1])
        AC.same_as_checker(r, AC.run(*j), m)
        assert r[3] == 0 and 0 < len(r[4]) < m - 1


@pytest.mark.parametrize("m", (31, 32, 33, 63, 64, 65))
def test_word_edges(ctx, m):
    """pairs on the seeds at both ends of every 32-bit word of a row, and one class across the word boundaries"""
    C, ss, mn, mx = SC.mixed_problem(m, 8, 300 + m, frozen_every=0)
    edge = [s for s in (0, 31, 32, 63, 64, m - 1) if s < m]
    base = SC.run(C, ss, mn, mx, 2)["log"]
    # the edge seeds among themselves, and each with the seed the unconstrained run merges it with (so that the pairs bite)
    pairs = [(a, b) for a in edge for b in edge if a < b] + [(int(a), int(b)) for a, b in base if a < m and b < m and (a in edge or b in edge)]
    pairs = np.array(pairs, np.int32).reshape(-1, 2)
    cls = np.zeros(m, np.int32)
    cls[[s for s in (30, 31, 32, 33, 62, 63, 64) if s < m]] = 3
    jobs = [(C, ss, mn, mx, 2, None, pairs), (C, ss, mn, mx, 2, cls, None), (C, ss, mn, mx, 2, cls, pairs[:, ::-1])]
    bites = 0
    for q, (j, r) in enumerate(zip(jobs, apart(ctx, jobs))):
        ref = AC.run(*j)
        assert len(ref["log"]) >= m // 4
        AC.same_as_checker(r, ref, (m, q))
        bites += not np.array_equal(ref["log"], base)
    assert bites >= 2, m   # (the constraints change the run)


def test_cut_and_resume_is_the_same_run(ctx, cases):
    """The state after t merges, with the bans its clusters inherited as pairs, resumed with k_target: the rest of the log, and the uncut
    run's final centroids."""
    jobs, want = [], []
    for name, j, ref in cases:
        if name not in ("constrained 64 x 8", "constrained 255 x 3", "constrained 300 x 8", "ties 300 x 8"):
            continue
        log, m = ref["log"], len(j[1])
        for t in SC.cuts(len(log)):
            C2, ss2, seeds2, ids, pairs2 = AC.state_after(j[0], j[1], log, t, j[5], j[6])
            jobs.append((C2, ss2, j[2], j[3], len(ids) - (len(log) - t), None, pairs2))
            log2 = SC.resumed_log(log, t, ids, m)
            want.append((name, t, log2, SC.centroids_from_log(C2, ss2, log2), ref["C_out"], seeds2))
    assert len(jobs) >= 10 and any(len(j[1]) > 256 for j in jobs)
    for r, (name, t, log2, cen2, full, seeds2) in zip(apart(ctx, jobs), want):
        assert r[3] == 0 and np.array_equal(r[4], log2), (name, t)
        assert SC.same_bits(r[5], cen2), (name, t)
        for q in np.flatnonzero(r[1] == 0):
            assert SC.same_bits(r[5][q], full[seeds2[q][0]]), (name, t, q)


def test_result_does_not_depend_on_the_batch(ctx, cases):
    jobs = [j for _, j, _ in cases]
    base = apart(ctx, jobs)
    plain = [bare(j) for m, d in ((17, 3), (64, 8), (300, 8)) for j in shape_problems(m, d)[:2]]   # unconstrained problems in between
    mixed = [x for pair in zip(jobs, plain * (len(jobs) // len(plain) + 1)) for x in pair]
    perm = np.random.default_rng(4).permutation(len(mixed))
    shuf = apart(ctx, [mixed[i] for i in perm])
    for pos, i in enumerate(perm):
        if i % 2 == 0:
            same_results(base[i // 2][:5], shuf[pos][:5], i)
            assert SC.same_bits(base[i // 2][5], shuf[pos][5]), i
    alone = apart(ctx, [jobs[0]])[0]
    same_results(base[0][:5], alone[:5], 0)


def test_dev_equals_host(ctx, cases):
    jobs = [j for _, j, _ in cases]
    for q, (a, b) in enumerate(zip(apart(ctx, jobs), apart(ctx, jobs, dev=True))):
        same_results(a[:5], b[:5], q)
        assert SC.same_bits(a[5], b[5]), q


def test_failed_problems_and_bad_arguments(ctx):
    from imageclust_amd import _lib

    good, other = AC.constrained(33, 8), AC.constrained(17, 3)
    big = (np.zeros((2049, 1), np.float32), np.ones(2049, np.int32), 1, 4, 0, None, np.array([[0, 2048]], np.int32))
    res = apart(ctx, [good, big, other])
    assert [r[3] for r in res] == [0, _lib.ICL_ERR_UNSUPPORTED, 0]
    AC.same_as_checker(res[0], AC.run(*good), "before the refused problem")
    AC.same_as_checker(res[2], AC.run(*other), "behind the refused problem")
    r = res[1]
    assert (r[0] == -1).all() and (r[1] == -1).all() and r[2] == 0 and len(r[4]) == 0 and not r[5].any()

    # argument errors: ICL_ERR_ARG, nothing written
    two = (good, other)
    pk = _lib.pack_many([(j[0], j[2], j[3]) for j in two])
    ss = np.concatenate([j[1] for j in two]).astype(np.int32)
    cls = np.concatenate([j[5] for j in two]).astype(np.int32)
    pairs = np.concatenate([j[6] for j in two]).astype(np.int32)
    off = np.array([0, len(good[6]), len(good[6]) + len(other[6])], np.int64)
    assert len(good[6]) > 0 and len(other[6]) > 0
    L, h = ctx.L, ctx.h
    arr = lambda a: None if a is None else a.ctypes.data

    def call(cls=cls, off=off, pairs=pairs):
        outs = [np.full(200, 777, np.int32) for _ in range(6)]
        co = np.full(pk["E"].size, 777.0, np.float32)
        rc = L.icl_cluster_many_apart(h, 2, arr(pk["E"]), pk["E"].size, arr(pk["e_off"]), arr(pk["n"]), arr(pk["d"]), arr(ss), arr(pk["min_size"]),
                                      arr(pk["max_size"]), None, arr(cls), arr(off), arr(pairs), arr(outs[0]), arr(outs[1]), arr(outs[2]),
                                      arr(outs[3]), arr(outs[4]), arr(outs[5]), arr(co))
        return rc, all((o == 777).all() for o in outs) and bool((co == 777.0).all())

    def changed(a, at, v):
        a = a.copy()
        a.reshape(-1)[at] = v
        return a

    assert call() == (0, False)                      # the well-formed call writes
    assert call(cls=None) == (0, False) and call(off=None, pairs=None) == (0, False)
    n0 = 2 * len(good[6])                            # the first int of problem 1's pairs
    bad = dict(index_m=changed(pairs, 0, 33), index_of_the_other_problem=changed(pairs, n0, 17), negative_index=changed(pairs, 1, -1),
               same_seed=changed(pairs, n0 + 1, pairs[len(good[6]), 0]))
    for name, p in bad.items():
        assert call(pairs=p) == (_lib.ICL_ERR_ARG, True), name
    assert call(cls=changed(cls, 40, -1)) == (_lib.ICL_ERR_ARG, True)
    assert call(off=changed(off, 0, -1)) == (_lib.ICL_ERR_ARG, True)
    assert call(off=changed(off, 1, off[2] + 1)) == (_lib.ICL_ERR_ARG, True)     # decreasing
    assert call(pairs=None) == (_lib.ICL_ERR_ARG, True)
    assert call(off=None) == (_lib.ICL_ERR_ARG, True)
    assert L.icl_cluster_many_apart(h, 0, None, 0, *([None] * 17)) == 0
    with pytest.raises(_lib.ICLError) as ei:
        ctx.cluster_many_apart([tuple(good[:6]) + (np.array([[0, 33]], np.int32),)])
    assert ei.value.code == _lib.ICL_ERR_ARG


def test_clustering_state_on_the_gpu(ctx):
    """Clustering.start -> keep_apart -> recluster -> absorb_leftovers on the GPU equals the same state over the checker."""
    from imageclust_amd import clustering
    from tests import ward_cases as WC
    from tests.test_cluster_apart_cpu import engine_with

    E = WC.mog(47, 6, 5, k=5, sigma=0.3)
    ids = ["img_%d" % i for i in range(47)]
    states = [clustering.Clustering.start(E[:40], ids[:40], 4, 6, ctx=ctx), clustering.Clustering.start(E[:40], ids[:40], 4, 6, engine=engine_with([]))]
    for st in states:
        st.add(E[40:], ids[40:])
        big = next(c for c in st.clusters if len(c.Members) >= 3)
        keys = big.Members[:2]
        st.dissolve(keys[:1])
        st.keep_apart(keys)
        assert st.recluster()
        st.absorb_leftovers()
    a, b = states
    assert a.as_map() == b.as_map() and np.array_equal(a.last_merges, b.last_merges) and len(a.last_merges) > 0
    assert all(SC.same_bits(x.Centroid, y.Centroid) for x, y in zip(a.clusters, b.clusters))
    cen, ss = b.seeds()
    (cid, rank, nc, mg, co), ok = clustering.PerformClusteringSeeded(cen, ss, 4, 6, k_target=max(1, len(ss) - 2), ctx=ctx, apart_pairs=b._apart_pairs())
    ref = AC.run(cen, ss, 4, 6, max(1, len(ss) - 2), None, b._apart_pairs())
    assert ok and np.array_equal(mg, ref["log"]) and np.array_equal(cid, ref["cluster_id"]) and SC.same_bits(co, ref["C_out"])
