"""icl_cluster_apart[_dev] (imageclust_amd/csrc/ward.hip, DESIGN.md "Constrained seeded clustering, large N"): one constrained seeded
problem on the large-N engine's one-merge-per-step exact loop, any number of seeds.  Bar: cluster ids, seed ranks, cluster count, status,
merge log, merge values and C_out (floats as uint32) equal the cap-free checker's (tests/apart_large_cases.py), icl_cluster_many_apart's
up to 2 048 seeds and, with no constraint, icl_cluster_seeded's, BIT-EXACT."""
import ctypes as CT
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import apart_cases as AC
from tests import apart_large_cases as AL
from tests import seeded_cases as SC
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """(kind, m, d) -> (problem, the checker's result), computed once"""
    memo = {}

    def get(kind, m, d):
        if (kind, m, d) not in memo:
            job = AL.case(kind, m, d)
            memo[(kind, m, d)] = (job, AL.run(*job))
        return memo[(kind, m, d)]
    return get


def apart_mode(ctx):
    from imageclust_amd import _lib

    assert _lib.ROWS_SINGLE_APART == AL.ROWS_SINGLE_APART
    return ctx.last_ward_mode() == (_lib.ROWS_SINGLE_APART, False) and ctx.last_ward_bound_violations() == 0


@pytest.mark.parametrize("d", AL.SHAPES_D)
def test_equals_the_checker_and_the_many_call(ctx, refs, d):
    """AC.constrained and AC.anchored on every shape, host and _dev form: the checker's result with its merge values, and
    icl_cluster_many_apart's (small route up to 256 seeds, mid route at 300).  The shapes cross the table's word boundaries, the 64-slot
    seam of the update kernel, recycled row storage (more than WB_K merges) and both ways of launching the steps."""
    from imageclust_amd import _lib

    merged = recycled = replayed = direct = 0
    for m in AL.SHAPES_M:
        for kind in ("constrained", "anchored"):
            job, ref = refs(kind, m, d)
            r = AL.large(ctx, job)
            AL.same_as_checker(r, ref, (kind, m, d), ctx.last_merge_values())
            assert apart_mode(ctx), (kind, m, d)
            assert ctx.last_ward_stats()["merges"] == len(ref["log"])
            rd = AL.large(ctx, job, dev=True)
            AL.same_as_checker(rd, ref, (kind, m, d, "dev"), ctx.last_merge_values())
            AL.same_tuple(r, AL.many(ctx, job), (kind, m, d, "many"))
            k = job[4] or _lib.calc_optimal_clusters(int(np.abs(job[1]).sum()), job[2], job[3])[0]
            asked = max(0, m - k) if ref["status"] == 0 else 0
            merged += len(ref["log"])
            recycled += len(ref["log"]) > AL.WB_K
            replayed += asked >= AL.GRAPH_MERGES and len(ref["log"]) > AL.WB_K
            direct += asked < AL.GRAPH_MERGES and len(ref["log"]) > AL.WB_K
    print("d = %d: %d merges, %d cases past WB_K, %d on replayed steps, %d on direct launches" % (d, merged, recycled, replayed, direct))
    assert merged > 300 and recycled >= 6 and direct >= 3, (merged, recycled, replayed, direct)   # (replay: the test below asks for it by k_target)


def test_captured_steps_replay_under_constraints(ctx, refs):
    """m = 300 with a small k_target asks for at least 2 x GRAPH_STEPS merges: the steps -- update under the relation, commit, finish --
    are replayed from the captured graph, twice over (the second call finds the graph in place)"""
    job, _ = refs("constrained", 300, 8)
    job = job[:4] + (300 // 8,) + job[5:]
    ref = AL.run(*job)
    assert 300 - job[4] >= AL.GRAPH_MERGES and len(ref["log"]) > AL.GRAPH_MERGES // 2
    for rep in range(2):
        AL.same_as_checker(AL.large(ctx, job), ref, rep, ctx.last_merge_values())
    AL.same_tuple(AL.large(ctx, job, dev=True), AL.many(ctx, job), "many")
    assert not np.array_equal(ref["log"], SC.run(*job[:5])["log"])   # (the constraints bite)


@pytest.mark.parametrize("d", AL.SHAPES_D)
def test_no_constraint_equals_the_seeded_call(ctx, d):
    """apart_class all zero with no pair, and both NULL: icl_cluster_seeded's results (there the batched loop, here one merge per step)"""
    shapes = [(m, d) for m in AL.SHAPES_M] + ([AL.ABOVE_CAP] if d == AL.ABOVE_CAP[1] else [])
    merged = 0
    for m, dd in shapes:
        C, ss, mn, mx = SC.mixed_problem(m, dd, 100 + m + dd)
        want = ctx.cluster_seeded(C, ss, mn, mx, 0)
        vals = ctx.last_merge_values()
        for cls, pairs in ((np.zeros(m, np.int32), np.zeros((0, 2), np.int32)), (None, None)):
            got = ctx.cluster_apart(C, ss, mn, mx, 0, cls, pairs)
            AL.same_tuple(want, got, (m, dd))
            assert np.array_equal(vals.view(np.uint32), ctx.last_merge_values().view(np.uint32)), (m, dd)
            assert apart_mode(ctx)
        merged += len(want[4])
    assert merged > 300


@pytest.mark.parametrize("kind", ("constrained", "anchored"))
def test_above_the_cap(ctx, kind):
    """2 100 seeds, where icl_cluster_many_apart refuses: 200 merges against the cap-free checker, host and _dev form"""
    from imageclust_amd import _lib

    job = AL.above_cap(kind)
    ref = AL.run(*job)
    assert len(job[1]) > SC.MAX_SEEDS and len(ref["log"]) > AL.ABOVE_CAP_MERGES // 2
    assert AL.many(ctx, job)[3] == _lib.ICL_ERR_UNSUPPORTED
    for dev in (False, True):
        AL.same_as_checker(AL.large(ctx, job, dev=dev), ref, (kind, dev), ctx.last_merge_values())
        assert apart_mode(ctx)
    if kind == "constrained":
        assert len(job[6]) > 0 and not np.array_equal(ref["log"], AL.run(*job[:5])["log"])
    else:   # no final cluster holds two anchors
        assert all(sum(int(job[5][s]) for s in f[1]) <= 1 for f in ref["finals"])


def test_cut_and_resume_is_the_same_run(ctx, refs):
    """The state after t merges (the first, the middle, before the last) with the bans its clusters inherited as pairs, resumed with
    k_target: the rest of the log, the rest of the merge values and the uncut run's final centroids."""
    n = 0
    for m, d in ((64, 8), (255, 3), (300, 8)):
        job, ref = refs("constrained", m, d)
        log = ref["log"]
        for t in SC.cuts(len(log)):
            C2, ss2, seeds2, ids, pairs2 = AC.state_after(job[0], job[1], log, t, job[5], job[6])
            r = AL.large(ctx, (C2, ss2, job[2], job[3], len(ids) - (len(log) - t), None, pairs2))
            log2 = SC.resumed_log(log, t, ids, m)
            assert r[3] == 0 and np.array_equal(r[4], log2), (m, d, t)
            assert np.array_equal(ctx.last_merge_values().view(np.uint32), ref["values"][t:].view(np.uint32)), (m, d, t)
            assert SC.same_bits(r[5], SC.centroids_from_log(C2, ss2, log2)), (m, d, t)
            for q in np.flatnonzero(r[1] == 0):
                assert SC.same_bits(r[5][q], ref["C_out"][seeds2[q][0]]), (m, d, t, q)
            n += 1
    assert n >= 8


def test_the_cases_separate_inheritance(ctx, refs):
    """Over the (m, d) where it is on record (10 of 10 and 9 of 10): the constrained log differs from the unconstrained one, and from the
    log of a loop that bans at the start only, in at least three quarters of the cases"""
    n = diff = dinh = 0
    for m in AC.CASES_M + AC.CASES_MID:
        for d in AC.CASES_D:
            job, _ = refs("constrained", m, d)
            got = AL.large(ctx, job)[4]
            plain = ctx.cluster_seeded(*job[:5])[4]
            loose = AC.run(*job, inherit=False)["log"]
            n += 1
            diff += not np.array_equal(got, plain)
            dinh += not np.array_equal(got, loose)
    print("separation: %d cases, %d differ from the unconstrained log, %d from inherit=False" % (n, diff, dinh))
    assert n == 10 and 4 * diff >= 3 * n and 4 * dinh >= 3 * n, (n, diff, dinh)


def test_rule_edges(ctx):
    known = AL.large(ctx, AC.KNOWN)
    assert np.array_equal(known[4], AC.KNOWN_LOG) and known[2] == 2 and known[3] == 0
    AL.same_as_checker(known, AL.run(*AC.KNOWN), "known answer", ctx.last_merge_values())
    m = 65
    C, ss, mn, mx = SC.mixed_problem(m, 8, 300 + m)
    frozen = int(np.flatnonzero(ss < 0)[0])
    base = SC.run(C, ss, mn, mx, 2)["log"]
    bite = np.array([(a, b) for a, b in base[:8] if a < m and b < m], np.int32).reshape(-1, 2)
    assert len(bite) >= 2
    cls = np.zeros(m, np.int32)
    cls[[s for s in (0, 31, 32, 33, 63, 64)]] = 3
    cls[[5, 6, 40]] = 9
    jobs = {
        "a pair naming a frozen seed": (C, ss, mn, mx, 2, None, np.array([[frozen, 0], [1, frozen]], np.int32)),
        "duplicates, either order": (C, ss, mn, mx, 2, None, np.concatenate([bite, bite[:, ::-1], bite])),
        "the same pairs once": (C, ss, mn, mx, 2, None, bite),
        "class and pairs": (C, ss, mn, mx, 2, cls, bite),
        "two classes": (C, ss, mn, mx, 2, cls, None),
    }
    res = {}
    for name, job in jobs.items():
        ref = AL.run(*job)
        res[name] = AL.large(ctx, job)
        AL.same_as_checker(res[name], ref, name, ctx.last_merge_values())
        AL.same_tuple(res[name], AL.large(ctx, job, dev=True), name)
    AL.same_tuple(res["duplicates, either order"], res["the same pairs once"], "duplicates")
    AL.same_tuple(res["a pair naming a frozen seed"], ctx.cluster_seeded(C, ss, mn, mx, 2), "a frozen seed's pairs change nothing")
    assert not np.array_equal(res["the same pairs once"][4], base)   # (the first of these pairs is the unconstrained run's first merge of two seeds)
    # a relation that ends the loop early: the anchors never merge with each other, k_target 1 asks for m - 1 merges
    for mm in (64, 300):
        job = AC.anchored(mm, 8, k_target=1)
        r = AL.large(ctx, job)
        AL.same_as_checker(r, AL.run(*job), ("early end", mm), ctx.last_merge_values())
        assert r[3] == 0 and 0 < len(r[4]) < mm - 1 and ctx.last_ward_stats()["merges"] == len(r[4])
    # m <= 1: no merge, the seed is its own cluster
    one = (C[:1], np.array([4], np.int32), 3, 9, 1, np.array([1], np.int32), None)
    r = AL.large(ctx, one)
    AL.same_as_checker(r, AL.run(*one), "one seed")
    assert r[2] == 1 and len(r[4]) == 0 and SC.same_bits(r[5], C[:1]) and apart_mode(ctx)
    nc = CT.c_int32(777)
    assert ctx.L.icl_cluster_apart(ctx.h, None, 0, 8, None, 3, 9, 1, None, 0, None, None, None, CT.byref(nc), None) == 0 and nc.value == 0


def test_errors_and_engine_state(ctx):
    from imageclust_amd import _lib

    m, d = 65, 8
    C, ss, mn, mx, kt, cls, pairs = AC.constrained(m, d)
    L, h = ctx.L, ctx.h
    dC = ctx.malloc(C.nbytes)
    ctx.h2d(dC, C)
    arr = lambda a: None if a is None else a.ctypes.data

    def call(fn, cptr, seed=ss, cls=cls, npairs=len(pairs), pairs=pairs, with_out=True):
        cid, rank = np.full(m, 777, np.int32), np.full(m, 777, np.int32)
        co = np.full((m, d), 777.0, np.float32)
        nc = CT.c_int32(777)
        rc = fn(h, cptr, m, d, arr(seed), mn, mx, kt, arr(cls), npairs, arr(pairs), arr(cid), arr(rank), CT.byref(nc), arr(co) if with_out else None)
        return rc, bool((cid == 777).all() and (rank == 777).all() and nc.value == 777 and (co == 777.0).all())

    def changed(a, at, v):
        a = a.copy()
        a.reshape(-1)[at] = v
        return a

    try:
        assert len(pairs) >= 2
        bad = dict(negative_count=dict(npairs=-1), null_pairs=dict(pairs=None), negative_class=dict(cls=changed(cls, 40, -1)),
                   index_m=dict(pairs=changed(pairs, 0, m)), negative_index=dict(pairs=changed(pairs, 3, -1)),
                   same_seed=dict(pairs=changed(pairs, 1, pairs[0, 0])), size_zero=dict(seed=changed(ss, 7, 0)), null_sizes=dict(seed=None))
        for name, kw in bad.items():
            assert call(L.icl_cluster_apart, arr(C), **kw) == (_lib.ICL_ERR_ARG, True), name
            assert call(L.icl_cluster_apart_dev, dC, with_out=False, **kw) == (_lib.ICL_ERR_ARG, True), (name, "dev")
        assert call(L.icl_cluster_apart, None) == (_lib.ICL_ERR_ARG, True)
        assert call(L.icl_cluster_apart, arr(C)) == (0, False)                       # the well-formed call writes
        assert call(L.icl_cluster_apart, arr(C), cls=None) == (0, False) and call(L.icl_cluster_apart, arr(C), npairs=0, pairs=None) == (0, False)
    finally:
        ctx.free(dC)
    with pytest.raises(_lib.ICLError) as ei:
        ctx.cluster_apart(C, ss, mn, mx, kt, cls, np.array([[0, m]], np.int32))
    assert ei.value.code == _lib.ICL_ERR_ARG
    # refused problems: rows of -1, no log, a C_out of zeros -- as the seeded call's
    big = ss.copy()
    big[int(np.flatnonzero(ss > 0)[0])] = mx + 1
    for job, code in (((C, big, mn, mx, kt, cls, pairs), _lib.ICL_ERR_UNSUPPORTED), ((C[:2], np.ones(2, np.int32), 3, 6, 0, np.array([1, 1], np.int32), None), _lib.ICL_ERR_CONSTRAINT)):
        for dev in (False, True):
            r = AL.large(ctx, job, dev=dev)
            assert r[3] == code and (r[0] == -1).all() and (r[1] == -1).all() and r[2] == 0 and len(r[4]) == 0 and not r[5].any(), (code, dev)
            assert len(ctx.last_merges()) == 0 and ctx.last_ward_mode()[0] == _lib.ROWS_SINGLE_APART
    # the workspace a constrained call leaves: the hook that reads it as singletons refuses it, and takes icl_cluster's again
    E = WC.mog(m, d, 3)
    AL.large(ctx, (C, ss, mn, mx, kt, cls, pairs))
    assert apart_mode(ctx)
    with pytest.raises(_lib.ICLError) as ei:
        ctx.ward_dump_pairs(np.arange(4, dtype=np.int32), d)
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
    ctx.cluster(E, 3, 6)
    assert ctx.last_ward_mode()[0] != _lib.ROWS_SINGLE_APART
    ctx.ward_dump_pairs(np.arange(4, dtype=np.int32), d)


@pytest.mark.parametrize("order", ("apart,seeded,apart", "seeded,apart,seeded"))
def test_constrained_and_unconstrained_steps_do_not_share_a_graph(tmp_path, refs, order):
    """ICL_WARD_BATCH=0 (read once per process: a child): icl_cluster_seeded runs the one-merge-per-step loop too, on the same workspace and
    shape as the constrained call, and both ask for at least 128 merges -- each must replay a graph captured for its own steps."""
    here = os.path.dirname(os.path.abspath(__file__))
    job, _ = refs("constrained", 300, 8)
    job = job[:4] + (300 // 8,) + job[5:]
    want = {"apart": AL.run(*job), "seeded": SC.run(*job[:5])}
    assert not np.array_equal(want["apart"]["log"], want["seeded"]["log"]) and len(want["seeded"]["log"]) >= AL.GRAPH_MERGES // 2
    np.savez(tmp_path / "job.npz", **dict(zip(("C", "ss", "mn", "mx", "kt", "cls", "pairs"), (np.asarray(v) for v in job))))
    p = subprocess.run([sys.executable, os.path.join(here, "apart_large_child.py"), str(tmp_path / "job.npz"), str(tmp_path / "out.npz"), order],
                       env=dict(os.environ, ICL_WARD_BATCH="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    for i, kind in enumerate(order.split(",")):
        r = tuple(out["%s%d" % (k, i)] for k in ("cid", "rank", "nc", "st", "log", "co"))
        assert tuple(out["mode%d" % i]) == ((AL.ROWS_SINGLE_APART, 0) if kind == "apart" else (0, 0)), (i, kind)
        SC.same_as_checker((r[0], r[1], int(r[2]), int(r[3]), r[4], r[5]), want[kind], (i, kind))
        if kind == "apart":
            assert np.array_equal(out["vals%d" % i].view(np.uint32), want[kind]["values"].view(np.uint32)), i


def test_clustering_state_above_the_cap(ctx):
    """Clustering.keep_apart -> recluster and absorb_leftovers at more than 2 100 held clusters: through the context (icl_cluster_apart) and
    through the stand-in engine over the checker, the same state.  Most of the singletons are frozen so that the checker stays quick."""
    from imageclust_amd import clustering

    n, groups, free = 2420, 60, 170   # 2 300 held clusters: 60 of three, 170 free singletons, the rest frozen
    E = WC.mog(n, 8, 41, k=40, sigma=0.3)
    ids = ["img_%d" % i for i in range(n)]
    calls = []
    states = [clustering.Clustering(3, 6, ctx=ctx), clustering.Clustering(3, 6, engine=AL.engine_on(calls))]
    for st in states:
        st.add(E, ids)
        for g in range(groups):   # kept clusters of three, made on the host
            st.keep_together(ids[3 * g:3 * g + 3])
        st.freeze(ids[3 * groups + free:])
        assert len(st.clusters) == n - 2 * groups > 2100
        st.keep_apart([ids[0], ids[3 * groups], ids[3 * groups + 1]])
        st.keep_apart([ids[3], ids[3 * groups + 2]])
        assert st.recluster(len(st.clusters) - 100)
        if st.ctx is not None:
            assert apart_mode(ctx) and len(ctx.last_merges()) > 0
    a, b = states
    assert len(calls) == 1 and len(calls[0][1]) == 4
    assert a.as_map() == b.as_map() and np.array_equal(a.last_merges, b.last_merges) and len(a.last_merges) > 50
    assert len(a.clusters) > 2100
    left = [st.absorb_leftovers() for st in states]
    assert apart_mode(ctx)
    assert len(calls) == 2 and calls[1][0].sum() >= groups and left[0] == left[1]
    assert a.as_map() == b.as_map() and np.array_equal(a.last_merges, b.last_merges) and len(a.last_merges) > 0
    assert all(SC.same_bits(x.Centroid, y.Centroid) for x, y in zip(a.clusters, b.clusters))
    where = {k: i for i, c in enumerate(a.clusters) for k in c.Members}
    assert len({where[ids[0]], where[ids[3 * groups]], where[ids[3 * groups + 1]]}) == 3 and where[ids[3]] != where[ids[3 * groups + 2]]
