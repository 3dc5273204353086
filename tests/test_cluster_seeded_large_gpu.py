"""icl_cluster_seeded[_dev] (imageclust_amd/csrc/ward.hip, DESIGN.md "Seeded clustering": the large-N route): one seeded problem on the
large-N engine's exact pipeline, any number of seeds.  Bar: cluster ids, seed ranks, cluster count, status, merge log and C_out (as
uint32) equal the checker's (tests/seeded_cases.py), icl_cluster_many_seeded's and, from all-ones seeds, icl_cluster's, BIT-EXACT."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import seeded_cases as SC
from tests import seeded_large_cases as LC
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def ones(E):
    return np.ones(len(E), np.int32)


def unseeded(ctx, E, mn, mx):
    """icl_cluster and its reports: (cid, rank, nc, log, merge values, (row mode, initial bounds))"""
    cid, rank, nc = ctx.cluster(E, mn, mx)
    return cid, rank, nc, ctx.last_merges(), ctx.last_merge_values(), tuple(ctx.last_ward_mode())


@pytest.mark.parametrize("d", LC.SHAPES_D)
def test_equals_the_checker_and_the_many_call(ctx, d):
    """Mixed sizes, frozen seeds, duplicates, a seed of max_size, exact ties: the checker's result, and icl_cluster_many_seeded's (its
    small route up to 256 seeds, its mid route at 300), bit for bit."""
    from imageclust_amd import _lib

    merged = replayed = 0
    for m in LC.SHAPES_M:
        for q, job in enumerate(LC.shape_jobs(m, d)):
            ref = SC.run(*job)
            r = LC.large(ctx, job)
            SC.same_as_checker(r, ref, (m, d, q))
            # exact rows, no bounds in the initial matrix, whatever the size
            assert ctx.last_ward_mode() == (_lib.ROWS_EXACT_BATCH, False) and ctx.last_ward_bound_violations() == 0
            assert len(ctx.last_merge_values()) == len(ref["log"])
            LC.same_tuple(r, LC.many(ctx, job), (m, d, q))
            merged += len(ref["log"])
            replayed += job[4] > 0 and m - job[4] >= LC.GRAPH_MERGES and len(ref["log"]) >= LC.GRAPH_MERGES
    assert merged >= 2 * LC.GRAPH_MERGES and replayed >= 1  # (m = 300 with a k_target: more than 128 merges asked for and made -- the captured steps replay)


@pytest.fixture(scope="module")
def restart(ctx):
    """icl_cluster on 4 200 rows (auto mode: int8 bounds in the initial matrix, bound rows in the loop): the run the seeded calls resume"""
    E, mn, mx = LC.restart_problem()
    return E, mn, mx, unseeded(ctx, E, mn, mx)


def test_all_ones_equals_icl_cluster(ctx, restart):
    """n = 300: both calls run the exact batched loop; n = 4 200: icl_cluster takes the bounds (initial matrix and new rows), the seeded
    call the exact pipeline -- two different pipelines, one result."""
    from imageclust_amd import _lib

    E300 = WC.mog(300, 8, 3)
    for E, mn, mx, ref in ((E300, 3, 6, unseeded(ctx, E300, 3, 6)), restart):
        n = len(E)
        cid, rank, nc, st, log, co = ctx.cluster_seeded(E, ones(E), mn, mx)
        assert st == 0 and nc == ref[2] and np.array_equal(cid, ref[0]) and np.array_equal(rank, ref[1]), n
        assert np.array_equal(log, ref[3]) and len(log) == n - n // 4, n  # (k = n / 4 at min 3 / max 6)
        assert np.array_equal(ctx.last_merge_values().view(np.uint32), ref[4].view(np.uint32)), n
        assert ctx.last_ward_mode() == (_lib.ROWS_EXACT_BATCH, False)
        assert ref[5] == ((_lib.ROWS_LW_BOUND, True) if n >= 4096 else (_lib.ROWS_EXACT_BATCH, False)), ref[5]
        assert SC.same_bits(co, SC.centroids_from_log(E, ones(E), log)), n


@pytest.mark.parametrize("t", (1, 1575, 3149))
def test_restart_identity_above_the_old_cap(ctx, restart, t):
    """The run of 3 150 merges cut after t of them and resumed from that state (4 199, 2 625 and 1 051 seeds): the rest of the log, the same
    merge values and the centroids of the uncut run; the cut that fits icl_cluster_many_seeded equals it too."""
    E, mn, mx, (_, _, _, log, vals, _) = restart
    assert len(log) == 3150
    C2, ss2, seeds2, ids = SC.state_after(E, ones(E), log, t)
    assert len(ids) == len(E) - t
    job = (C2, ss2, mn, mx, len(ids) - (len(log) - t))
    r = LC.large(ctx, job)
    log2 = SC.resumed_log(log, t, ids, len(E))
    assert r[3] == 0 and np.array_equal(r[4], log2), t
    assert np.array_equal(ctx.last_merge_values().view(np.uint32), vals[t:].view(np.uint32)), t
    assert SC.same_bits(r[5], SC.centroids_from_log(C2, ss2, log2)), t
    full = SC.centroids_from_log(E, ones(E), log)  # ... which are the uncut run's: cluster q of the state starts with the uncut run's item seeds2[q][0]
    for q in np.flatnonzero(r[1] == 0):
        assert SC.same_bits(r[5][q], full[seeds2[q][0]]), (t, q)
    if len(ids) <= SC.MAX_SEEDS:
        LC.same_tuple(r, LC.many(ctx, job), t)


def test_edge_cases(ctx):
    from imageclust_amd import _lib

    C, ss, mn, mx = SC.mixed_problem(65, 8, 11)
    N = int(np.abs(ss).sum())
    k0 = _lib.calc_optimal_clusters(N, mn, mx)[0]
    for kt in (k0 + 9, max(1, k0 - 9), 65, 200):  # above and below the default; no merge asked for
        job = (C, ss, mn, mx, kt)
        r = LC.large(ctx, job)
        SC.same_as_checker(r, SC.run(*job), kt)
        assert len(r[4]) <= max(0, 65 - kt)
    assert len(LC.large(ctx, (C, ss, mn, mx, k0 + 9))[4]) == 65 - (k0 + 9)
    # every seed frozen: nothing may merge although 64 merges are asked for
    fr = (C, -np.abs(ss), mn, mx, 1)
    r = LC.large(ctx, fr)
    SC.same_as_checker(r, SC.run(*fr), "all frozen")
    assert r[3] == 0 and len(r[4]) == 0 and SC.same_bits(r[5], C) and ctx.last_ward_stats()["merges"] == 0
    # every pair banned before k is reached: seeds of 2 and 3 items under max_size 4 -- the 2s pair up, then no pair is left
    s5 = np.array([2, 3] * 20 + [4], np.int32)  # (the seed of exactly max_size stays as it is)
    ban = (C[:41], s5, 1, 4, 1)
    r = LC.large(ctx, ban)
    ref = SC.run(*ban)
    SC.same_as_checker(r, ref, "no pair left")
    assert len(r[4]) == 10 and r[2] == 31 and r[0][40] >= 0 and r[1][40] == 0
    # refused problems: rows of -1, no log, a C_out of zeros -- as the many-call's
    big = ss.copy()
    big[0] = mx + 1
    for job, code in (((C, big, mn, mx, 0), _lib.ICL_ERR_UNSUPPORTED), ((C[:2], np.array([1, 1], np.int32), 3, 6, 0), _lib.ICL_ERR_CONSTRAINT)):
        for dev in (False, True):
            r = LC.large(ctx, job, dev=dev)
            assert r[3] == code and (r[0] == -1).all() and (r[1] == -1).all() and r[2] == 0 and len(r[4]) == 0 and not r[5].any(), (code, dev)
            assert len(ctx.last_merges()) == 0
            LC.same_tuple(r, LC.many(ctx, job), code)
    # a size of 0 and a null array: ICL_ERR_ARG, nothing written
    L, h = ctx.L, ctx.h
    import ctypes as CT

    for seed in (np.where(np.arange(65) == 7, 0, ss).astype(np.int32), None):
        cid, rank, co = np.full(65, 777, np.int32), np.full(65, 777, np.int32), np.full((65, 8), 777.0, np.float32)
        nc = CT.c_int32(777)
        rc = L.icl_cluster_seeded(h, C.ctypes.data, 65, 8, seed.ctypes.data if seed is not None else None, mn, mx, 0, cid.ctypes.data,
                                  rank.ctypes.data, CT.byref(nc), co.ctypes.data)
        assert rc == _lib.ICL_ERR_ARG and (cid == 777).all() and (rank == 777).all() and nc.value == 777 and (co == 777.0).all()
    # no seeds: the many-call's answers -- (nil,false) without a k_target, no cluster with one
    assert L.icl_cluster_seeded(h, None, 0, 8, None, mn, mx, 0, None, None, CT.byref(nc), None) == _lib.ICL_ERR_CONSTRAINT and nc.value == 0
    assert L.icl_cluster_seeded(h, None, 0, 8, None, mn, mx, 1, None, None, CT.byref(nc), None) == 0 and nc.value == 0


def test_dev_equals_host_and_the_workspace_is_shared_both_ways(ctx):
    """icl_cluster_seeded_dev gives the host call's results; a seeded call between two identical icl_cluster calls on the same (n, d)
    -- the same workspace and, at 300 rows, the same captured graph -- leaves the second one's results equal to the first's, and the
    seeded call's own results do not depend on what ran before it."""
    from imageclust_amd import _lib

    for m, d in ((17, 3), (65, 8), (129, 1037), (300, 8)):
        for q, job in enumerate(LC.shape_jobs(m, d)):
            LC.same_tuple(LC.large(ctx, job), LC.large(ctx, job, dev=True), (m, d, q))
    E = WC.mog(300, 8, 3)
    job = LC.shape_jobs(300, 8)[1]
    alone = LC.large(ctx, job)
    first = unseeded(ctx, E, 3, 6)
    between = LC.large(ctx, job)
    second = unseeded(ctx, E, 3, 6)
    again = LC.large(ctx, job)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    LC.same_tuple(alone, between, "after icl_cluster")
    LC.same_tuple(alone, again, "after icl_cluster, twice")
    # the test hook that reads a workspace as singletons refuses the one a seeded call leaves
    with pytest.raises(_lib.ICLError) as ei:
        ctx.ward_dump_pairs(np.arange(4, dtype=np.int32), 8)
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
    unseeded(ctx, E, 3, 6)
    ctx.ward_dump_pairs(np.arange(4, dtype=np.int32), 8)  # ... and takes icl_cluster's again


def test_one_merge_per_step_pipeline(tmp_path):
    """ICL_WARD_BATCH=0 (read once per process: a child): the seeded call on the one-merge-per-step loop against the checker."""
    here = os.path.dirname(os.path.abspath(__file__))
    jobs = [j for m, d in ((65, 3), (129, 8), (300, 8)) for j in LC.shape_jobs(m, d)]
    np.savez(tmp_path / "jobs.npz", **{"%s%d" % (k, i): np.asarray(v) for i, j in enumerate(jobs) for k, v in zip("CSNXK", j)})
    p = subprocess.run([sys.executable, os.path.join(here, "seeded_large_child.py"), str(tmp_path / "jobs.npz"), str(tmp_path / "out.npz"), str(len(jobs))],
                       env=dict(os.environ, ICL_WARD_BATCH="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    for i, job in enumerate(jobs):
        r = tuple(out["%s%d" % (k, i)] for k in ("cid", "rank", "nc", "st", "log", "co"))
        assert tuple(out["mode%d" % i]) == (0, 0), i  # ICL_ROWS_SINGLE, no bounds
        SC.same_as_checker((r[0], r[1], int(r[2]), int(r[3]), r[4], r[5]), SC.run(*job), i)


def test_clustering_state_above_the_cap(ctx):
    """Clustering.start on 2 100 images takes the new call (2 100 seeds) and gives PerformClusteringWithConstraints' map; 64 more images and
    recluster() equal cluster_seeded on the seeds the state held before the call."""
    from imageclust_amd import clustering

    n, extra = 2100, 64
    E = WC.mog(n + extra, 8, 77)
    ids = ["img_%d" % i for i in range(n + extra)]
    st = clustering.Clustering.start(E[:n], ids[:n], 3, 6, ctx=ctx)
    assert st.ok and len(st.last_merges) == n - n // 4
    assert (st.as_map(), True) == clustering.PerformClusteringWithConstraints(E[:n], ids[:n], 3, 6, ctx=ctx)
    st.add(E[n:], ids[n:])
    Cs, ss = st.seeds()
    members = [list(c.Members) for c in st.clusters]
    assert len(ss) == len(members) and (ss[-extra:] == 1).all() and int(ss.sum()) == n + extra
    assert st.recluster()
    cid, rank, nc, status, log, co = ctx.cluster_seeded(Cs, ss, 3, 6)
    assert status == 0 and len(log) > 0 and np.array_equal(st.last_merges, log)
    finals = {}
    for i in np.lexsort((rank, cid)):
        if cid[i] >= 0:
            finals.setdefault(int(cid[i]), []).extend(members[i])
    assert st.as_map() == finals
    for c in st.clusters:  # every held cluster's centroid is the row of its first seed
        first = next(i for i, mem in enumerate(members) if mem[0] == c.Members[0])
        assert SC.same_bits(c.Centroid, co[first])
