"""FAST mode from seeds (icl_cluster_seeded_fast[_dev], icl_distance_mfma_seeded_dev; DESIGN.md "Seeded clustering in FAST mode") against its
definition, tests/lw_seeded_numpy.py, bit for bit: the sized matrix alone against the formula applied to icl_distance_mfma_dev's output, the call's
log, heights, ids, ranks and C_out against the restatement on that matrix -- the batched loop here, the one-merge-per-step loop in a child
process --, all-ones seeds against icl_cluster(update=LW), three kinds of call sharing one context, statuses, and the Python layer.  Against the
exact seeded call only the Rand index on separated seeds is asserted: the two are different algorithms.
Not tested here: a replica context of a group (ICL_ERR_UNSUPPORTED) and ICL_ERR_NOMEM."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lw_seeded_numpy as LS
from tests import seeded_cases as SC
from tests import seeded_large_cases as LC
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu
F = np.float32
SENT = F(-7.25)  # what every output cell holds before a call
SINGLE = os.environ.get("ICL_WARD_BATCH", "")[:1] == "0"  # the one-merge-per-step loop in THIS process


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the sized matrix alone ------------------------------------------------------------------------------------------------------------
def matrix_rows(n, d, seed):
    """Random rows; from n = 4 on: an exact duplicate on small integers (D~ exactly 0, stored +0), a duplicate on coordinates bf16 does not hold
    (rounding noise around 0), and one NaN row."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n, d)).astype(F)
    if n >= 4:
        E[1] = rng.integers(-3, 4, d).astype(F)
        E[n - 1] = E[1]
        E[n // 2] = E[0]
        E[2, d // 2] = np.nan
    ss = rng.integers(1, 51, n).astype(np.int32)
    ss[rng.random(n) < 0.3] *= -1
    if n >= 2:
        ss[0], ss[1] = 50, -1
    return E, ss


def dense_matrix(ctx, E, ld, ss=None):
    """icl_distance_mfma_dev (ss None) or icl_distance_mfma_seeded_dev into n rows of pitch ld prefilled with SENT -> the n x ld array"""
    n, d = E.shape
    out = np.full((n, ld), SENT, F)
    dE, dD = ctx.malloc(max(E.nbytes, 16)), ctx.malloc(max(out.nbytes, 16))
    try:
        ctx.h2d(dE, E)
        if out.size:
            ctx.h2d(dD, out)
        if ss is None:
            rc = ctx.L.icl_distance_mfma_dev(ctx.h, C.c_void_p(dE), n, d, C.c_void_p(dD), ld)
            assert rc == 0
        else:
            ctx.distance_mfma_seeded_dev(dE, n, d, ss, dD, ld)
        if out.size:
            ctx.d2h(out, dD)
    finally:
        ctx.free(dE)
        ctx.free(dD)
    return out


MATRIX_SHAPES = [(n, d) for n in (1, 2, 127, 128, 129, 257, 300) for d in (1, 3, 64, 100, 192)] + [(129, 2048)]


@pytest.mark.parametrize("n,d", MATRIX_SHAPES, ids=["%dx%d" % s for s in MATRIX_SHAPES])
def test_sized_matrix_equals_formula_on_the_unsized_matrix(ctx, n, d):
    E, ss = matrix_rows(n, d, 1000 * n + d)
    D = np.tril(dense_matrix(ctx, E, n), -1)
    want = LS.sized_matrix(D, ss)
    low, diag = np.tri(n, n, -1, dtype=bool), np.eye(n, dtype=bool)
    if n >= 4:  # the inputs hold what they are for
        assert np.isnan(D[2, :2]).all() and np.isnan(D[3:, 2]).all()
        assert D[n - 1, 1] == 0 and not np.signbit(D[n - 1, 1])
        assert (ss < 0).any() and (ss > 1).any() and (np.abs(ss) != np.abs(ss[0])).any()
    for ld in range(n, n + 6):
        got = dense_matrix(ctx, E, ld, ss)
        sq = got[:, :n]
        ok = (bits(sq) == bits(want)) | (np.isnan(sq) & np.isnan(want))
        assert ok[low].all(), "n %d d %d ld %d: %d entries differ from the formula" % (n, d, ld, int((~ok[low]).sum()))
        assert not np.signbit(sq[low][sq[low] == 0]).any(), "a zero is stored as -0"
        assert (bits(sq[diag]) == 0).all(), "diagonal"
        assert (bits(sq[~low & ~diag]) == bits(SENT)).all() and (bits(got[:, n:]) == bits(SENT)).all(), "n %d d %d ld %d: a cell outside the triangle was written" % (n, d, ld)


def test_sized_matrix_with_all_ones_is_the_unsized_matrix(ctx):
    E, _ = matrix_rows(257, 100, 5)
    a, b = dense_matrix(ctx, E, 260), dense_matrix(ctx, E, 260, np.ones(257, np.int32))
    assert ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


def test_sized_matrix_argument_errors(ctx):
    from imageclust_amd import _lib

    dC, dD = ctx.malloc(64), ctx.malloc(256)
    try:
        ctx.h2d(dC, np.ones((4, 3), F))
        ctx.h2d(dD, np.full(64, SENT, F))
        for what, ss, ld, c, o in [("a size of 0", [1, 0, 1, 1], 4, dC, dD), ("ld < m", [1, 1, 1, 1], 3, dC, dD), ("2^30 items", [1, 1 << 30, 1, 1], 4, dC, dD),
                                   ("C", [1, 1, 1, 1], 4, None, dD), ("D", [1, 1, 1, 1], 4, dC, None)]:
            with pytest.raises(_lib.ICLError) as ei:
                ctx.distance_mfma_seeded_dev(c, 4, 3, ss, o, ld)
            assert ei.value.code == _lib.ICL_ERR_ARG, what
        out = np.zeros(64, F)
        ctx.d2h(out, dD)
        assert (bits(out) == bits(SENT)).all()
    finally:
        ctx.free(dC)
        ctx.free(dD)


# ---- the call against the restatement --------------------------------------------------------------------------------------------------
SEEN = []  # what the problems check_job ran contained


def fast_dev(ctx, job):
    """icl_cluster_seeded_fast_dev with every output prefilled -> (cid, rank, nc, status, log, C_out)"""
    from imageclust_amd import _lib

    Cs, ss, mn, mx, kt = np.ascontiguousarray(job[0], F), job[1], job[2], job[3], job[4]
    m, d = Cs.shape
    co = np.full((m, d), SENT, F)
    dC, dO = ctx.malloc(max(Cs.nbytes, 16)), ctx.malloc(max(co.nbytes, 16))
    try:
        if Cs.size:
            ctx.h2d(dC, Cs)
            ctx.h2d(dO, co)
        cid, rank, nc, st = ctx.cluster_seeded_dev(dC, m, d, ss, mn, mx, kt, dO, update=_lib.UPDATE_LW)
        if co.size:
            ctx.d2h(co, dO)
    finally:
        ctx.free(dC)
        ctx.free(dO)
    return cid, rank, nc, st, (ctx.last_merges() if st == _lib.ICL_OK else np.zeros((0, 2), np.int32)), co


def expected(ctx, job, D=None):
    """The restatement's answer for a job on the engine's own stand-alone matrix, with C_out"""
    Cs, ss, mn, mx, kt = job
    if D is None:
        D = ctx.distance_mfma(Cs) if len(ss) else np.zeros((0, 0), F)
    want = LS.cluster_lw_seeded(D, ss, mn, mx, kt)
    want["C_out"] = LS.centroids_from_log(Cs, ss, want["log"]) if want["status"] == LS.OK else np.zeros_like(np.asarray(Cs, F))
    want["D"] = D
    return want


def first_difference(log, val, want):
    wl, wv = want["log"], want["values"]
    for t in range(min(len(log), len(wl))):
        if tuple(log[t]) != tuple(wl[t]) or bits(val[t:t + 1])[0] != bits(wv[t:t + 1])[0]:
            return "merge %d: engine (%d, %d) at %r, restatement (%d, %d) at %r" % (t, log[t][0], log[t][1], float(val[t]), wl[t][0], wl[t][1], float(wv[t]))
    return "the first %d merges agree; engine made %d, restatement %d" % (min(len(log), len(wl)), len(log), len(wl))


def same_as_restatement(got, val, want, what):
    cid, rank, nc, st, log, co = got
    assert st == want["status"], (what, st, want["status"])
    same_log = len(log) == len(want["log"]) and np.array_equal(log, want["log"]) and np.array_equal(bits(val), bits(want["values"]))
    assert same_log, "%s: %s" % (what, first_difference(log, val, want))
    assert np.array_equal(cid, want["cluster_id"]) and np.array_equal(rank, want["seed_rank"]) and nc == want["n_clusters"], what
    assert SC.same_bits(co, want["C_out"]), what + ": C_out"


def check_job(ctx, job, what, note=True):
    from imageclust_amd import _lib

    want = expected(ctx, job)
    for form in ("host", "dev"):
        got = ctx.cluster_seeded(*job, update=_lib.UPDATE_LW) if form == "host" else fast_dev(ctx, job)
        val = ctx.last_merge_values() if got[3] == _lib.ICL_OK else np.zeros(0, F)
        same_as_restatement(got, val, want, "%s, %s form" % (what, form))
        if got[3] == _lib.ICL_OK:
            assert ctx.last_ward_mode()[0] == (_lib.ROWS_SINGLE if SINGLE else _lib.ROWS_LW_FAST), what
            assert ctx.last_ward_stats()["merges"] == len(want["log"]), what
    if note and want["status"] == LS.OK:
        Cs, ss, mn, mx, kt = job
        m = len(ss)
        st, N, k, kmax, eff = LS.admit(ss, mn, mx, kt)
        low = np.tri(m, m, -1, dtype=bool)
        V0 = LS.sized_matrix(want["D"], ss)[low] if m > 1 else np.zeros(0, F)
        V0 = V0[np.isfinite(V0) & (V0 > 0)]
        SEEN.append(dict(mixed=len(set(np.abs(ss).tolist())) > 1, frozen=bool((ss < 0).any()), k_target=kt > 0, asked=max(0, m - k),
                         early=len(want["log"]) < max(0, m - k), ties=bool(len(V0) and np.unique(V0, return_counts=True)[1].max() > 5),
                         dup=bool(m > 1 and (np.asarray(Cs)[:, None, :] == np.asarray(Cs)[None, :, :]).all(2)[low].any()), nan=bool(np.isnan(Cs).any()),
                         merges=len(want["log"])))
    return want


SHAPES = [(m, d) for m in (0, 1, 2, 3, 64, 65, 129, 130, 257, 300) for d in (3, 8, 100)]


def nan_job(m, d):
    """LC.shape_jobs' first problem with one NaN row"""
    Cs, ss, mn, mx, kt = LC.shape_jobs(m, d)[0]
    Cs = Cs.copy()
    Cs[m // 3, d // 2] = np.nan
    return Cs, ss, mn, mx, kt


@pytest.mark.parametrize("m,d", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_call_equals_restatement(ctx, m, d):
    """Mixed sizes, frozen seeds, a seed of max_size, duplicated centroids with the default k; exact ties with a k_target that asks for more merges than
    the sizes allow; from 64 seeds on a NaN row too.  Host and _dev forms, every output prefilled in the latter."""
    jobs = LC.shape_jobs(m, d) + ([nan_job(m, d)] if m >= 64 else [])
    for i, job in enumerate(jobs):
        check_job(ctx, job, "m %d d %d job %d" % (m, d, i))


def test_call_tests_are_not_vacuous(ctx):
    """The problems above held each thing the restatement has a rule for, and the captured graph replayed (2 x 64 merges asked for, and more than one
    replay's worth made)."""
    if not SEEN:  # run on its own
        for m, d in ((300, 8), (130, 3)):
            for i, job in enumerate(LC.shape_jobs(m, d) + [nan_job(m, d)]):
                check_job(ctx, job, "m %d d %d job %d" % (m, d, i))
    for key in ("mixed", "frozen", "k_target", "early", "ties", "dup", "nan"):
        assert any(s[key] for s in SEEN), key
    assert any(s["asked"] >= 128 and s["merges"] > 64 for s in SEEN)
    assert any(not s["early"] and s["merges"] > 0 for s in SEEN)


@pytest.mark.parametrize("n,d,mn,mx", [(300, 8, 3, 9), (1000, 16, 5, 50)])
def test_all_ones_seeds_equal_unseeded_fast(ctx, n, d, mn, mx):
    from imageclust_amd import _lib

    E = WC.mog(n, d, n + d)
    cid, rank, nc = ctx.cluster(E, mn, mx, _lib.UPDATE_LW)
    log, val = ctx.last_merges(), ctx.last_merge_values()
    assert len(log) >= 128
    got = ctx.cluster_seeded(E, np.ones(n, np.int32), mn, mx, 0, update=_lib.UPDATE_LW)
    assert got[3] == _lib.ICL_OK and np.array_equal(got[4], log) and np.array_equal(bits(ctx.last_merge_values()), bits(val))
    assert np.array_equal(got[0], cid) and np.array_equal(got[1], rank) and got[2] == nc


def test_c_out_rows(ctx):
    """C_out against the numpy replay of the call's OWN log; zero rows where no rank-0 seed sits, the input row for a never-merged seed."""
    job = LC.shape_jobs(130, 100)[0]
    cid, rank, nc, st, log, co = fast_dev(ctx, job)
    Cs, ss = np.asarray(job[0], F), job[1]
    assert st == 0 and len(log) > 10
    assert SC.same_bits(co, LS.centroids_from_log(Cs, ss, log))
    merged = set(log.ravel().tolist())
    never = [i for i in range(len(ss)) if i not in merged]
    _, _, _, finals = LS.final_list(ss, job[2], log)
    heads = {f[1][0] for f in finals}
    assert never and len(heads) < len(ss)
    for i in range(len(ss)):
        if i in never:
            assert np.array_equal(bits(co[i]), bits(Cs[i])), i
        elif i not in heads:
            assert (bits(co[i]) == 0).all(), i


def test_one_context_three_kinds_of_call(ctx):
    """Seeded FAST, unseeded FAST and exact seeded on one (m, d), each replaying a captured graph (>= 128 merges), each against its own reference, then
    seeded FAST again: a graph replayed under another call's key would cluster wrongly without any error."""
    from imageclust_amd import _lib
    from tests import lw_numpy as LW

    Cs, ss, mn, mx, _ = LC.shape_jobs(300, 8)[0]
    kt = 100  # 200 merges asked for
    job = (Cs, ss, mn, mx, kt)
    want = check_job(ctx, job, "seeded FAST first", note=False)
    asked = len(ss) - LS.admit(ss, mn, mx, kt)[2]
    assert asked >= 128 and len(want["log"]) > 64  # (the graph is replayed from 2 x 64 merges ASKED for; this run ends early for want of pairs)
    lw = LW.cluster_lw(want["D"], mn, mx)
    cid, rank, nc = ctx.cluster(Cs, mn, mx, _lib.UPDATE_LW)
    assert len(lw[3]) >= 128 and np.array_equal(ctx.last_merges(), lw[3]) and np.array_equal(bits(ctx.last_merge_values()), bits(lw[4]))
    assert np.array_equal(cid, lw[0]) and np.array_equal(rank, lw[1]) and nc == lw[2]
    check_job(ctx, job, "seeded FAST after unseeded FAST", note=False)
    ref = SC.run(*job)
    assert len(ref["log"]) > 64
    SC.same_as_checker(ctx.cluster_seeded(*job), ref, "exact seeded after seeded FAST")
    check_job(ctx, job, "seeded FAST after exact seeded", note=False)
    cid, rank, nc = ctx.cluster(Cs, mn, mx, _lib.UPDATE_LW)
    assert np.array_equal(ctx.last_merges(), lw[3]) and np.array_equal(cid, lw[0])
    SC.same_as_checker(ctx.cluster_seeded(*job), ref, "exact seeded after unseeded FAST")


def test_one_merge_per_step_loop_equals_restatement(ctx, tmp_path):
    """ICL_WARD_BATCH=0 (read once per process: a child): the seeded FAST call on ward_update_lw_kernel's loop, held to the same restatement."""
    here = os.path.dirname(os.path.abspath(__file__))
    jobs = [j for m, d in ((65, 3), (130, 8), (300, 8)) for j in LC.shape_jobs(m, d)] + [nan_job(130, 8)]
    np.savez(tmp_path / "jobs.npz", **{"%s%d" % (k, i): np.asarray(v) for i, j in enumerate(jobs) for k, v in zip("CSNXK", j)})
    p = subprocess.run([sys.executable, os.path.join(here, "seeded_fast_child.py"), str(tmp_path / "jobs.npz"), str(tmp_path / "out.npz"), str(len(jobs))],
                       env=dict(os.environ, ICL_WARD_BATCH="0"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.load(tmp_path / "out.npz")
    asked = 0
    for i, job in enumerate(jobs):
        want = expected(ctx, job)
        r = tuple(out["%s%d" % (k, i)] for k in ("cid", "rank", "nc", "st", "log", "co"))
        assert tuple(out["mode%d" % i]) == (0, 0), i  # ICL_ROWS_SINGLE, no bounds
        same_as_restatement((r[0], r[1], int(r[2]), int(r[3]), r[4], r[5]), out["val%d" % i], want, "job %d, one merge per step" % i)
        asked = max(asked, len(job[1]) - LS.admit(*job[1:])[2] if len(want["log"]) > 64 else 0)
    assert asked >= 128  # the captured graph of single steps replayed, and more than one replay did work


def test_against_exact_seeded_on_separated_seeds(ctx):
    """Reported: how the FAST partition of separated mixture-of-Gaussians seeds (m = 300, d = 64, mixed sizes, every blob fits max_size, k_target = the
    blobs) compares with the exact seeded call's.  Asserted: the criterion of the unseeded pair, Rand index >= 0.999."""
    from imageclust_amd import _lib
    from tests.test_fast_mode_gpu import mog, rand_index

    Cs, lab = mog(300, 64, 64, k=15)
    ss = np.random.default_rng(9).integers(1, 5, 300).astype(np.int32)
    k = len(set(lab.tolist()))
    e = ctx.cluster_seeded(Cs, ss, 1, 400, k)
    f = ctx.cluster_seeded(Cs, ss, 1, 400, k, update=_lib.UPDATE_LW)
    assert e[3] == 0 and f[3] == 0
    ri = rand_index(e[0], f[0])
    print("m=300 d=64: exact %d clusters, fast %d clusters, identical ids %.4f, Rand index %.4f, against the blobs %.4f / %.4f"
          % (e[2], f[2], float((e[0] == f[0]).mean()), ri, rand_index(e[0], lab), rand_index(f[0], lab)))
    assert ri >= 0.999


# ---- statuses --------------------------------------------------------------------------------------------------------------------------
def reports(ctx):
    return (ctx.last_merges().tobytes(), ctx.last_merge_values().tobytes(), tuple(sorted(ctx.last_ward_stats().items())), ctx.last_ward_mode())


def test_argument_errors_write_nothing(ctx):
    from imageclust_amd import _lib

    check_job(ctx, LC.shape_jobs(65, 3)[0], "a call whose reports must survive", note=False)
    before = reports(ctx)
    Cs = np.ones((4, 3), F)
    good = np.array([1, 2, -1, 1], np.int32)
    zero = np.array([1, 0, 1, 1], np.int32)
    dC, dO = ctx.malloc(64), ctx.malloc(64)
    try:
        for fn, cp, op in ((ctx.L.icl_cluster_seeded_fast, Cs.ctypes.data, None), (ctx.L.icl_cluster_seeded_fast_dev, dC, dO)):
            for what, kw in [("m < 0", dict(m=-1)), ("d < 0", dict(d=-1)), ("n_clusters", dict(nc=False)), ("C", dict(c=None)), ("seed_size", dict(ss=None)),
                             ("cluster_id", dict(cid=False)), ("seed_rank", dict(rank=False)), ("a size of 0", dict(ss=zero))]:
                cid, rank, nc = np.full(4, -5, np.int32), np.full(4, -5, np.int32), C.c_int32(-5)
                co = np.full((4, 3), SENT, F)
                if op is not None:
                    ctx.h2d(dO, co)
                ssa = kw.get("ss", good)
                rc = fn(ctx.h, kw["c"] if "c" in kw else cp, kw.get("m", 4), kw.get("d", 3), None if ssa is None else ssa.ctypes.data, 1, 4, 0,
                        cid.ctypes.data if kw.get("cid", True) else None, rank.ctypes.data if kw.get("rank", True) else None,
                        C.byref(nc) if kw.get("nc", True) else None, co.ctypes.data if op is None else op)
                assert rc == _lib.ICL_ERR_ARG, what
                if op is not None:
                    ctx.d2h(co, dO)
                assert (cid == -5).all() and (rank == -5).all() and nc.value == -5 and (bits(co) == bits(SENT)).all(), what
                assert reports(ctx) == before, what
    finally:
        ctx.free(dC)
        ctx.free(dO)
    with pytest.raises(_lib.ICLError) as ei:  # FAST mode has no constrained call
        ctx.cluster_seeded(Cs, good, 1, 4, 0, update=_lib.UPDATE_LW, _apart=ctx._apart_args(4, None, [(0, 1)]))
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED


@pytest.mark.parametrize("ss,mn,mx,status", [([3, 3, 4], 4, 4, LS.ERR_CONSTRAINT), ([1, 7, -9, 2], 2, 6, LS.ERR_UNSUPPORTED)])
def test_refused_problems(ctx, ss, mn, mx, status):
    """ICL_ERR_CONSTRAINT (the item total does not split) and ICL_ERR_UNSUPPORTED (an unfrozen seed above max_size): rows of -1, a C_out of zeros."""
    Cs = WC.mog(len(ss), 5, 3)
    job = (Cs, np.array(ss, np.int32), mn, mx, 0)
    assert expected(ctx, job)["status"] == status
    for got in (fast_dev(ctx, job), ctx.cluster_seeded(*job, update=1)):
        assert got[3] == status and got[2] == 0 and (got[0] == -1).all() and (got[1] == -1).all() and (bits(got[5]) == 0).all()
    assert len(ctx.last_merges()) == 0 and ctx.last_ward_stats()["merges"] == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_clustering_state_in_fast_mode(ctx):
    """Clustering(update=UPDATE_LW): start / add / freeze / recluster through the context (icl_cluster_seeded_fast at any seed count) and through a
    stand-in engine made of the restatement on the context's matrix: the same clusters, members and centroid bits after every step."""
    from imageclust_amd import _lib
    from imageclust_amd import clustering as CL

    def engine(Cs, ss, mn, mx, kt):
        want = expected(ctx, (Cs, ss, mn, mx, kt))
        return want["cluster_id"], want["seed_rank"], want["n_clusters"], want["status"], want["log"], want["C_out"]

    E = WC.mog(90, 8, 12)
    ids = ["img_%d" % i for i in range(90)]

    def same(a, b, what):
        assert a.as_map() == b.as_map(), what
        assert [c.Members for c in a.clusters] == [c.Members for c in b.clusters] and [c.Frozen for c in a.clusters] == [c.Frozen for c in b.clusters], what
        assert all(SC.same_bits(x.Centroid, y.Centroid) for x, y in zip(a.clusters, b.clusters)), what

    a = CL.Clustering.start(E[:70], ids[:70], 2, 6, ctx=ctx, update=_lib.UPDATE_LW)
    b = CL.Clustering.start(E[:70], ids[:70], 2, 6, engine=engine, update=_lib.UPDATE_LW)
    assert a.ok and ctx.last_ward_mode()[0] == (_lib.ROWS_SINGLE if SINGLE else _lib.ROWS_LW_FAST)
    same(a, b, "start")
    for s in (a, b):
        s.add(E[70:], ids[70:])
        s.freeze([ids[0], ids[5]])
        assert s.recluster()
    same(a, b, "add + freeze + recluster")
    assert any(c.Frozen for c in a.clusters) and len(a.last_merges) > 0
    held = [c.Members for c in a.clusters if c.Frozen]
    for s in (a, b):
        assert s.recluster(k_target=max(1, len(s.clusters) // 2))
    same(a, b, "recluster(k_target)")
    assert all(m in [c.Members for c in a.clusters] for m in held)  # frozen clusters came through as they were
    a.keep_apart([a.clusters[0].Members[0], a.clusters[1].Members[0]])  # an LW state with a keep-apart constraint raises
    with pytest.raises(_lib.ICLError) as ei:
        a.recluster()
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
