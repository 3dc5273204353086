"""icl_cluster_fit / icl_ward_values_at and their _dev forms (imageclust_amd/csrc/fit.hip): each clustered row's exact cost against its
own cluster, its nearest alternatives, and each cluster's representative and worst row, with no distance matrix.  Bar: every output
equals the checker's (tests/fit_cases.py: the oracle's values, the rules in plain numpy) -- integers as they are, floats as uint32 bit
patterns (NaN by isnan) -- for every tile edge, both load paths, frozen clusters, bans, ties, NaN / Inf rows and every column-split
count.  No tolerance anywhere."""
import numpy as np
import pytest

from tests import fit_cases as FC
from tests import nearest_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def run(ctx, P, k_alt, dev=False, **over):
    kw = dict(q_size=P["q_size"], c_size=P["c_size"], max_size=P["max_size"])
    kw.update(over)
    return ctx.cluster_fit(P["Q"], P["cluster_of"], P["C"], k_alt, dev=dev, **kw)


def check_problem(ctx, P, k_alts=FC.K_ALTS, forms=(False, True)):
    """Both forms against the checker for each k_alt, from one evaluation of the oracle -> the values"""
    V = FC.values(P["Q"], P["C"], P["q_size"], P["c_size"])
    for k in k_alts:
        want = FC.from_values(V, P["cluster_of"], k, P["q_size"], P["c_size"], P["max_size"])
        for dev in forms:
            got = run(ctx, P, k, dev)
            assert not FC.why(got, want), "k_alt=%d dev=%s: %s" % (k, dev, FC.why(got, want))
    return V


@pytest.mark.parametrize("nq,K,d", FC.CASES)
def test_cases_with_everything_the_rules_can_meet(ctx, nq, K, d):
    P = FC.problem(nq, K, d, 1000 + nq)
    V = check_problem(ctx, P)
    want = FC.from_values(V, P["cluster_of"], 64, P["q_size"], P["c_size"], P["max_size"])
    if nq >= 8 and K >= 5:
        assert not FC.covers(P, want), "the case lacks " + FC.covers(P, want)
    if K == 1:
        assert (want["alt_idx"][P["cluster_of"] == 0] == -1).all()                      # the only cluster is the row's own: all tails


@pytest.mark.parametrize("nq,K,d", FC.CASES)
def test_cases_plain_and_without_sizes(ctx, nq, K, d):
    P = FC.problem(nq, K, d, 2000 + nq, plain=True)
    check_problem(ctx, P, k_alts=(0, 10), forms=(False,))
    P.update(q_size=None, c_size=None, max_size=0)   # NULL sizes: singletons, nothing banned
    check_problem(ctx, P, k_alts=(1, 64), forms=(True,))


@pytest.fixture(scope="module")
def split_problem():
    nq, K, d = FC.SPLIT_CASE
    P = FC.problem(nq, K, d, 31)
    P["C"][650], P["C"][130] = P["C"][3], P["C"][3]   # exact ties between the first and the last split
    P["c_size"][[3, 130, 650]] = 2
    return P, FC.values(P["Q"], P["C"], P["q_size"], P["c_size"])


def test_every_split_count_gives_the_same_bits_and_one_writer_of_own(ctx, split_problem):
    """own is pre-filled with a sentinel on the device: every row must be written (exactly one workgroup meets its column, split 0 the
    rows of no cluster), with the value the run at splits == 1 gives."""
    P, V = split_problem
    nq, K, d = FC.SPLIT_CASE
    qs, cs, cof = P["q_size"], P["c_size"], P["cluster_of"]
    sentinel = np.full(nq, -123.0, np.float32)
    bufs = [ctx.malloc(n) for n in (nq * d * 4, K * d * 4, nq * 4, nq * 64 * 4, nq * 64 * 4, K * 4, K * 4, K * 4)]
    res = {}
    try:
        ctx.h2d(bufs[0], P["Q"])
        ctx.h2d(bufs[1], P["C"])
        for s in (1, 2, 3, 7, 0):
            ctx.set_nearest_options(s)
            for k in (1, 10, 64):
                ctx.h2d(bufs[2], sentinel)
                ctx.cluster_fit_dev(bufs[0], cof, nq, bufs[1], K, d, k, *bufs[2:], q_size=qs, c_size=cs, max_size=P["max_size"])
                ctx.sync()
                out = (np.empty(nq, np.float32), np.empty((nq, k), np.int32), np.empty((nq, k), np.float32), np.empty(K, np.int32),
                       np.empty(K, np.int32), np.empty(K, np.int32))
                for a, p in zip(out, bufs[2:]):
                    ctx.d2h(a, p)
                res[s, k] = dict(zip(FC.FIELDS, out))
                st = ctx.last_fit_stats()
                if s:
                    assert st["splits"] == min(s, 6)   # a forced count holds up to one tile per split: 700 columns are 6 tiles
                assert st["tiles"] == 6 and st["pairs"] == nq * K
                part = 8 * nq * k * st["splits"] if st["splits"] > 1 else 0   # the three host arrays' copies, the partial lists, the keys
                assert 2 * nq * 4 + K * 4 + part + 16 * K <= st["workspace_bytes"] <= 2 * nq * 4 + K * 4 + part + 16 * K + 7 * 16
    finally:
        ctx.set_nearest_options(0)
        for p in bufs:
            ctx.free(p)
    for k in (1, 10, 64):
        want = FC.from_values(V, cof, k, qs, cs, P["max_size"])
        for s in (1, 2, 3, 7, 0):
            assert not (res[s, k]["own"] == -123.0).any(), "splits=%d: a row's own cost was never written" % s
            assert not FC.why(res[s, k], res[1, k]), "splits=%d k=%d against splits=1: %s" % (s, k, FC.why(res[s, k], res[1, k]))
            assert not FC.why(res[s, k], want), "splits=%d k=%d: %s" % (s, k, FC.why(res[s, k], want))


def test_the_two_instantiations_of_the_band_walk_agree(ctx):
    """With no frozen cluster and every row in a cluster, cluster_fit's alternatives ARE nearest's lists with the own cluster excluded,
    and its own costs the listed pairs (i, cluster_of[i]): one kernel body (band_select.h) under two policies, bit for bit, with one
    workgroup per band, with three, and with the engine's own split count."""
    nq, K, d = FC.SPLIT_CASE
    P = FC.problem(nq, K, d, 77, plain=True)
    qs, cs, cof = P["q_size"], P["c_size"], P["cluster_of"]
    assert (cs > 0).all() and (cof >= 0).all()
    own = ctx.ward_values_at(P["Q"], P["C"], np.arange(nq), cof, qs, cs)
    try:
        for s in (1, 3, 0):
            ctx.set_nearest_options(s)
            for k in (1, 64):
                fit = run(ctx, P, k)
                idx, val = ctx.nearest(P["Q"], P["C"], k, qs, cs, P["max_size"], exclude=cof)
                assert ctx.last_fit_stats()["splits"] == ctx.last_nearest_stats()["splits"] and (s == 0 or ctx.last_fit_stats()["splits"] == s)
                assert np.array_equal(fit["alt_idx"], idx), "splits=%d k=%d" % (s, k)
                assert np.array_equal(fit["alt_val"].view(np.uint32), val.view(np.uint32)), "splits=%d k=%d" % (s, k)
                assert np.array_equal(fit["own"].view(np.uint32), own.view(np.uint32)), "splits=%d k=%d" % (s, k)
    finally:
        ctx.set_nearest_options(0)


def test_empty_sides(ctx):
    P = FC.problem(6, 5, 8, 41)
    r = ctx.cluster_fit(np.zeros((0, 8), np.float32), np.zeros(0, np.int32), P["C"], 3, c_size=P["c_size"])   # nq == 0
    assert r["own"].shape == (0,) and r["alt_idx"].shape == (0, 3)
    assert (r["listed"] == 0).all() and (r["rep"] == -1).all() and (r["worst"] == -1).all()
    r = ctx.cluster_fit(np.zeros((0, 8), np.float32), np.zeros(0, np.int32), P["C"], 3, dev=True)
    assert (r["listed"] == 0).all() and (r["rep"] == -1).all() and (r["worst"] == -1).all()
    none = np.full(6, -1, np.int32)
    for k in (0, 4):                                                                                         # K == 0, every row in no cluster
        for dev in (False, True):
            r = ctx.cluster_fit(P["Q"], none, np.zeros((0, 8), np.float32), k, q_size=P["q_size"], dev=dev)
            assert (r["own"] == FC.MAXF).all() and (r["alt_idx"] == -1).all() and (r["alt_val"] == FC.MAXF).all() and r["rep"].shape == (0,)
    assert ctx.last_fit_stats()["tiles"] == 0


def test_values_of_listed_pairs(ctx):
    from imageclust_amd import _lib

    for (nq, K, d), seed in zip(FC.CASES + [FC.SPLIT_CASE], range(50, 60)):
        P = FC.problem(nq, K, d, seed)
        V = FC.values(P["Q"], P["C"], P["q_size"], P["c_size"])
        rng = np.random.default_rng(seed)
        for npairs in (1, 63, 64, 65, 1000):
            qi, ej = rng.integers(0, nq, npairs).astype(np.int32), rng.integers(0, K, npairs).astype(np.int32)
            qi[-1], ej[-1] = nq - 1, K - 1                       # the last row and column
            if npairs > 2:
                qi[1], ej[1] = qi[0], ej[0]                      # a pair listed twice
            for dev in (False, True):
                got = ctx.ward_values_at(P["Q"], P["C"], qi, ej, q_size=P["q_size"], e_size=P["c_size"], dev=dev)
                want = V[qi, ej]
                bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
                assert not len(bad), "(%d, %d, %d) np=%d dev=%s: %d differ, first pair %d" % (nq, K, d, npairs, dev, len(bad), bad[0])
    P = FC.problem(9, 7, 2048, 61, plain=True)                   # a long chain, sizes NULL
    got = ctx.ward_values_at(P["Q"], P["C"], np.arange(9) % 9, np.arange(9) % 7)
    assert np.array_equal(got.view(np.uint32), NC.oracle_values(P["Q"], P["C"])[np.arange(9), np.arange(9) % 7].view(np.uint32))
    assert ctx.ward_values_at(P["Q"], P["C"], [], []).shape == (0,)
    for kw in (dict(qi=[9], ej=[0]), dict(qi=[-1], ej=[0]), dict(qi=[0], ej=[7]), dict(qi=[0], ej=[-1]), dict(qi=[0], ej=[0], q_size=[1] * 8 + [0]),
               dict(qi=[0], ej=[0], e_size=[1, 0, 1, 1, 1, 1, 1])):
        with pytest.raises(_lib.ICLError) as ei:
            ctx.ward_values_at(P["Q"], P["C"], **kw)
        assert ei.value.code == _lib.ICL_ERR_ARG, kw


def test_bad_arguments_write_nothing(ctx):
    from imageclust_amd import _lib

    L = ctx.L
    nq, K, d, k = 5, 4, 6, 3
    P = FC.problem(nq, K, d, 71, plain=True)
    Q, Cm, cof, qs, cs = P["Q"], P["C"], P["cluster_of"], P["q_size"], P["c_size"]
    outs = [np.full(nq, 77.0, np.float32), np.full((nq, 64), 77, np.int32), np.full((nq, 64), 77.0, np.float32), np.full(K, 77, np.int32),
            np.full(K, 77, np.int32), np.full(K, 77, np.int32)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(Q=Q, qs=qs, cof=cof, nq=nq, Cm=Cm, cs=cs, K=K, d=d, k=k, own=outs[0], ai=outs[1], av=outs[2]):
        return L.icl_cluster_fit(ctx.h, p(Q), p(qs), p(cof), nq, p(Cm), p(cs), K, d, k, 0, p(own), p(ai), p(av), p(outs[3]), p(outs[4]), p(outs[5]))

    bad_q, bad_c, hi, lo = qs.copy(), cs.copy(), cof.copy(), cof.copy()
    bad_q[1], bad_c[3], hi[2], lo[0] = 0, 0, K, -2
    cases = dict(null_Q=dict(Q=None), null_cof=dict(cof=None), null_C=dict(Cm=None), null_own=dict(own=None), null_idx=dict(ai=None),
                 null_val=dict(av=None), k_neg=dict(k=-1), k65=dict(k=65), d0=dict(d=0), neg_nq=dict(nq=-1), neg_K=dict(K=-1), huge_K=dict(K=1 << 31),
                 q_size_0=dict(qs=bad_q), c_size_0=dict(cs=bad_c), cof_K=dict(cof=hi), cof_below=dict(cof=lo), no_clusters=dict(K=0))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ICL_ERR_ARG, name
        assert all((a == 77).all() for a in outs), name
    assert L.icl_cluster_fit(None, p(Q), p(qs), p(cof), nq, p(Cm), p(cs), K, d, k, 0, *[p(a) for a in outs]) == _lib.ICL_ERR_ARG
    val = np.full(4, 77.0, np.float32)
    pairs = np.array([0, 1, 2, nq], np.int32), np.array([0, 1, 2, 0], np.int32)
    assert L.icl_ward_values_at(ctx.h, p(Q), p(qs), nq, p(Cm), p(cs), K, d, p(pairs[0]), p(pairs[1]), 4, p(val)) == _lib.ICL_ERR_ARG
    assert L.icl_ward_values_at(ctx.h, p(Q), p(qs), nq, p(Cm), p(cs), K, 0, p(pairs[1]), p(pairs[1]), 4, p(val)) == _lib.ICL_ERR_ARG
    assert (val == 77.0).all()
    assert call() == _lib.ICL_OK and (outs[1].reshape(-1)[nq * k:] == 77).all()   # rows of k entries, back to back


@pytest.fixture(scope="module")
def seeded_run(ctx):
    """A full seeded run on 600 rows with its final centroids, and the image-level view of it"""
    n, d = 600, 12
    rng = np.random.default_rng(81)
    E = (rng.standard_normal((40, d))[rng.integers(0, 40, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    cid, rank, nc, st, mg, co = ctx.cluster_seeded(E, np.ones(n, np.int32), 3, 30, 0, want_centroids=True)
    from imageclust_amd import _lib

    assert st == _lib.ICL_OK
    first = np.flatnonzero(np.any(co != 0, axis=1))      # C_out holds a final cluster's centroid at its first seed
    # the final cluster of every row from the merge log
    members = {i: [i] for i in range(n)}
    for t, (a, b) in enumerate(np.asarray(mg).reshape(-1, 2)):
        members[n + t] = members.pop(int(a)) + members.pop(int(b))
    cof, sizes, C = np.full(n, -1, np.int32), [], []
    for c, rows in sorted(members.items(), key=lambda kv: kv[1][0]):
        assert rows[0] in first or len(rows) == 1
        cof[rows] = len(C)
        C.append(co[rows[0]] if len(rows) > 1 else E[rows[0]])
        sizes.append(len(rows))
    return E, np.stack(C).astype(np.float32), np.array(sizes, np.int32), cof


def test_fit_of_a_finished_seeded_run(ctx, seeded_run):
    E, C, sizes, cof = seeded_run
    assert (cof >= 0).all() and len(C) > 10
    want = FC.expected(E, C, cof, 3, None, sizes, 30)
    got = ctx.cluster_fit(E, cof, C, 3, c_size=sizes, max_size=30)
    assert not FC.why(got, want), FC.why(got, want)
    assert (got["listed"] == sizes).all() and (cof[got["rep"]] == np.arange(len(C))).all()


def test_clustering_fit_through_the_context_equals_the_stand_in(ctx):
    from imageclust_amd import clustering as CL

    rng = np.random.default_rng(91)
    E = (rng.standard_normal((6, 10))[rng.integers(0, 6, 48)] + 0.2 * rng.standard_normal((48, 10))).astype(np.float32)
    ids = ["img_%d" % i for i in range(48)]
    real = CL.Clustering.start(E, ids, 2, 9, ctx=ctx)
    real.freeze([ids[0]])

    def stand_in(Q, cluster_of, C, k_alt, q_size, c_size, max_size):
        return FC.expected(Q, C, cluster_of, k_alt, q_size, c_size, max_size)

    twin = CL.Clustering(2, 9, fit_engine=stand_in)
    twin.clusters, twin.embeddings = real.clusters, real.embeddings
    assert real.fit(3) == twin.fit(3) and len(real.fit(3)) == 48
    assert real.representatives() == twin.representatives()
    assert real.misfits() == twin.misfits()


def test_other_reports_are_left_alone(ctx):
    E = NC.random_rows(40, 8, 95)
    ctx.cluster(E, 2, 6)
    ctx.nearest(E[:5], E, 3)
    before = (ctx.last_merges().copy(), ctx.last_ward_mode(), ctx.last_ward_layout(), ctx.last_ward_stats(), ctx.last_nearest_stats())
    P = FC.problem(9, 6, 8, 96)
    run(ctx, P, 4)
    run(ctx, P, 0)
    ctx.ward_values_at(P["Q"], P["C"], [0, 1], [2, 3])
    after = (ctx.last_merges(), ctx.last_ward_mode(), ctx.last_ward_layout(), ctx.last_ward_stats(), ctx.last_nearest_stats())
    assert np.array_equal(before[0], after[0]) and before[1:] == after[1:]
