"""icl_nearest / icl_nearest_dev (imageclust_amd/csrc/nearest.hip): each query's k nearest library clusters by exact WardDistance, with
no distance matrix.  Bar: idx equals the checker's (tests/nearest_cases.py: the oracle's values, the leave-out rules and a stable sort
in plain numpy) and val equals it as uint32 bit patterns (NaN by isnan), for every tile edge, both load paths, ties, bans, excluded
columns, NaN / Inf rows and every column-split count."""
import numpy as np
import pytest

from tests import nearest_cases as NC

pytestmark = pytest.mark.gpu

KS = (1, 7, 64)


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, Q, E, ks=KS, V=None, **kw):
    """ctx.nearest against the checker for each k; V: the oracle's values when the caller already holds them"""
    V = NC.oracle_values(Q, E, kw.get("q_size"), kw.get("e_size")) if V is None else V
    for k in ks:
        got = ctx.nearest(Q, E, k, **kw)
        want = NC.select(V, k, kw.get("q_size"), kw.get("e_size"), kw.get("max_size", 0), kw.get("exclude"))
        assert NC.same(got, want), "k=%d: %s" % (k, NC.why(got, want))
    return V


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 300])
@pytest.mark.parametrize("nq", [1, 5, 129])
def test_tile_edges(ctx, nq, n):
    check(ctx, NC.random_rows(nq, 36, 100 + nq), NC.random_rows(n, 36, 200 + n))


@pytest.mark.parametrize("d", [1, 3, 4, 1001, 2048])
def test_both_load_paths_and_a_long_chain(ctx, d):
    check(ctx, NC.random_rows(5, d, 300 + d), NC.random_rows(129, d, 400 + d))


def test_exact_ties_inside_and_across_tiles_and_splits(ctx):
    E = NC.tie_rows(300, 36, 11)     # 7 patterns over 300 rows: every value is shared by dozens of columns in each of the 3 tiles
    Q = np.concatenate([E[:3], NC.tie_rows(6, 36, 12)])
    V = check(ctx, Q, E)
    assert (V[0] == 0).sum() > 20
    try:
        for s in (2, 3):
            ctx.set_nearest_options(s)
            check(ctx, Q, E, V=V)
            assert ctx.last_nearest_stats()["splits"] == s
    finally:
        ctx.set_nearest_options(0)


def test_mixed_sizes_and_bans(ctx):
    Q, E = NC.random_rows(9, 36, 13), NC.random_rows(200, 36, 14)
    qs, es = NC.mixed_sizes(9, 15), NC.mixed_sizes(200, 16, lo=2)
    qs[0] = 12                    # 12 + anything > 12: the ban empties this row
    qs[1] = 11                    # only the singletons of E remain ...
    es[:200:29] = 1               # ... 7 of them: fewer than k = 64
    V = check(ctx, Q, E, q_size=qs, e_size=es, max_size=12)
    idx, val = ctx.nearest(Q, E, 7, q_size=qs, e_size=es, max_size=12)
    assert (idx[0] == -1).all() and (val[0] == NC.MAXF).all()
    left = int((es == 1).sum())
    idx, _ = ctx.nearest(Q, E, 64, q_size=qs, e_size=es, max_size=12)
    assert (idx[1] >= 0).sum() == left < 64 and (idx[1, left:] == -1).all()
    check(ctx, Q, E, V=V, q_size=qs, e_size=es, max_size=0)          # the same values, nothing banned
    check(ctx, Q, E, q_size=qs)                                       # one side's sizes only
    check(ctx, Q, E, e_size=es, max_size=5)
    ex = np.array([-1, 0, 199, 5, -1, 128, 127, 64, 63], np.int64)
    check(ctx, Q, E, V=V, q_size=qs, e_size=es, max_size=12, exclude=ex)


def test_self_join_equals_the_distance_matrix(ctx):
    E = NC.random_rows(300, 36, 17)
    E[250] = E[4]
    sizes = NC.mixed_sizes(300, 18)
    ex = np.arange(300, dtype=np.int64)
    for sz in (None, sizes):
        V = check(ctx, E, E, q_size=sz, e_size=sz, exclude=ex)
        D = ctx.ward_distance_matrix(E, sz)
        assert np.array_equal(D.view(np.uint32)[~np.eye(300, dtype=bool)], V.view(np.uint32)[~np.eye(300, dtype=bool)])
        for k in KS:  # ... and a stable sort of the engine's own matrix rows gives the same lists, bit for bit
            got = ctx.nearest(E, E, k, q_size=sz, e_size=sz, exclude=ex)
            want = NC.select(D, k, exclude=ex)
            assert NC.same(got, want), NC.why(got, want)


def test_nan_and_inf_rows(ctx):
    E = NC.random_rows(260, 36, 19)
    E[70, 3] = np.nan      # every pair with row 70 is NaN: behind every number
    E[200, :] = np.inf     # every pair with row 200 is +Inf (Inf - x = Inf); (Inf - Inf would be NaN: no query holds Inf)
    E[131, 35] = np.nan
    Q = NC.random_rows(6, 36, 20)
    V = check(ctx, Q, E, ks=(1, 7, 64))
    assert np.isnan(V[:, 70]).all() and np.isinf(V[:, 200]).all()
    es = np.full(260, 5, np.int32)
    es[[70, 131, 200, 7]] = 1
    got = ctx.nearest(Q, E, 7, e_size=es, max_size=2)   # what remains: one number, Inf, then the two NaN columns by j
    assert (got[0][:, :4] == [7, 200, 70, 131]).all() and (got[0][:, 4:] == -1).all()
    want = NC.expected(Q, E, 7, None, es, 2)
    assert NC.same(got, want), NC.why(got, want)


@pytest.fixture(scope="module")
def split_case():
    Q = NC.random_rows(5, 8, 21)
    E = NC.random_rows(3000, 8, 22)
    E[2900] = E[17]         # exact ties between the first and the last split
    E[1500] = E[17]
    Q[0] = E[17]
    es = NC.mixed_sizes(3000, 23)
    return Q, E, es, NC.oracle_values(Q, E, None, es)


def test_forced_splits_and_auto_agree(ctx, split_case):
    Q, E, es, V = split_case
    res = {}
    try:
        for s in (1, 2, 3, 7, 0):
            ctx.set_nearest_options(s)
            for k in KS:
                res[s, k] = ctx.nearest(Q, E, k, e_size=es, max_size=8)
                st = ctx.last_nearest_stats()
                if s:
                    assert st["splits"] == s
                assert st["tiles"] == 24 and st["pairs"] == 5 * 3000 and st["splits"] >= 1
                part = 8 * 5 * k * st["splits"] if st["splits"] > 1 else 0  # e_size's copy, and the partial lists when there are any
                assert 3000 * 4 + part <= st["workspace_bytes"] <= 3000 * 4 + part + 64
    finally:
        ctx.set_nearest_options(0)
    for k in KS:
        want = NC.select(V, k, None, es, 8, None)
        for s in (1, 2, 3, 7, 0):
            assert NC.same(res[s, k], want), "splits=%d k=%d: %s" % (s, k, NC.why(res[s, k], want))
            assert NC.same(res[s, k], res[1, k])


def test_host_buffers_equal_device_buffers(ctx, split_case):
    Q, E, es, _ = split_case
    qs = NC.mixed_sizes(5, 24)
    ex = np.array([17, -1, 2999, 0, 128], np.int64)
    for k in KS:
        a = ctx.nearest(Q, E, k, q_size=qs, e_size=es, max_size=9, exclude=ex)
        b = ctx.nearest(Q, E, k, q_size=qs, e_size=es, max_size=9, exclude=ex, dev=True)
        assert NC.same(a, b), NC.why(a, b)


def test_empty_sides_and_bad_arguments(ctx):
    from imageclust_amd import _lib

    Q = NC.random_rows(3, 8, 25)
    idx, val = ctx.nearest(Q, np.zeros((0, 8), np.float32), 4)
    assert (idx == -1).all() and (val == NC.MAXF).all() and idx.shape == (3, 4)
    idx, val = ctx.nearest(np.zeros((0, 8), np.float32), Q, 4)
    assert idx.shape == (0, 4)
    E = NC.random_rows(6, 8, 26)
    for kw in (dict(k=0), dict(k=65), dict(k=2, q_size=[1, 0, 1]), dict(k=2, e_size=[1, 1, 1, 1, 1, -3]), dict(k=2, exclude=[0, 6, 1]),
               dict(k=2, exclude=[-2, 0, 1])):
        with pytest.raises(_lib.ICLError) as ei:
            ctx.nearest(Q, E, **kw)
        assert ei.value.code == _lib.ICL_ERR_ARG, kw
    with pytest.raises(_lib.ICLError) as ei:
        ctx.set_nearest_options(-1)
    assert ei.value.code == _lib.ICL_ERR_ARG
