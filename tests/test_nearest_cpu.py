"""icl_nearest_from_matrix (imageclust_amd/csrc/nearest.hip + nearest_select.h, host only) and the Python layer over icl_nearest
(NearDuplicates, Clustering.nearest) through stub engines: the leave-out and order rules against the plain-numpy checker of
tests/nearest_cases.py.  No GPU."""
import numpy as np
import pytest

from tests import nearest_cases as NC


def from_matrix(D, k, **kw):
    from imageclust_amd import _lib

    return _lib.nearest_from_matrix(D, k, **kw)


def check(D, k, q_size=None, e_size=None, max_size=0, exclude=None):
    got = from_matrix(D, k, q_size=q_size, e_size=e_size, max_size=max_size, exclude=exclude)
    want = NC.select(D, k, q_size, e_size, max_size, exclude)
    assert NC.same(got, want), NC.why(got, want)
    return got


@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("nq,n", [(1, 1), (3, 5), (9, 64), (17, 200)])
def test_random_matrices(nq, n, k):
    check(np.random.default_rng(nq * 1000 + n).standard_normal((nq, n)).astype(np.float32), k)  # (k > n where n < 64: short rows)


@pytest.mark.parametrize("k", [1, 7, 64])
def test_ties_dominate(k):
    D = np.random.default_rng(5).integers(0, 3, (11, 150)).astype(np.float32)
    D[D == 1] = np.float32(-0.0)  # -0 and +0 compare equal: the tie goes by j
    check(D, k)


@pytest.mark.parametrize("k", [1, 7, 64])
def test_nan_and_inf(k):
    D = np.random.default_rng(6).standard_normal((8, 90)).astype(np.float32)
    D[0, :] = np.nan
    D[1, ::2] = np.nan
    D[2, :] = np.inf
    D[3, 5:70] = np.inf
    D[3, 70:] = np.nan
    D[4, 10] = -np.inf
    D[5, :] = NC.MAXF  # a real value equal to the tail's: still listed, with its column
    idx, val = check(D, k)
    assert np.isnan(val[0]).all() and (idx[0] == np.arange(k)).all()  # NaN among themselves by j
    assert (idx[5] == np.arange(k)).all()


def test_exclude_and_bans():
    rng = np.random.default_rng(7)
    nq, n = 12, 40
    D = rng.integers(0, 5, (nq, n)).astype(np.float32)
    qs, es = NC.mixed_sizes(nq, 1), NC.mixed_sizes(n, 2)
    ex = rng.integers(-1, n, nq).astype(np.int64)
    for k in (1, 7, 64):
        check(D, k, exclude=ex)
        check(D, k, q_size=qs, e_size=es, max_size=10)
        check(D, k, q_size=qs, e_size=es, max_size=10, exclude=ex)
        check(D, k, e_size=es, max_size=4)       # q_size NULL: singletons
        check(D, k, q_size=qs, max_size=6)       # e_size NULL
        check(D, k, q_size=qs, e_size=es, max_size=0)  # no ban: the sizes do not matter
    idx, val = check(D, 7, q_size=np.full(nq, 9, np.int32), e_size=es, max_size=9)  # every pair banned
    assert (idx == -1).all() and (val == NC.MAXF).all()
    idx, _ = check(np.zeros((3, 3), np.float32), 2, exclude=np.arange(3))  # a self-join's diagonal
    assert idx.tolist() == [[1, 2], [0, 2], [0, 1]]


def test_no_columns_and_no_rows():
    idx, val = from_matrix(np.zeros((4, 0), np.float32), 3)
    assert idx.shape == (4, 3) and (idx == -1).all() and (val == NC.MAXF).all()
    idx, val = from_matrix(np.zeros((0, 6), np.float32), 3)
    assert idx.shape == (0, 3) and val.shape == (0, 3)


def test_leading_dimension():
    D = np.random.default_rng(8).integers(0, 4, (6, 50)).astype(np.float32)
    D[:, 33:] = -1.0  # beyond n: must never be listed
    es = NC.mixed_sizes(33, 3)
    got = from_matrix(D, 7, e_size=es, max_size=5, n=33)
    want = NC.select(D[:, :33], 7, None, es, 5, None)
    assert NC.same(got, want), NC.why(got, want)


def test_bad_arguments_write_nothing():
    from imageclust_amd import _lib

    L = _lib.load()
    nq, n, k = 3, 5, 4
    D = np.zeros((nq, n), np.float32)
    ok_q, ok_e, ok_x = np.ones(nq, np.int32), np.ones(n, np.int32), np.full(nq, -1, np.int64)
    idx, val = np.full((nq, 64), 77, np.int32), np.full((nq, 64), 77.0, np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(D=D, nq=nq, n=n, ld=n, qs=ok_q, es=ok_e, k=k, ex=ok_x, idx=idx, val=val):
        return L.icl_nearest_from_matrix(p(D), nq, n, ld, p(qs), p(es), k, 0, p(ex), p(idx), p(val))

    bad_q, bad_e = ok_q.copy(), ok_e.copy()
    bad_q[1], bad_e[4] = 0, -2
    hi, lo = ok_x.copy(), ok_x.copy()
    hi[2], lo[0] = n, -2
    cases = dict(null_D=dict(D=None), null_idx=dict(idx=None), null_val=dict(val=None), k0=dict(k=0), k65=dict(k=65), neg_nq=dict(nq=-1),
                 neg_n=dict(n=-1), huge_n=dict(n=1 << 31, ld=1 << 31), short_ld=dict(ld=n - 1), q_size_0=dict(qs=bad_q), e_size_neg=dict(es=bad_e),
                 exclude_n=dict(ex=hi), exclude_below=dict(ex=lo))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ICL_ERR_ARG, name
        assert (idx == 77).all() and (val == 77.0).all(), name
    assert call() == _lib.ICL_OK  # rows of k entries, back to back: all values tie, so each row lists columns 0 .. k - 1
    assert (idx.reshape(-1)[:nq * k].reshape(nq, k) == np.arange(k)).all() and (idx.reshape(-1)[nq * k:] == 77).all()
    with pytest.raises(_lib.ICLError) as ei:
        _lib.nearest_from_matrix(D, 65)
    assert ei.value.code == _lib.ICL_ERR_ARG


# ---- the Python layer, with the checker standing in for the GPU ---------------------------------------------------------------
class StubContext:
    """Context.nearest by the checker"""

    def __init__(self):
        self.calls = []

    def nearest(self, Q, E, k, q_size=None, e_size=None, max_size=0, exclude=None, dev=False):
        self.calls.append(dict(nq=len(Q), n=len(E), k=k, max_size=max_size, exclude=exclude))
        return NC.expected(Q, E, k, q_size, e_size, max_size, exclude)


def test_near_duplicates_each_pair_once():
    from imageclust_amd import clustering as CL

    E = NC.random_rows(40, 12, 9)
    E[7] = E[3]             # an exact duplicate: value 0
    E[21] = E[3]
    E[30] = E[12] + np.float32(1e-3)
    ids = ["img_%d" % i for i in range(40)]
    stub = StubContext()
    V = NC.oracle_values(E, E)
    thr = float(V[12, 30]) * 1.5
    got = CL.NearDuplicates(E, ids, 5, thr, ctx=stub)
    want = [(ids[a], ids[b], float(V[a, b])) for a in range(40) for b in range(a + 1, 40) if V[a, b] <= thr]
    assert got == want and len(got) == len({(a, b) for a, b, _ in got})
    assert {(a, b) for a, b, _ in got} == {("img_3", "img_7"), ("img_3", "img_21"), ("img_7", "img_21"), ("img_12", "img_30")}
    assert stub.calls[0]["exclude"].tolist() == list(range(40)) and stub.calls[0]["max_size"] == 0
    assert CL.NearDuplicates(np.zeros((0, 12), np.float32), [], 5, 1.0, ctx=stub) == []
    # k = 1: img_3 lists img_7 only, img_21 lists img_3: the pair (3, 21) still comes out, once
    got1 = CL.NearDuplicates(E, ids, 1, 0.0, ctx=stub)
    assert [g[:2] for g in got1] == [("img_3", "img_7"), ("img_3", "img_21")]


def test_clustering_nearest_through_the_stub_engine():
    from imageclust_amd import clustering as CL

    d = 6
    rows = NC.random_rows(9, d, 10)
    ids = ["p%d" % i for i in range(9)]
    seen = []

    def engine(Q, E, k, q_size, e_size, max_size):
        seen.append((len(Q), len(E), k, list(map(int, q_size)), list(map(int, e_size)), max_size))
        return NC.expected(Q, E, k, q_size, e_size, max_size)

    st = CL.Clustering(2, 3, nearest_engine=engine)
    st.add(rows, ids)
    H = CL.HeldCluster
    st.clusters = [H(["p4", "p0"], rows[[4, 0]].mean(0)), H(["p1", "p2", "p3"], rows[[1, 2, 3]].mean(0)),  # named p4 (first member); full
                   H(["p5"], rows[5].copy(), Frozen=True), H(["p6", "p7"], rows[[6, 7]].mean(0)), H(["p8"], rows[8].copy())]
    Q = np.stack([rows[5], rows[0] + 0.01, rows[8]])
    out = st.nearest(Q, 4)
    assert seen == [(3, 4, 4, [1, 1, 1], [2, 3, 2, 1], 3)]  # the frozen cluster is not offered
    cand = [st.clusters[i] for i in (0, 1, 3, 4)]
    V = NC.oracle_values(Q, np.stack([c.Centroid for c in cand]).astype(np.float32), np.ones(3, np.int32), np.array([2, 3, 2, 1], np.int32))
    for qi, lst in enumerate(out):
        names = [nm for nm, _ in lst]
        assert "p1" not in names and "p5" not in names            # full (3 + 1 > maxSize) and frozen clusters are absent
        assert sorted(names) == ["p4", "p6", "p8"]                # named by first member; a short row (3 of k = 4) has no filler
        order = sorted([0, 2, 3], key=lambda c: (V[qi, c], c))
        assert lst == [(cand[c].Members[0], float(V[qi, c])) for c in order]
    assert out[2][0] == ("p8", 0.0)
    assert len(st.clusters) == 5 and st.nearest(np.zeros((0, d), np.float32), 4) == []
    for c in st.clusters:
        c.Frozen = True
    assert st.nearest(Q, 4) == [[], [], []] and len(seen) == 1
