"""icl_pairs_within_from_matrix and icl_pair_groups (imageclust_amd/csrc/pairs.hip + pairs_select.h, host only) and the Python layer over
icl_pairs_within (DuplicatePairs, DuplicateGroups) through a stub engine: the pair rule, the CSR layout and the capacity convention
against the plain-numpy checker of tests/pairs_cases.py.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import pairs_cases as PC


def from_matrix(D, thr, **kw):
    from imageclust_amd import _lib

    return _lib.pairs_within_from_matrix(D, thr, **kw)


def check(D, thr):
    got, want = from_matrix(D, thr), PC.select(D, thr)
    assert PC.same(got, want), PC.why(got, want)
    return got


@pytest.mark.parametrize("n", [0, 1, 2, 5, 64, 200])
def test_random_matrices(n):
    D = np.random.default_rng(n).standard_normal((n, n)).astype(np.float32)
    for thr in (-10.0, -0.5, 0.0, 0.5, 10.0):
        check(D, thr)


def test_ties_and_signed_zeros():
    D = np.random.default_rng(5).integers(0, 3, (90, 90)).astype(np.float32)
    D[D == 1] = np.float32(-0.0)
    for thr in (0.0, -0.0, 2.0, np.nextafter(np.float32(2.0), np.float32(0.0)), np.nextafter(np.float32(0.0), np.float32(-1.0))):
        rp, col, val = check(D, thr)
    assert rp[-1] == 0                                       # just below zero: neither zero is listed
    rp0, _, val0 = check(D, np.float32(-0.0))
    assert rp0[-1] == int((PC.lower_values(D) == 0).sum()) > 1000 and np.signbit(val0).any() and not np.signbit(val0).all()
    assert check(D, 2.0)[0][-1] == 90 * 89 // 2 > check(D, np.nextafter(np.float32(2.0), np.float32(0.0)))[0][-1]


def test_nan_inf_and_a_real_maxfloat():
    D = np.random.default_rng(6).standard_normal((40, 40)).astype(np.float32)
    D[5, :] = np.nan
    D[9, :] = np.inf
    D[20, 3] = -np.inf
    D[30, :] = PC.MAXF
    D[:, 7] = np.nan
    low = PC.lower_values(D)
    for thr, count in ((np.inf, int((~np.isnan(low)).sum())), (PC.MAXF, int((low <= PC.MAXF).sum())), (-np.inf, 1), (0.0, None)):
        rp, col, val = check(D, thr)
        assert not np.isnan(val).any()
        assert count is None or rp[-1] == count
    rp, col, val = check(D, PC.MAXF)
    assert (val[rp[30]:rp[31]] == PC.MAXF).sum() == 29 and not np.isinf(val[val > 0]).any()  # row 30 without its NaN column
    assert rp[6] - rp[5] == 0                                 # a NaN row lists nothing, whatever the threshold
    assert check(D, -np.inf)[1].tolist() == [3]


def test_leading_dimension():
    D = np.random.default_rng(8).integers(0, 4, (50, 50)).astype(np.float32)
    got = from_matrix(D, 1.0, n=33)
    want = PC.select(D[:33, :33], 1.0)
    assert PC.same(got, want), PC.why(got, want)


def test_capacity_convention_and_bad_arguments_write_nothing():
    from imageclust_amd import _lib

    L = _lib.load()
    n = 6
    D = np.random.default_rng(9).integers(0, 3, (n, n)).astype(np.float32)
    wr, wc, wv = PC.select(D, 1.0)
    total = int(wr[-1])
    assert 2 < total < n * (n - 1) // 2
    p = lambda a: None if a is None else a.ctypes.data
    rp, col, val = np.full(n + 1, 77, np.int64), np.full(32, 77, np.int32), np.full(32, 77.0, np.float32)
    tot = ctypes.c_int64(-5)

    def call(D=D, n=n, ld=n, thr=1.0, rp=rp, col=col, val=val, cap=32, tot=tot):
        return L.icl_pairs_within_from_matrix(p(D), n, ld, thr, p(rp), p(col), p(val), cap, None if tot is None else ctypes.byref(tot))

    cases = dict(null_D=dict(D=None), null_row_ptr=dict(rp=None), null_total=dict(tot=None), null_col=dict(col=None), null_val=dict(val=None),
                 null_both_with_cap=dict(col=None, val=None, cap=3), neg_n=dict(n=-1), huge_n=dict(n=1 << 31, ld=1 << 31),
                 short_ld=dict(ld=n - 1), neg_cap=dict(cap=-1), nan_threshold=dict(thr=float("nan")))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ICL_ERR_ARG, name
        assert (rp == 77).all() and (col == 77).all() and (val == 77.0).all() and tot.value == -5, name
    # the size query
    assert call(col=None, val=None, cap=0) == _lib.ICL_OK and tot.value == total and np.array_equal(rp, wr)
    # one short: ICL_ERR_ARG with row_ptr and total complete
    rp[:], tot.value = 77, -5
    assert call(cap=total - 1) == _lib.ICL_ERR_ARG and tot.value == total and np.array_equal(rp, wr) and (col == 77).all()
    # exactly enough
    rp[:] = 77
    assert call(cap=total) == _lib.ICL_OK and np.array_equal(rp, wr)
    assert PC.same((rp, col[:total], val[:total]), (wr, wc, wv)) and (col[total:] == 77).all() and (val[total:] == 77.0).all()
    # n <= 1: ICL_OK, no pairs, D not needed
    for m in (0, 1):
        rp[:], tot.value = 77, -5
        assert call(D=None, n=m, ld=m) == _lib.ICL_OK and tot.value == 0 and (rp[:m + 1] == 0).all() and (rp[m + 1:] == 77).all()
    with pytest.raises(_lib.ICLError) as ei:
        _lib.pairs_within_from_matrix(D, float("nan"))
    assert ei.value.code == _lib.ICL_ERR_ARG


# ---- icl_pair_groups -------------------------------------------------------------------------------------------------------------
def csr(n, pairs):
    """CSR of the pair set {(i, j)}, j < i"""
    rows = [sorted(j for i2, j in pairs if i2 == i) for i in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rp, np.array([j for r in rows for j in r], np.int32)


def groups(n, pairs):
    from imageclust_amd import _lib

    g, ng = _lib.pair_groups(*csr(n, pairs))
    return g.tolist(), ng


def test_pair_groups():
    assert groups(0, []) == ([], 0)
    assert groups(4, []) == ([0, 1, 2, 3], 0)                                       # no pairs: everyone alone
    assert groups(5, [(1, 0), (2, 1), (3, 2), (4, 3)]) == ([0] * 5, 1)              # a chain
    assert groups(6, [(5, 1), (4, 1), (3, 1), (2, 1)]) == ([0, 1, 1, 1, 1, 1], 1)   # a star whose centre is not row 0
    assert groups(7, [(2, 0), (4, 3), (5, 4)]) == ([0, 1, 0, 3, 3, 3, 6], 2)
    # two components that join only through a late row, the higher root first
    assert groups(8, [(3, 1), (5, 2), (6, 5), (7, 3), (7, 6)]) == ([0, 1, 1, 1, 4, 1, 1, 1], 1)
    assert groups(6, [(3, 2), (4, 1), (5, 3), (5, 4)]) == ([0, 1, 1, 1, 1, 1], 1)
    # against a plain flood fill on a random graph
    rng = np.random.default_rng(3)
    n = 200
    pairs = {(int(max(a, b)), int(min(a, b))) for a, b in rng.integers(0, n, (90, 2)) if a != b}
    want = list(range(n))
    changed = True
    while changed:
        changed = False
        for i, j in pairs:
            m = min(want[i], want[j])
            if want[i] != m or want[j] != m:
                want[i] = want[j] = m
                changed = True
    got, ng = groups(n, pairs)
    assert got == want and ng == sum(1 for r in set(want) if want.count(r) >= 2)


def test_pair_groups_malformed_csr():
    from imageclust_amd import _lib

    L = _lib.load()
    n = 4
    group, ng = np.full(n, 77, np.int32), ctypes.c_int64(-5)
    p = lambda a: None if a is None else a.ctypes.data

    def call(rp, col, n=n, group=group, ng=ng):
        rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int32)
        return L.icl_pair_groups(n, p(rp), p(col) if col.size else None, p(group), None if ng is None else ctypes.byref(ng))

    bad = dict(decreasing=([0, 2, 1, 2, 3], [0, 0, 0]), first_not_0=([1, 1, 1, 1, 1], [0]), self_pair=([0, 0, 1, 1, 1], [1]),
               upper_triangle=([0, 1, 1, 1, 1], [2]), negative_col=([0, 0, 1, 1, 1], [-1]), no_col=([0, 0, 1, 1, 1], []))
    for name, (rp, col) in bad.items():
        assert call(rp, col) == _lib.ICL_ERR_ARG, name
        assert (group == 77).all() and ng.value == -5, name
    assert call([0, 0, 1, 1, 1], [0], n=-1) == _lib.ICL_ERR_ARG and call([0, 0, 1, 1, 1], [0], group=None) == _lib.ICL_ERR_ARG
    assert call([0, 0, 1, 1, 1], [0], ng=None) == _lib.ICL_ERR_ARG and (group == 77).all()
    assert call([0, 0, 1, 1, 1], [0]) == _lib.ICL_OK and group.tolist() == [0, 0, 2, 3] and ng.value == 1
    with pytest.raises(_lib.ICLError):
        _lib.pair_groups([0, 1], [0])


# ---- the Python layer, with the checker standing in for the GPU ---------------------------------------------------------------
def test_duplicate_pairs_and_groups_through_the_stub_engine():
    from imageclust_amd import clustering as CL

    E = PC.random_rows(40, 12, 9)
    for c in (7, 21, 22, 23, 24, 25, 26, 27, 28, 29, 31, 32):   # 13 copies of one image: more partners than any k of the old route
        E[c] = E[3]
    E[30] = E[12] + np.float32(1e-3)
    ids = ["img_%d" % i for i in range(40)]
    V = PC.oracle_matrix(E)
    thr = float(V[30, 12]) * 1.5
    seen = []

    def engine(rows, threshold):
        seen.append((rows.shape, rows.dtype, threshold))
        return PC.expected(rows, threshold)

    got = CL.DuplicatePairs(E, ids, thr, engine=engine)
    want = [(ids[a], ids[b], float(V[b, a])) for a in range(40) for b in range(a + 1, 40) if V[b, a] <= thr]
    assert got == want and len(got) == 13 * 12 // 2 + 1 and seen == [((40, 12), np.float32, thr)]
    assert CL.DuplicateGroups(E, ids, thr, engine=engine) == [
        ["img_%d" % i for i in (3, 7, 21, 22, 23, 24, 25, 26, 27, 28, 29, 31, 32)], ["img_12", "img_30"]]
    assert CL.DuplicatePairs(E, ids, -1.0, engine=engine) == [] and CL.DuplicateGroups(E, ids, -1.0, engine=engine) == []
    assert CL.DuplicatePairs(np.zeros((0, 12), np.float32), [], 1.0, engine=engine) == [] and len(seen) == 4
    assert CL.DuplicateGroups(np.zeros((0, 12), np.float32), [], 1.0, engine=engine) == []
    with pytest.raises(ValueError):
        CL.DuplicatePairs(E, ids[:-1], thr, engine=engine)
    # a flat list of floats, as the Go side passes it
    assert CL.DuplicatePairs(E.reshape(-1).tolist(), ids, thr, engine=engine) == want


def test_near_duplicates_is_unchanged():
    """the existing route through its stub: the same list as before, capped at k -- and DuplicatePairs where it is complete"""
    from imageclust_amd import clustering as CL
    from tests import nearest_cases as NC

    class StubContext:
        def nearest(self, Q, E, k, q_size=None, e_size=None, max_size=0, exclude=None, dev=False):
            return NC.expected(Q, E, k, q_size, e_size, max_size, exclude)

    E = PC.random_rows(40, 12, 9)
    E[7] = E[3]
    E[21] = E[3]
    E[30] = E[12] + np.float32(1e-3)
    ids = ["img_%d" % i for i in range(40)]
    V = NC.oracle_values(E, E)
    thr = float(V[12, 30]) * 1.5
    got = CL.NearDuplicates(E, ids, 5, thr, ctx=StubContext())
    assert got == [(ids[a], ids[b], float(V[a, b])) for a in range(40) for b in range(a + 1, 40) if V[a, b] <= thr]
    assert got == CL.DuplicatePairs(E, ids, thr, engine=lambda rows, t: PC.expected(rows, t))
    assert [g[:2] for g in CL.NearDuplicates(E, ids, 1, 0.0, ctx=StubContext())] == [("img_3", "img_7"), ("img_3", "img_21")]
    assert "DuplicatePairs" in CL.NearDuplicates.__doc__


def test_readme_states_the_header_s_symbol_count():
    """README's figure is the number of icl_* declarations tests/test_abi.py counts in include/imageclust.h, and the five new ones are among them"""
    import os
    import re

    from imageclust_amd import _lib
    from tests.test_abi import ROOT, declared_symbols

    names = declared_symbols()
    stated = re.findall(r"(\d+) symbols in `include/imageclust\.h`", open(os.path.join(ROOT, "README.md")).read())
    assert stated == [str(len(names))] and len(names) == len(_lib.SYMBOLS)
    assert {"icl_pairs_within", "icl_pairs_within_dev", "icl_pairs_within_from_matrix", "icl_pair_groups", "icl_last_pairs_stats"} <= set(names)
