"""icl_pairs_between_from_matrix (imageclust_amd/csrc/pairs.hip + pairs_plan.h + pairs_select.h, host only) against the
plain-numpy checker of tests/pairs_between_cases.py; tests/pairs_plan_main.cpp, the same host code of both pairs families with the prefix
and placement arithmetic in a stand-alone program under the address and undefined-behaviour sanitizers; and the Python layer over icl_pairs_between
(DuplicatesOf, Clustering.duplicates_of, Clustering.add(skip_duplicates=), workflow.RunMore(dedupe_threshold=)) through engine stand-ins.
No GPU, no Python in the sanitised process."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import pairs_between_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["rule", "from_matrix sweep", "prefix and placement", "bad arguments", "within rule", "within from_matrix sweep", "within prefix"]
LIMIT_S = 300
INF = np.float32(np.inf)


def from_matrix(V, thr, **kw):
    from imageclust_amd import _lib

    return _lib.pairs_between_from_matrix(V, thr, **kw)


def check(V, thr, exclude=None):
    got, want = from_matrix(V, thr, exclude=exclude), BC.select(V, thr, exclude)
    assert BC.same(got, want), "threshold %r: %s" % (thr, BC.why(got, want))
    return got


def test_thresholds_special_values_and_exclude():
    V = np.array([[0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 2.0],
                  [np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, np.nan],
                  [np.inf, 3.0, -0.0, 0.0, BC.MAXF, 1.0, 1.0]], np.float32)
    rp, col, val = check(V, -0.0)
    assert rp.tolist() == [0, 3, 3, 5] and col.tolist() == [0, 1, 5, 2, 3] and np.signbit(val[1]) and not np.signbit(val[0])
    assert BC.same(check(V, 0.0), (rp, col, val))
    rp, col, val = check(V, INF)
    assert rp.tolist() == [0, 6, 6, 13] and not np.isnan(val).any() and np.isinf(val).sum() == 3
    assert check(V, BC.MAXF)[0].tolist() == [0, 5, 5, 11]
    assert check(V, -INF)[0].tolist() == [0, 1, 1, 1]
    assert check(V, -1.0)[1].tolist() == [5]
    ex = np.array([0, 3, -1], np.int64)
    rp, col, _ = check(V, INF, exclude=ex)
    assert rp.tolist() == [0, 5, 5, 12] and col[:5].tolist() == [1, 2, 4, 5, 6]
    assert check(V, 1.0, exclude=np.array([5, -1, 6], np.int64))[1].tolist() == [0, 1, 2, 2, 3, 5]


def test_random_sweep_and_leading_dimension():
    rng = np.random.default_rng(7)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, 3.5, -1.0, np.inf, -np.inf, np.nan, BC.MAXF], np.float32)
    for _ in range(300):
        nq, n = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        V = pool[rng.integers(0, len(pool), (nq, n))]
        ex = rng.integers(-1, n, nq).astype(np.int64) if n and rng.integers(0, 2) else None
        thr = pool[rng.integers(0, len(pool))]
        check(V, INF if np.isnan(thr) else thr, ex)
    D = rng.integers(0, 4, (6, 50)).astype(np.float32)
    D[:, 33:] = -1.0  # beyond n: must never be listed
    ex = np.array([0, 32, -1, 5, 5, 32], np.int64)
    got, want = from_matrix(D, 1.0, exclude=ex, n=33), BC.select(D[:, :33], 1.0, ex)
    assert BC.same(got, want), BC.why(got, want)


def test_oracle_values_of_planted_copies():
    Q, L, plant = BC.planted(20, 31, 5, 11)
    qs, ls = BC.mixed_sizes(20, 12), BC.mixed_sizes(31, 13)
    V = BC.oracle_values(Q, L, qs, ls)
    mask = np.zeros(V.shape, bool)
    for i, j in plant.items():
        mask[i, j] = True
    assert (V[mask] == 0).all()
    rp, col, val = check(V, BC.between(V, mask))
    assert rp[-1] == len(plant) and [int(col[rp[i]]) for i in plant] == list(plant.values())
    assert BC.tile_stats(V, BC.between(V, mask)) == (1, 1, 2 * 20 * 31) and BC.tile_stats(V, -1.0) == (1, 0, 20 * 31)


def test_capacity_convention_and_the_size_query():
    from imageclust_amd import _lib

    L = _lib.load()
    V = np.zeros((4, 5), np.float32)
    V[2] = 9.0
    wr, wc, wv = BC.select(V, 1.0)
    total = int(wr[-1])
    p = lambda a: None if a is None else a.ctypes.data

    def call(cap, with_buffers=True):
        rp, tot = np.full(5, 77, np.int64), ctypes.c_int64(-5)
        col, val = np.full(total + 8, 77, np.int32), np.full(total + 8, 77.0, np.float32)
        rc = L.icl_pairs_between_from_matrix(p(V), 4, 5, 5, 1.0, None, p(rp), p(col) if with_buffers else None, p(val) if with_buffers else None, cap,
                                             ctypes.byref(tot))
        return rc, rp, col, val, tot.value

    rc, rp, col, val, tot = call(0, with_buffers=False)
    assert rc == _lib.ICL_OK and tot == total == 15 and np.array_equal(rp, wr)
    rc, rp, col, val, tot = call(total - 1)
    assert rc == _lib.ICL_ERR_ARG and tot == total and np.array_equal(rp, wr) and (col == 77).all() and (val == 77.0).all()
    rc, rp, col, val, tot = call(total)
    assert rc == _lib.ICL_OK and BC.same((rp, col[:total], val[:total]), (wr, wc, wv)) and (col[total:] == 77).all() and (val[total:] == 77.0).all()


def test_bad_arguments_write_nothing():
    from imageclust_amd import _lib

    L = _lib.load()
    nq, n = 3, 5
    D = np.zeros((nq, n), np.float32)
    rp, col, val, tot = np.full(nq + 1, 77, np.int64), np.full(32, 77, np.int32), np.full(32, 77.0, np.float32), ctypes.c_int64(-5)
    ok_ex, hi, lo = np.array([-1, 0, 4], np.int64), np.array([-1, 5, 0], np.int64), np.array([-2, 0, 0], np.int64)
    p = lambda a: None if a is None else a.ctypes.data

    def call(D=D, nq=nq, n=n, ld=n, thr=1.0, ex=ok_ex, rp=rp, col=col, val=val, cap=32, tot=tot):
        return L.icl_pairs_between_from_matrix(p(D), nq, n, ld, thr, p(ex), p(rp), p(col), p(val), cap, None if tot is None else ctypes.byref(tot))

    cases = dict(null_D=dict(D=None), null_row_ptr=dict(rp=None), null_total=dict(tot=None), null_col=dict(col=None), null_val=dict(val=None),
                 null_both_with_cap=dict(col=None, val=None, cap=1), neg_nq=dict(nq=-1), neg_n=dict(n=-1), huge_n=dict(n=1 << 31, ld=1 << 31, ex=None),
                 short_ld=dict(ld=n - 1), exclude_n=dict(ex=hi), exclude_below=dict(ex=lo), nan_threshold=dict(thr=float("nan")), neg_cap=dict(cap=-1))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ICL_ERR_ARG, name
        assert (rp == 77).all() and (col == 77).all() and (val == 77.0).all() and tot.value == -5, name
    assert call() == _lib.ICL_OK and tot.value == 13 and rp.tolist() == [0, 5, 9, 13] and col[5:9].tolist() == [1, 2, 3, 4] and (col[13:] == 77).all()
    for kw, rows in ((dict(D=None, nq=0, ex=None), 0), (dict(D=None, n=0, ld=0, ex=np.full(3, -1, np.int64)), 3)):   # an empty side: ICL_OK, no pairs
        rp[:], tot.value = 77, -5
        assert call(**kw) == _lib.ICL_OK and tot.value == 0 and (rp[:rows + 1] == 0).all() and (rp[rows + 1:] == 77).all()
    with pytest.raises(_lib.ICLError) as ei:
        _lib.pairs_between_from_matrix(D, float("nan"))
    assert ei.value.code == _lib.ICL_ERR_ARG


# ---- the Python layer, with the checker standing in for the GPU ---------------------------------------------------------------
def between_engine(seen=None):
    def engine(Q, L, thr):
        if seen is not None:
            seen.append((len(Q), len(L)))
        return BC.expected(Q, L, thr)
    return engine


def pairs_engine(E, thr):
    from tests import pairs_cases as PC

    return PC.expected(E, thr)


def chain_rows():
    """held h0, h1; then a ~ b ~ c with a not ~ c (points on a line, 0.6 apart: the singleton value is half the squared distance),
    h1x an exact copy of h1, and e, a new image beside nobody"""
    held = np.array([[10.0, 0.0], [20.0, 0.0]], np.float32)
    batch = np.array([[0.0, 0.0], [0.6, 0.0], [1.2, 0.0], [20.0, 0.0], [40.0, 0.0]], np.float32)
    return held, ["h0", "h1"], batch, ["a", "b", "c", "h1x", "e"]


THR = 0.25   # 0.6^2 / 2 = 0.18 is under it, 1.2^2 / 2 = 0.72 is not


def test_duplicates_of_function():
    from imageclust_amd import clustering as CL

    held, hid, batch, bid = chain_rows()
    lib = np.concatenate([held, batch[:3]])
    lid = hid + ["a0", "b0", "c0"]
    got = CL.DuplicatesOf(batch, bid, lib, lid, THR, engine=between_engine())
    V = BC.oracle_values(batch, lib)
    assert [(x, y) for x, y, _ in got] == [("a", "a0"), ("a", "b0"), ("b", "a0"), ("b", "b0"), ("b", "c0"), ("c", "b0"), ("c", "c0"), ("h1x", "h1")]
    assert all(np.float32(v).view(np.uint32) == V[bid.index(x), lid.index(y)].view(np.uint32) for x, y, v in got)
    assert CL.DuplicatesOf(batch[:0], [], lib, lid, THR, engine=between_engine()) == []
    assert CL.DuplicatesOf(batch, bid, lib[:0], [], THR, engine=between_engine()) == []
    with pytest.raises(ValueError):
        CL.DuplicatesOf(batch, bid[:-1], lib, lid, THR, engine=between_engine())


def new_state(seen=None):
    from imageclust_amd import clustering as CL

    held, hid, batch, bid = chain_rows()
    st = CL.Clustering(1, 9, between_engine=between_engine(seen), pairs_engine=pairs_engine)
    assert st.add(held, hid) is None   # None: today's behaviour and today's return
    return st, batch, bid


def test_clustering_duplicates_of_and_the_chain():
    seen = []
    st, batch, bid = new_state(seen)
    before = (list(st.embeddings), len(st.clusters))
    out = st.duplicates_of(batch, bid, THR)
    assert [[k for k, _ in row] for row in out] == [[], ["a"], ["b"], ["h1"], []]   # a ~ b ~ c, a not ~ c; the held partner of the copy
    assert out[3][0][1] == 0.0 and abs(out[1][0][1] - 0.18) < 1e-6 and seen == [(5, 2)]
    assert (list(st.embeddings), len(st.clusters)) == before
    assert st.duplicates_of(batch[:0], [], THR) == []


def test_add_skip_duplicates_names_the_partner():
    from imageclust_amd import clustering as CL

    st, batch, bid = new_state()
    skipped = st.add(batch, bid, skip_duplicates=THR)
    # b duplicates a; c duplicates b, which was itself skipped: c is skipped too, and the partner named is b, its earliest batch partner
    assert [(s, p) for s, p, _ in skipped] == [("b", "a"), ("c", "b"), ("h1x", "h1")]
    assert list(st.embeddings) == ["h0", "h1", "a", "e"] and [c.Members for c in st.clusters] == [["h0"], ["h1"], ["a"], ["e"]]
    # a held partner is named before a batch partner, and the held partner added first before the others
    st2 = CL.Clustering(1, 9, between_engine=between_engine(), pairs_engine=pairs_engine)
    st2.add(np.array([[5.0, 0.0], [0.0, 0.0], [0.1, 0.0]], np.float32), ["far", "first", "second"])
    sk = st2.add(np.array([[0.05, 0.0], [0.06, 0.0]], np.float32), ["x", "y"], skip_duplicates=THR)
    assert [(s, p) for s, p, _ in sk] == [("x", "first"), ("y", "first")]
    V = BC.oracle_values(np.array([[0.05, 0.0]], np.float32), np.array([[0.0, 0.0]], np.float32))
    assert np.float32(sk[0][2]).view(np.uint32) == V[0, 0].view(np.uint32)
    # an empty state compares the batch with itself alone; nothing held, nothing skipped but the batch's own copies
    st3 = CL.Clustering(1, 9, between_engine=between_engine(), pairs_engine=pairs_engine)
    assert [(s, p) for s, p, _ in st3.add(batch, bid, skip_duplicates=THR)] == [("b", "a"), ("c", "b")] and len(st3.clusters) == 3
    assert st3.add(batch[:0], [], skip_duplicates=THR) == []


def test_add_with_an_id_that_is_already_clustered():
    st, batch, bid = new_state()
    for kw in (dict(), dict(skip_duplicates=THR)):
        with pytest.raises(ValueError, match="already clustered"):
            st.add(batch[:1], ["h1"], **kw)
    with pytest.raises(ValueError):
        st.add(batch[:2], ["z", "z"], skip_duplicates=THR)
    assert list(st.embeddings) == ["h0", "h1"] and len(st.clusters) == 2   # a refused batch changes nothing


def test_add_without_a_threshold_is_as_it_was():
    from imageclust_amd import clustering as CL

    def boom(*a):
        raise AssertionError("no comparison is made without a threshold")

    held, hid, batch, bid = chain_rows()
    st = CL.Clustering(1, 9, between_engine=boom, pairs_engine=boom)
    assert st.add(held, hid) is None and st.add(batch, bid, None) is None
    assert list(st.embeddings) == hid + bid and [c.Members for c in st.clusters] == [[k] for k in hid + bid]
    assert all(np.array_equal(c.Centroid, r) for c, r in zip(st.clusters, np.concatenate([held, batch])))


def test_run_more_dedupe_threshold():
    from imageclust_amd import _lib, clustering as CL, workflow as WF

    held, hid, batch, bid = chain_rows()

    def seeded(C, sizes, minSize, maxSize, k_target, *more):   # a loop that merges nothing: every seed stays a cluster of its own
        m = len(C)
        return np.arange(m, dtype=np.int32), np.zeros(m, np.int32), m, _lib.ICL_OK, np.zeros((0, 2), np.int32), np.asarray(C, np.float32)

    class Net:
        ctx = types.SimpleNamespace(embed_files=lambda paths, head, prec, threads: (batch[:, :1].copy(), np.zeros(len(paths), np.int32)))

        def Empty(self):
            return False

    app = types.SimpleNamespace(Net=Net(), Head=0)
    new = (["%s.jpg" % k for k in bid], bid, [["x"]] * 5, {"x": 0, "y": 1})   # every image carries label x: the combined rows differ in column 0 alone

    def state():
        st = CL.Clustering(1, 9, engine=seeded, between_engine=between_engine(), pairs_engine=pairs_engine)
        st.add(np.concatenate([held[:, :1], np.array([[1.0, 0.0]] * 2, np.float32)], axis=1), hid)
        return st

    st = state()
    out = WF.RunMore(app, st, new)
    assert len(out) == 2 and out[1] is True and sorted(sum(out[0].values(), [])) == sorted(hid + bid)
    st = state()
    m, ok, skipped = WF.RunMore(app, st, new, dedupe_threshold=THR)
    assert ok and [(s, p) for s, p, _ in skipped] == [("b", "a"), ("c", "b"), ("h1x", "h1")]
    assert sorted(sum(m.values(), [])) == sorted(hid + ["a", "e"])


# ---- the same host code under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("pairs_plan") / "pairs_plan")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "pairs_plan_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_host_form_prefix_and_placement_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
