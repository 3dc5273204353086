"""icl_cluster_fit_from_matrix (imageclust_amd/csrc/fit.hip + fit_select.h, host only) and the Python layer over icl_cluster_fit
(Clustering.fit / representatives / misfits) through engine stand-ins: the leave-out, order and key rules against the plain-numpy
checker of tests/fit_cases.py; tests/fit_select_main.cpp, the same host code in a stand-alone program under the address and
undefined-behaviour sanitizers.  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fit_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["keys and leave-out rule", "case list", "sweep", "bad arguments"]
LIMIT_S = 300


def from_matrix(V, cluster_of, k_alt, **kw):
    from imageclust_amd import _lib

    return _lib.cluster_fit_from_matrix(V, cluster_of, k_alt, **kw)


def check(V, cluster_of, k_alt, q_size=None, c_size=None, max_size=0):
    got = from_matrix(V, cluster_of, k_alt, q_size=q_size, c_size=c_size, max_size=max_size)
    want = FC.from_values(V, cluster_of, k_alt, q_size, c_size, max_size)
    assert not FC.why(got, want), "k_alt=%d: %s" % (k_alt, FC.why(got, want))
    return want


@pytest.mark.parametrize("nq,K,d", FC.CASES + [FC.SPLIT_CASE])
def test_every_case_of_the_gpu_suite(nq, K, d):
    for plain in (False, True):
        P = FC.problem(nq, K, d, 1000 + nq, plain=plain)
        V = FC.values(P["Q"], P["C"], P["q_size"], P["c_size"])
        for k in FC.K_ALTS:
            want = check(V, P["cluster_of"], k, P["q_size"], P["c_size"], P["max_size"])
        if not plain and nq >= 8 and K >= 5:
            assert not FC.covers(P, want), "the case lacks " + FC.covers(P, want)
        check(V, P["cluster_of"], 10)   # NULL sizes: singletons, nothing frozen, nothing banned


def test_random_sweep():
    rng = np.random.default_rng(3)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, 3.5, -1.0, np.inf, -np.inf, np.nan, FC.MAXF], np.float32)
    for _ in range(300):
        nq, K = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        V = pool[rng.integers(0, len(pool), (nq, K))]
        cof = (rng.integers(-1, K, nq) if K else np.full(nq, -1)).astype(np.int32)
        qs = rng.integers(1, 7, nq).astype(np.int32)
        cs = (rng.integers(1, 10, K) * rng.choice([1, 1, 1, -1], K)).astype(np.int32)
        check(V, cof, int(rng.integers(0, 6)), qs, cs, int(rng.choice([0, 6, 9, 13])))


def test_empty_sides_and_leading_dimension():
    r = from_matrix(np.zeros((0, 4), np.float32), np.zeros(0, np.int32), 3)
    assert r["own"].shape == (0,) and (r["listed"] == 0).all() and (r["rep"] == -1).all() and (r["worst"] == -1).all()
    r = from_matrix(np.zeros((3, 0), np.float32), np.full(3, -1, np.int32), 2)
    assert (r["own"] == FC.MAXF).all() and (r["alt_idx"] == -1).all() and (r["alt_val"] == FC.MAXF).all()
    D = np.random.default_rng(4).integers(0, 4, (6, 50)).astype(np.float32)
    D[:, 33:] = -1.0  # beyond K: must never be listed
    cof = np.array([0, 32, -1, 5, 5, 32], np.int32)
    got = from_matrix(D, cof, 7, K=33)
    want = FC.from_values(D[:, :33], cof, 7)
    assert not FC.why(got, want), FC.why(got, want)


def test_the_checker_reports_planted_faults():
    P = FC.problem(40, 9, 6, 5)
    P["cluster_of"][0] = 0
    V = FC.values(P["Q"], P["C"], P["q_size"], P["c_size"])
    V[0, 0] = -1.0   # row 0's own cluster is its nearest column by far: leaving it in must show
    want = check(V, P["cluster_of"], 3, P["q_size"], P["c_size"], P["max_size"])
    assert "alt_idx" in FC.why(FC.plant_own_column(want, P["cluster_of"], V), want)
    tied = FC.plant_highest_index_tie(want, P["cluster_of"])
    assert (tied["rep"] != want["rep"]).any() and "rep" in FC.why(tied, want)   # (rows 6 and 7 tie inside their cluster)
    assert not FC.why(want, want)


def test_bad_arguments_write_nothing():
    from imageclust_amd import _lib

    L = _lib.load()
    nq, K, k = 3, 5, 4
    D = np.zeros((nq, K), np.float32)
    ok_q, ok_c, ok_of = np.ones(nq, np.int32), np.ones(K, np.int32), np.array([0, -1, 4], np.int32)
    outs = [np.full(nq, 77.0, np.float32), np.full((nq, 64), 77, np.int32), np.full((nq, 64), 77.0, np.float32), np.full(K, 77, np.int32),
            np.full(K, 77, np.int32), np.full(K, 77, np.int32)]
    p = lambda a: None if a is None else a.ctypes.data

    def call(D=D, nq=nq, K=K, ld=K, qs=ok_q, cof=ok_of, cs=ok_c, k=k, own=outs[0], ai=outs[1], av=outs[2]):
        return L.icl_cluster_fit_from_matrix(p(D), nq, K, ld, p(qs), p(cof), p(cs), k, 0, p(own), p(ai), p(av), p(outs[3]), p(outs[4]), p(outs[5]))

    bad_q, bad_c, hi, lo = ok_q.copy(), ok_c.copy(), ok_of.copy(), ok_of.copy()
    bad_q[1], bad_c[4], hi[2], lo[0] = 0, 0, K, -2
    cases = dict(null_D=dict(D=None), null_cof=dict(cof=None), null_own=dict(own=None), null_idx=dict(ai=None), null_val=dict(av=None),
                 k_neg=dict(k=-1), k65=dict(k=65), neg_nq=dict(nq=-1), neg_K=dict(K=-1), huge_K=dict(K=1 << 31, ld=1 << 31), short_ld=dict(ld=K - 1),
                 q_size_0=dict(qs=bad_q), c_size_0=dict(cs=bad_c), cof_K=dict(cof=hi), cof_below=dict(cof=lo), no_clusters=dict(K=0, ld=0))
    for name, kw in cases.items():
        assert call(**kw) == _lib.ICL_ERR_ARG, name
        assert all((a == 77).all() for a in outs), name
    assert call(k=0, ai=None, av=None) == _lib.ICL_OK and (outs[1] == 77).all()   # k_alt == 0: no alternative array is needed
    assert call() == _lib.ICL_OK   # rows of k entries, back to back: all values tie, so each row lists its first k columns but its own
    assert outs[1].reshape(-1)[:nq * k].reshape(nq, k).tolist() == [[1, 2, 3, 4], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert (outs[1].reshape(-1)[nq * k:] == 77).all() and outs[3].tolist() == [1, 0, 0, 0, 1]
    with pytest.raises(_lib.ICLError) as ei:
        _lib.cluster_fit_from_matrix(D, ok_of, 65)
    assert ei.value.code == _lib.ICL_ERR_ARG


# ---- the Python layer, with the checker standing in for the GPU ---------------------------------------------------------------
def test_clustering_fit_representatives_and_misfits_through_stand_ins():
    from imageclust_amd import clustering as CL

    d = 6
    rng = np.random.default_rng(10)
    rows = rng.standard_normal((9, d)).astype(np.float32)
    rows[7] = rows[6]                              # two members at one place: the cover is the earlier one
    rows[8] = rows[1] + np.float32(0.01)           # p8 sits in a cluster of its own, right beside p1's
    ids = ["p%d" % i for i in range(9)]
    seen = []

    def engine(Q, cluster_of, C, k_alt, q_size, c_size, max_size):
        seen.append((len(Q), list(map(int, cluster_of)), len(C), k_alt, list(map(int, q_size)), list(map(int, c_size)), max_size))
        return FC.expected(Q, C, cluster_of, k_alt, q_size, c_size, max_size)

    st = CL.Clustering(2, 3, fit_engine=engine)
    st.add(rows, ids)
    H = CL.HeldCluster
    st.clusters = [H(["p4", "p0"], rows[[4, 0]].mean(0)), H(["p1", "p2", "p3"], rows[[1, 2, 3]].mean(0)),  # full: 3 + 1 > maxSize
                   H(["p5"], rows[5].copy(), Frozen=True), H(["p6", "p7"], rows[[6, 7]].mean(0)), H(["p8"], rows[8].copy())]
    before = [(list(c.Members), c.Centroid.copy(), c.Frozen) for c in st.clusters]
    out = st.fit(4)
    order = ["p4", "p0", "p1", "p2", "p3", "p5", "p6", "p7", "p8"]
    cof = [0, 0, 1, 1, 1, 2, 3, 3, 4]
    assert seen == [(9, cof, 5, 4, [1] * 9, [2, 3, -1, 2, 1], 3)] and list(out) == order
    C = np.stack([c.Centroid for c in st.clusters]).astype(np.float32)
    Q = np.stack([rows[int(k[1:])] for k in order])
    V = FC.values(Q, C, np.ones(9, np.int32), np.array([2, 3, 1, 2, 1], np.int32))
    for i, key in enumerate(order):
        own, alts = out[key]
        assert np.float32(own).view(np.uint32) == V[i, cof[i]].view(np.uint32)     # the own cluster is measured, frozen (p5) or full (p1's)
        names = [nm for nm, _ in alts]
        assert "p1" not in names and "p5" not in names and st.clusters[cof[i]].Members[0] not in names
        cand = [c for c in (0, 3, 4) if c != cof[i]]
        assert alts == [(st.clusters[c].Members[0], float(V[i, c])) for c in sorted(cand, key=lambda c: (V[i, c], c))]  # short rows, no filler
    assert out["p8"][0] == 0.0 and out["p5"][0] == 0.0
    assert st.representatives() == {"p4": "p4" if V[0, 0] <= V[1, 0] else "p0", "p1": ["p1", "p2", "p3"][int(np.argmin(V[2:5, 1]))], "p5": "p5",
                                    "p6": "p6", "p8": "p8"}
    assert seen[-1][3] == 0
    gains = {key: own - alts[0][1] for key, (own, alts) in out.items() if alts and alts[0][1] < own}
    assert st.misfits() == sorted(gains, key=lambda k: -gains[k]) and "p8" not in gains
    assert [(list(c.Members), c.Frozen) for c in st.clusters] == [(m, f) for m, _, f in before]
    assert all(np.array_equal(c.Centroid, b[1]) for c, b in zip(st.clusters, before))
    empty = CL.Clustering(2, 3, fit_engine=engine)
    assert empty.fit() == {} and empty.representatives() == {} and empty.misfits() == []


def test_misfits_orders_by_gain():
    from imageclust_amd import clustering as CL

    def engine(Q, cluster_of, C, k_alt, q_size, c_size, max_size):
        own = np.array([5.0, 1.0, 9.0, 2.0, np.nan], np.float32)
        alt = np.array([[3.0], [2.0], [1.0], [2.0], [1.0]], np.float32)  # gains 2, none, 8, none (equal is not below), none (NaN)
        return dict(own=own, alt_idx=np.array([[1], [0], [0], [0], [0]], np.int32), alt_val=alt, listed=None, rep=None, worst=None)

    st = CL.Clustering(1, 9, fit_engine=engine)
    st.add(np.zeros((5, 2), np.float32), list("abcde"))
    assert st.misfits() == ["c", "a"]


# ---- the same host code under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("fit_select") / "fit_select")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "fit_select_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_rules_and_from_matrix_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
