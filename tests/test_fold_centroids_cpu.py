"""icl_fold_centroids without a GPU (DESIGN.md "Editing a held clustering"): the numpy restatement of tests/fold_cases.py against a
literal loop over float32 scalars and against Clustering.keep_together, imageclust_amd/csrc/fold_plan.h in a stand-alone program under
the address and undefined-behaviour sanitizers, and the planted mistakes the case list must tell from the rule."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from imageclust_amd import _lib, clustering
from tests import fold_cases as FC

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["accepted calls", "refusals", "geometry"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def cases():
    """The case list without the 70 000-group case, each with the rule's answer, computed once."""
    return [(name, E, rp, mb, sz, FC.fold(E, rp, mb, sz)) for name, E, rp, mb, sz in FC.cases(big=False)]


def scalar_fold(E, row_ptr, member, size):
    """The rule of the issue, literally: one float32 scalar operation per line."""
    K, d = len(row_ptr) - 1, E.shape[1]
    C, total = np.zeros((K, d), np.float32), np.zeros(K, np.int64)
    with np.errstate(all="ignore"):
        for g in range(K):
            ms = [int(m) for m in member[row_ptr[g]:row_ptr[g + 1]]]
            for t, m in enumerate(ms):
                s = int(size[m]) if size is not None else 1
                if t == 0:
                    C[g], total[g] = E[m], s
                    continue
                fa, fb, fs = np.float32(int(total[g])), np.float32(s), np.float32(int(total[g]) + s)
                for k in range(d):
                    pa = np.float32(fa * C[g, k])
                    pb = np.float32(fb * E[m, k])
                    sm = np.float32(pa + pb)
                    C[g, k] = np.float32(sm / fs)
                total[g] += s
    return C, total


def test_restatement_is_the_scalar_loop(cases):
    ran = 0
    for name, E, rp, mb, sz, want in cases:
        if E.shape[1] > 8 or rp[-1] > 1500:
            continue  # (the scalar loop is slow; the wide cases run the same lines on longer arrays)
        assert FC.why(want, scalar_fold(E, rp, mb, sz)) is None, name
        ran += 1
    assert ran >= 10


def test_known_answer():
    E = np.array([[1.0, -0.0], [2.0, 3.0], [4.0, 0.1]], np.float32)
    C, s = FC.fold(E, [0, 3, 3, 4, 6], [0, 1, 2, 0, 2, 0], np.array([1, 2, 3], np.int32))
    assert s.tolist() == [6, 0, 1, 4]
    c01 = (np.float32(1) * E[0] + np.float32(2) * E[1]) / np.float32(3)
    assert FC.why((C[:1], s[:1]), (((np.float32(3) * c01 + np.float32(3) * E[2]) / np.float32(6))[None], [6])) is None
    assert C[1].view(np.uint32).tolist() == [0, 0]                       # an empty group: +0.0
    assert C[2].view(np.uint32).tolist() == E[0].view(np.uint32).tolist()  # one member: the row's bits, -0.0 included
    assert FC.why((C[3:], s[3:]), (((np.float32(3) * E[2] + np.float32(1) * E[0]) / np.float32(4))[None], [4])) is None  # list order, not row order


def test_restatement_is_keep_together():
    """Clusters merged one at a time by Clustering.keep_together (singletons: the unsized fold; whole clusters: the sized fold over the
    clusters' centroids) hold the restatement's bits."""
    rng = np.random.default_rng(3)
    E = FC.rows(40, 8, rng)
    ids = ["i%d" % i for i in range(40)]
    for order in ([0, 5, 3, 9, 31], [1, 39], [2] + [int(i) for i in 3 + rng.permutation(37)[:16]]):
        st = clustering.Clustering(1, 1000)  # (keep_together merges in held order: the growing cluster holds the lowest position)
        st.add(E, ids)
        for a in order[1:]:
            st.keep_together([ids[order[0]], ids[a]])  # the growing cluster stands first: members join in list order
        got = next(c for c in st.clusters if ids[order[0]] in c.Members)
        assert got.Members == [ids[i] for i in order]
        assert FC.why((got.Centroid[None], [len(order)]), FC.fold(E, [0, len(order)], order)) is None, order
    # sized: clusters of 3, 1, 4 and 2 images merged in held order
    parts = [[0, 1, 2], [3], [4, 5, 6, 7], [8, 9]]
    st = clustering.Clustering(1, 1000)
    st.add(E[:10], ids[:10])
    for p in parts:
        for a in p[1:]:
            st.keep_together([ids[p[0]], ids[a]])
    cen = np.stack([c.Centroid for c in st.clusters])
    assert FC.why((cen, [3, 1, 4, 2]), FC.fold(E, [0, 3, 4, 8, 10], list(range(10)))) is None
    st.keep_together([ids[p[0]] for p in parts])
    assert len(st.clusters) == 1
    assert FC.why((st.clusters[0].Centroid[None], [10]), FC.fold(cen, [0, 4], [0, 1, 2, 3], np.array([3, 1, 4, 2], np.int32))) is None


def test_the_cases_tell_every_planted_mistake(cases):
    """Each wrong arithmetic differs from the rule, as bits, on at least one case.  Of the 21 cases (K = 0 holds nothing to differ on): members in sorted order
    20, the plain mean 19, contracted product and sum 20, weight 1 for a sized row 11 (every sized case), the total converted after the
    next size was added 20, the total added in fp32 1 (the case with sizes around 2^24)."""
    differs = {m: 0 for m in FC.MISTAKES}
    for name, E, rp, mb, sz, want in cases:
        for m in FC.MISTAKES:
            differs[m] += FC.why(FC.fold(E, rp, mb, sz, mistake=m), want) is not None
    print(len(cases), differs)
    assert all(v >= 1 for v in differs.values()), differs
    assert differs["total_in_f32"] >= 1 and differs["weight1"] >= 7, differs


def test_python_layer_lists():
    rp, mb = _lib.groups_as_csr([[3, 1], [], [2]])
    assert rp.dtype == np.int64 and rp.tolist() == [0, 2, 2, 3] and mb.dtype == np.int32 and mb.tolist() == [3, 1, 2]
    assert _lib.groups_as_csr([])[0].tolist() == [0]
    with pytest.raises(ValueError):
        _lib._fold_lists([0, 2], [1])
    assert {"icl_fold_centroids", "icl_fold_centroids_dev", "icl_last_fold_stats"} <= {s[0] for s in _lib.SYMBOLS}
    for name in ("fold_centroids", "fold_centroids_dev", "last_fold_stats"):
        assert callable(getattr(_lib.Context, name))
    assert callable(clustering.FoldCentroids)


# ---- the host code of the entry points under the sanitizers ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("fold_plan") / "fold_plan")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "fold_plan_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_argument_check_and_geometry_under_the_sanitizers(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_the_python_geometry_is_the_headers(program):
    """tests/fold_cases.geometry, by which the GPU tests say how many waves their cases' workgroups hold, against fold_geometry itself:
    every case's shape, aligned and not, on 256 and 304 compute units."""
    shapes = {(len(rp) - 1, E.shape[1]) for _, E, rp, _, _ in FC.cases()} | {(11000, 2048), (1, 2048), (205, 1037), (204, 1037)}
    for K, d in sorted(shapes):
        for aligned in (0, 1):
            for cus in (256, 304):
                r = subprocess.run([program, str(K), str(d), str(aligned), str(cus)], capture_output=True, text=True, timeout=LIMIT_S)
                assert r.returncode == 0, r.stderr[-2000:]
                vec, threads, chunks, grid = (int(x) for x in r.stdout.split())
                assert (bool(vec), threads, chunks) == FC.geometry(K, d, aligned, cus), (K, d, aligned, cus)
                assert grid == K * chunks
    assert {FC.geometry(K, d, True, 256)[1] for _, K, d, _ in FC.WAVES} == {128, 256}
