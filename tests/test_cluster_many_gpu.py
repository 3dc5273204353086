"""icl_cluster_many (imageclust_amd/csrc/ward_many.hip): many independent exact-mode clustering problems in one call.  Bar: every
problem's cluster ids, member ranks, cluster count, status and merge log equal the CPU oracle's and icl_cluster's on that problem
alone, BIT-EXACT, whichever route (one workgroup per problem, or the large-N engine above the cap) the problem took."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import ward_cases as WC
from tests.many_cases import oracles, same_as_cluster, same_as_oracle, same_reports, same_results, serving_problems, ward_reports

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def test_every_small_case_in_one_call(ctx):
    cases = WC.small_cases()
    res = ctx.cluster_many([(E, mn, mx) for _, E, mn, mx in cases], want_merges=True)
    assert len(res) == len(cases)
    for (name, E, mn, mx), r in zip(cases, res):
        same_as_oracle(r, O.cluster(E, mn, mx, want_log=True), name)
        same_as_cluster(ctx, (E, mn, mx), r, name)


def test_reference_shape_2000_problems(ctx):
    probs = serving_problems(2000, 20261016, dup_every=50)
    res = ctx.cluster_many(probs, want_merges=True)
    for p, (pr, r, ref) in enumerate(zip(probs, res, oracles(probs))):
        same_as_oracle(r, ref, "problem %d (n %d, d %d)" % (p, pr[0].shape[0], pr[0].shape[1]))


def test_result_does_not_depend_on_the_batch(ctx):
    probs = serving_problems(40, 7, dup_every=13)
    base = ctx.cluster_many(probs, want_merges=True)
    perm = np.random.default_rng(1).permutation(len(probs))
    shuf = ctx.cluster_many([probs[i] for i in perm], want_merges=True)
    for j, i in enumerate(perm):
        same_results(base[i], shuf[j], i)
    for i in range(0, len(probs), 5):
        alone = ctx.cluster_many([probs[i]], want_merges=True)[0]
        same_results(base[i], alone, i)
    copies = ctx.cluster_many([probs[3]] * 1000, want_merges=True)
    for r in copies:
        same_results(base[3], r, "copies")


def test_failed_problems_and_bad_arguments(ctx):
    from imageclust_amd import _lib

    rng = np.random.default_rng(3)
    good = lambda n: (WC.mog(n, 9, n), 2, 5)
    probs = [good(30), (WC.mog(2, 9, 1), 3, 6), good(1), (np.zeros((0, 9), np.float32), 1, 1), (WC.mog(7, 9, 2), 4, 5),
             (rng.standard_normal((1, 4)).astype(np.float32), 1, 1), good(64), (WC.mog(10, 3, 4), 0, 5), good(17)]
    res = ctx.cluster_many(probs, want_merges=True)
    for p, (pr, r) in enumerate(zip(probs, res)):
        same_as_oracle(r, O.cluster(pr[0], pr[1], pr[2], want_log=True), "problem %d" % p)
    assert [r[3] for r in res] == [0, 2, 2, 2, 2, 0, 0, 2, 0]
    with pytest.raises(_lib.ICLError) as ei:
        ctx.cluster_many(probs, raise_on_error=True)
    assert ei.value.code == _lib.ICL_ERR_CONSTRAINT and "problem 1:" in str(ei.value)

    # argument errors: ICL_ERR_ARG, nothing written
    pk = _lib.pack_many(probs[:1] + probs[6:7])
    L, h = ctx.L, ctx.h

    def call(nprob=2, E=None, e_len=None, e_off=None, n=None, d=None, cid=True):
        outs = [np.full(200, 777, np.int32) for _ in range(6)]
        arr = lambda a: a.ctypes.data
        rc = L.icl_cluster_many(h, nprob, arr(pk["E"]) if E is None else E, pk["E"].size if e_len is None else e_len,
                                arr(pk["e_off"] if e_off is None else e_off), arr(pk["n"] if n is None else n), arr(pk["d"] if d is None else d),
                                arr(pk["min_size"]), arr(pk["max_size"]), arr(outs[0]) if cid else None, arr(outs[1]), arr(outs[2]),
                                arr(outs[3]), arr(outs[4]), arr(outs[5]))
        return rc, all((o == 777).all() for o in outs)

    assert call() == (0, False)  # the well-formed call writes
    assert call(nprob=-1) == (_lib.ICL_ERR_ARG, True)
    assert call(E=C.c_void_p(0)) == (_lib.ICL_ERR_ARG, True)
    assert call(cid=False) == (_lib.ICL_ERR_ARG, True)
    assert call(e_len=pk["E"].size - 1) == (_lib.ICL_ERR_ARG, True)
    assert call(e_off=np.array([0, -4], np.int64)) == (_lib.ICL_ERR_ARG, True)
    assert call(n=np.array([30, -1], np.int32)) == (_lib.ICL_ERR_ARG, True)
    assert call(d=np.array([9, -9], np.int32)) == (_lib.ICL_ERR_ARG, True)
    assert call(e_len=-1) == (_lib.ICL_ERR_ARG, True)
    assert L.icl_cluster_many(h, 0, None, 0, None, None, None, None, None, None, None, None, None, None, None) == 0


def test_mixed_routes(ctx):
    big = WC.mog(3000, 2048, 5)
    probs = serving_problems(500, 11, n_lo=3, n_hi=300)
    probs.insert(123, (big, 3, 6))
    res = ctx.cluster_many(probs, want_merges=True)
    for p, (pr, r) in enumerate(zip(probs, res)):
        assert r[3] == 0, p
        same_as_cluster(ctx, pr, r, p)


def test_dev_equals_host_and_last_merges_unchanged(ctx):
    from imageclust_amd import _lib

    probs = serving_problems(60, 13) + [(WC.mog(700, 12, 9), 3, 6)]  # (the last one above the cap: the large-N route)
    probs += [(WC.mog(37, 3, 1), 2, 4)]
    host = ctx.cluster_many(probs, want_merges=True)
    pk = _lib.pack_many(probs)
    E = np.concatenate([[7.0], pk["E"]]).astype(np.float32)  # every problem one float further: rows the float4 loads cannot read in place
    dE = ctx.malloc(E.nbytes)
    try:
        ctx.h2d(dE, E)
        dev = ctx.cluster_many_dev(dE, E.size, pk["e_off"] + 1, pk["n"], pk["d"], pk["min_size"], pk["max_size"], want_merges=True)
    finally:
        ctx.free(dE)
    for p, (a, b) in enumerate(zip(host, dev)):
        same_results(a, b, p)

    E1 = WC.mog(90, 16, 4)
    ctx.cluster(E1, 3, 6)
    before = ward_reports(ctx)
    ctx.cluster_many(probs)
    same_reports(ward_reports(ctx), before)


def test_python_api_many_equals_single(ctx):
    from imageclust_amd import clustering

    probs = serving_problems(30, 17) + [(WC.mog(2, 8, 1), 3, 6), (WC.mog(25, 8, 2), 5, 5)]
    jobs = [(E, ["img%d_%d" % (p, i) for i in range(len(E))], mn, mx) for p, (E, mn, mx) in enumerate(probs)]
    many = clustering.PerformClusteringWithConstraintsMany(jobs, ctx=ctx)
    assert len(many) == len(jobs)
    for job, got in zip(jobs, many):
        one = clustering.PerformClusteringWithConstraints(job[0].tolist(), job[1], job[2], job[3], ctx=ctx)
        assert got == one


_CHILD = """
from imageclust_amd import _lib
from oracle import oracle as O
from tests import ward_cases as WC
from tests.many_cases import not_as_oracle
ctx = _lib.Context(0)
cases = WC.small_cases()
probs = [(E, mn, mx) for _, E, mn, mx in cases]
res = ctx.cluster_many(probs, want_merges=True)
bad = not_as_oracle(probs, res, [O.cluster(E, mn, mx, want_log=True) for E, mn, mx in probs], [c[0] for c in cases])
ctx.close()
print("BAD", bad)
"""


def test_triangle_in_global_memory():
    """With the cap raised to 1024 (ICL_MANY_CAP, read at start-up: a child process), the small cases of up to 600 rows take the
    one-workgroup route with their triangle in global memory (it fits in LDS up to 281 rows)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ICL_MANY_CAP="1024")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "BAD []" in r.stdout, r.stdout[-2000:]
