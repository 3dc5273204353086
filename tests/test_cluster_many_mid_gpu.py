"""The mid-size route of icl_cluster_many (ward_many.hip: problems of 257 to 2048 rows, one workgroup each, run in groups under a
workspace budget; icl_set_many_options).  Bar: that of test_cluster_many_gpu.py -- every problem's cluster ids, member ranks,
cluster count, status and merge log equal oracle.cluster_fast's, BIT-EXACT, and icl_cluster's on the problem alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ward_cases as WC
from tests.many_cases import oracles, same_as_cluster, same_as_oracle, same_reports, same_results, serving_problems, ward_reports

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture()
def mid_on(ctx):
    from imageclust_amd import _lib

    ctx.set_many_options(_lib.MANY_MID_ON)
    yield ctx
    ctx.set_many_options(_lib.MANY_MID_AUTO)


def test_reference_shape_200_mid_problems(mid_on):
    ctx = mid_on
    probs = serving_problems(200, 20261017, n_lo=257, n_hi=2048, dup_every=25)
    assert {pr[0].shape[1] % 2 for pr in probs} == {0, 1}
    res = ctx.cluster_many(probs, want_merges=True)
    stats = ctx.last_many_stats()
    assert stats["mid"] == 200 and stats["small"] == 0 and stats["large"] == 0 and stats["mid_groups"] >= 1, stats
    for p, (pr, r, ref) in enumerate(zip(probs, res, oracles(probs))):
        what = "problem %d (n %d, d %d)" % (p, pr[0].shape[0], pr[0].shape[1])
        same_as_oracle(r, ref, what)
        same_as_cluster(ctx, pr, r, what)


def adversarial():
    E_nan = WC.mog(400, 6, 3)
    E_nan[7, 2] = np.nan
    E_nan[11, 0] = np.inf
    E_nan[300, 5] = -np.inf
    E_nan[399, 1] = np.nan
    out = [("ties300", WC.ties(300, 8, 1), 3, 6), ("ties777", WC.ties(777, 8, 2), 2, 9), ("ties2048", WC.ties(2048, 8, 3), 3, 6),
           ("ties777_big", WC.ties(777, 8, 4), 1, 777),
           ("mog_40_300", WC.mog(2048, 24, 5), 40, 300), ("mog_1_2048", WC.mog(2048, 16, 6), 1, 2048), ("mog1000_40_300", WC.mog(1000, 33, 7), 40, 300),
           ("no_pairs_left", WC.mog(300, 3, 1), 5, 5),  # 231 merges of the 240 asked for: "No more clusters to merge"
           ("good_a", WC.mog(500, 12, 8), 3, 6), ("cannot_be_met", WC.mog(302, 9, 9), 4, 4), ("good_b", WC.mog(640, 10, 10), 2, 5),
           ("nan_inf", E_nan, 1, 3), ("nan_inf_3_6", E_nan, 3, 6),
           ("d1", WC.mog(900, 1, 11), 3, 6), ("d3", WC.mog(513, 3, 12), 3, 6), ("d4", WC.mog(1025, 4, 13), 3, 6),
           ("d2052", WC.mog(600, 2052, 14), 3, 6), ("d2051", WC.mog(300, 2051, 15), 3, 6),
           ("n257", WC.mog(257, 1003, 16), 3, 6), ("n2048", WC.mog(2048, 1100, 17), 3, 6), ("n2049", WC.mog(2049, 16, 18), 3, 6),
           ("identical", np.ones((700, 5), np.float32), 2, 4), ("max1", WC.mog(300, 4, 19), 1, 1)]
    return out


def test_adversarial_inputs_at_mid_size(mid_on):
    from imageclust_amd import _lib

    ctx = mid_on
    cases = adversarial()
    probs = [(E, mn, mx) for _, E, mn, mx in cases]
    res = ctx.cluster_many(probs, want_merges=True)
    stats = ctx.last_many_stats()
    refs = oracles(probs)
    assert not refs[[c[0] for c in cases].index("cannot_be_met")]["ok"]
    assert len(refs[7]["log"]) == 231
    for (name, E, mn, mx), r, ref in zip(cases, res, refs):
        same_as_oracle(r, ref, name)
        same_as_cluster(ctx, (E, mn, mx), r, name)
    # n2049 is above the route; cannot_be_met and max1 (nothing to merge) take no route
    assert stats["large"] == 1 and stats["small"] == 0 and stats["mid"] == len(cases) - 3, stats
    assert [r[3] for r in res].count(_lib.ICL_ERR_CONSTRAINT) == 1


def mixed_batch():
    small = serving_problems(300, 21, n_lo=3, n_hi=256)
    mid = serving_problems(40, 22, n_lo=257, n_hi=2048)
    probs = []
    for i, pr in enumerate(small):
        probs.append(pr)
        if i % 7 == 3 and mid:
            probs.append(mid.pop())
    probs += mid
    probs.insert(123, (WC.mog(3000, 64, 5), 3, 6))
    probs.insert(200, (WC.mog(2, 9, 1), 3, 6))  # cannot be met: no route
    return probs


def test_mixed_batch_auto_and_off(ctx):
    from imageclust_amd import _lib

    probs = mixed_batch()
    assert len(probs) == 342
    ctx.set_many_options(_lib.MANY_MID_AUTO)
    auto = ctx.cluster_many(probs, want_merges=True)
    s = ctx.last_many_stats()
    assert s["small"] == 300 and s["small"] + s["mid"] + s["large"] == 341, s
    for p, (pr, r) in enumerate(zip(probs, auto)):
        same_as_cluster(ctx, pr, r, "problem %d" % p)
    try:
        ctx.set_many_options(_lib.MANY_MID_OFF)
        off = ctx.cluster_many(probs, want_merges=True)
        s = ctx.last_many_stats()
        assert s == {"small": 300, "mid": 0, "large": 41, "mid_groups": 0}, s
        ctx.set_many_options(_lib.MANY_MID_ON)
        on = ctx.cluster_many(probs, want_merges=True)
        s = ctx.last_many_stats()
        assert s["small"] == 300 and s["mid"] == 40 and s["large"] == 1 and s["mid_groups"] >= 1, s
    finally:
        ctx.set_many_options(_lib.MANY_MID_AUTO)
    for p, (a, b, c) in enumerate(zip(auto, off, on)):
        same_results(a, b, p)
        same_results(a, c, p)


def test_result_does_not_depend_on_the_batch(mid_on):
    ctx = mid_on
    probs = serving_problems(24, 23, n_lo=257, n_hi=1400, dup_every=11)
    base = ctx.cluster_many(probs, want_merges=True)
    for pr, r, ref in zip(probs, base, oracles(probs)):
        same_as_oracle(r, ref, "base")
    perm = np.random.default_rng(1).permutation(len(probs))
    shuf = ctx.cluster_many([probs[i] for i in perm], want_merges=True)
    for j, i in enumerate(perm):
        same_results(base[i], shuf[j], i)
    for i in range(0, len(probs), 6):
        alone = ctx.cluster_many([probs[i]], want_merges=True)[0]
        assert ctx.last_many_stats() == {"small": 0, "mid": 1, "large": 0, "mid_groups": 1}
        same_results(base[i], alone, i)
    copies = ctx.cluster_many([probs[3]] * 64, want_merges=True)
    assert ctx.last_many_stats()["mid"] == 64
    for r in copies:
        same_results(base[3], r, "copies")


def test_dev_equals_host_and_last_merges_unchanged(mid_on):
    from imageclust_amd import _lib

    ctx = mid_on
    probs = serving_problems(12, 24, n_lo=257, n_hi=900) + [(WC.mog(700, 12, 9), 3, 6), (WC.mog(37, 3, 1), 2, 4), (WC.mog(90, 8, 2), 2, 4)]
    assert any(pr[0].shape[1] % 4 == 0 for pr in probs)
    host = ctx.cluster_many(probs, want_merges=True)
    assert ctx.last_many_stats()["mid"] == 13
    pk = _lib.pack_many(probs)
    E = np.concatenate([[7.0], pk["E"]]).astype(np.float32)  # every problem one float further: rows the float4 loads cannot read in place
    dE = ctx.malloc(E.nbytes)
    try:
        ctx.h2d(dE, E)
        dev = ctx.cluster_many_dev(dE, E.size, pk["e_off"] + 1, pk["n"], pk["d"], pk["min_size"], pk["max_size"], want_merges=True)
    finally:
        ctx.free(dE)
    assert ctx.last_many_stats()["mid"] == 13
    for p, (a, b, ref) in enumerate(zip(host, dev, oracles(probs))):
        same_results(a, b, p)
        same_as_oracle(a, ref, p)

    E1 = WC.mog(90, 16, 4)
    ctx.cluster(E1, 3, 6)
    before = ward_reports(ctx)
    ctx.cluster_many(probs)
    assert ctx.last_many_stats()["mid"] == 13
    same_reports(ward_reports(ctx), before)


def test_python_api_many_takes_the_route(mid_on):
    from imageclust_amd import clustering

    ctx = mid_on
    probs = serving_problems(3, 25, n_lo=257, n_hi=400)
    jobs = [(E, ["img%d_%d" % (p, i) for i in range(len(E))], mn, mx) for p, (E, mn, mx) in enumerate(probs)]
    many = clustering.PerformClusteringWithConstraintsMany(jobs, ctx=ctx)
    assert ctx.last_many_stats()["mid"] == 3
    for job, got in zip(jobs, many):
        assert got == clustering.PerformClusteringWithConstraints(job[0].tolist(), job[1], job[2], job[3], ctx=ctx)


def test_set_many_options_rejects_unknown_modes(ctx):
    from imageclust_amd import _lib

    with pytest.raises(_lib.ICLError) as ei:
        ctx.set_many_options(3)
    assert ei.value.code == _lib.ICL_ERR_ARG


_CHILD = """
from imageclust_amd import _lib
from tests.many_cases import not_as_oracle, oracles, serving_problems
ctx = _lib.Context(0)
assert ctx.last_many_stats() == {"small": 0, "mid": 0, "large": 0, "mid_groups": 0}
probs = serving_problems(24, 26, n_lo=1500, n_hi=1500)
res = ctx.cluster_many(probs, want_merges=True)   # (ICL_MANY_MID=on: the context's default)
stats = ctx.last_many_stats()
refs = oracles(probs)
bad = not_as_oracle(probs, res, refs) + [p for p, ref in enumerate(refs) if not ref["ok"]]
ctx.close()
print("BAD", bad)
print("STATS", stats["mid"], stats["mid_groups"])
"""


def test_several_groups():
    """24 problems of 1500 rows need 15 to 16 MB of workspace each (centroids + the square matrix); with a budget of 130 MB
    (ICL_MANY_MID_WS_MB, read at start-up: a child process) they run in at least 3 groups, one after the other in the same region."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ICL_MANY_MID_WS_MB="130", ICL_MANY_MID="on")
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "BAD []" in r.stdout, r.stdout[-2000:]
    mid, groups = [int(x) for x in r.stdout.split("STATS")[1].split()[:2]]
    assert mid == 24 and groups >= 3, r.stdout[-2000:]
