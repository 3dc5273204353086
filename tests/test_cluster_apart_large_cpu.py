"""icl_cluster_apart without a GPU (DESIGN.md "Constrained seeded clustering, large N"): the cap-free checker of
tests/apart_large_cases.py pinned to tests/apart_cases.run, and where imageclust_amd.clustering sends a seeded problem."""
import numpy as np
import pytest

from tests import apart_cases as AC
from tests import apart_large_cases as AL
from tests import seeded_cases as SC


@pytest.mark.parametrize("d", AC.CASES_D)
def test_the_checker_is_apart_cases_run(d):
    """constrained and anchored problems on the case list of apart_cases, with and without inheritance"""
    merged = 0
    for m in AC.CASES_M:
        for job in (AC.constrained(m, d), AC.anchored(m, d)):
            ref = AC.run(*job)
            got = AL.run(*job)
            assert AL.same_run(got, ref), (m, d)
            assert len(got["values"]) == len(ref["log"]) and (got["values"] < SC.MAXF).all()
            merged += len(ref["log"])
        job = AC.constrained(m, d)
        assert AL.same_run(AL.run(*job, inherit=False), AC.run(*job, inherit=False)), (m, d)
    assert merged > 200


def test_known_answer_and_small_problems():
    r = AL.run(*AC.KNOWN)
    assert AL.same_run(r, AC.run(*AC.KNOWN)) and np.array_equal(r["log"], AC.KNOWN_LOG)
    assert AL.run(*AC.KNOWN, inherit=False)["log"].tolist() == [[1, 0], [4, 2], [5, 3]]
    # the first value is d(0, 1) = 1/2 * 1, the second d(2, 3) = 1/2 * 7.9^2 in fp32
    assert r["values"][0] == np.float32(0.5) and abs(float(r["values"][1]) - 31.205) < 1e-3
    for m in (0, 1, 2, 3):
        C, ss, mn, mx = SC.mixed_problem(m, 3, 100 + m)
        for kt in (0, 1):
            assert AL.same_run(AL.run(C, ss, mn, mx, kt, None, None), AC.run(C, ss, mn, mx, kt, None, None)), (m, kt)
    # refusals: the statuses of apart_cases.run, and no refusal for the number of seeds
    C, ss, mn, mx = SC.mixed_problem(17, 3, 5, frozen_every=0)
    big = ss.copy()
    big[0] = mx + 1
    assert AL.run(C, big, mn, mx)["status"] == AC.ERR_UNSUPPORTED == AC.run(C, big, mn, mx)["status"]
    assert AL.run(C[:2], np.ones(2, np.int32), 3, 6)["status"] == AC.ERR_CONSTRAINT
    m = SC.MAX_SEEDS + 1
    r = AL.run(np.arange(m, dtype=np.float32).reshape(m, 1), np.ones(m, np.int32), 1, 2, m - 2, None, np.array([[0, 1]], np.int32))
    assert r["status"] == AC.OK and r["log"].tolist() == [[2, 1], [4, 3]]   # (0, 1) may not merge: (1, 2) is the first pair at 0.5


class RecordingContext:
    """stands in for _lib.Context: records which call a seeded problem took"""

    def __init__(self):
        self.calls = []

    def _answer(self, name, m, d):
        self.calls.append(name)
        return np.zeros(m, np.int32), np.zeros(m, np.int32), 1, 0, np.zeros((0, 2), np.int32), np.zeros((m, d), np.float32)

    def cluster_apart(self, C, ss, mn, mx, kt, apart_class=None, apart_pairs=None, want_centroids=True):
        assert apart_class is not None or apart_pairs is not None
        return self._answer("cluster_apart", *np.shape(C))

    def cluster_seeded(self, C, ss, mn, mx, kt, want_centroids=True):
        return self._answer("cluster_seeded", *np.shape(C))

    def cluster_many_apart(self, problems, want_merges=False, want_centroids=False):
        return [self._answer("cluster_many_apart", *np.shape(problems[0][0]))]

    def cluster_many_seeded(self, problems, want_merges=False, want_centroids=False):
        return [self._answer("cluster_many_seeded", *np.shape(problems[0][0]))]


def test_where_a_seeded_problem_goes():
    """constrained: icl_cluster_many_apart up to 2 048 seeds, icl_cluster_apart above; unconstrained: the calls of before, whatever the
    constraint arguments look like when they hold nothing"""
    from imageclust_amd import clustering as CL

    cap = CL.MANY_SEEDED_MAX
    assert cap == SC.MAX_SEEDS
    ctx = RecordingContext()
    prob = lambda m: (ctx, np.zeros((m, 1), np.float32), np.ones(m, np.int32), 1, 4, 0)
    pairs, cls = np.array([[0, 1]], np.int32), np.array([1, 1] + [0] * (cap - 1), np.int32)
    CL._seeded_call(*prob(cap + 1), None, pairs)
    CL._seeded_call(*prob(cap + 1), cls, None)
    CL._seeded_call(*prob(cap), None, pairs)
    CL._seeded_call(*prob(cap), cls[:cap], None)
    assert ctx.calls == ["cluster_apart", "cluster_apart", "cluster_many_apart", "cluster_many_apart"]
    del ctx.calls[:]
    for extra in ((), (None, None), (np.zeros(cap + 1, np.int32), np.zeros((0, 2), np.int32))):
        CL._seeded_call(*prob(cap + 1), *extra)
        CL._seeded_call(*prob(cap), *tuple(e[:cap] if e is not None and e.ndim == 1 else e for e in extra))
    assert ctx.calls == ["cluster_seeded", "cluster_many_seeded"] * 3
    (cid, rank, nc, mg, co), ok = CL.PerformClusteringSeeded(np.zeros((cap + 1, 1), np.float32), np.ones(cap + 1, np.int32), 1, 4, ctx=ctx, apart_pairs=[(0, 1)])
    assert ok and ctx.calls[-1] == "cluster_apart" and len(cid) == cap + 1
    # a handle without the large-N constrained call keeps the refusal (tests/test_cluster_apart_cpu.py holds it for a bare object)
    from imageclust_amd import _lib

    class NoLargeCall(RecordingContext):
        cluster_apart = None

    with pytest.raises(_lib.ICLError) as ei:
        CL._seeded_call(NoLargeCall(), *prob(cap + 1)[1:], None, pairs)
    assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
    CL._seeded_call(NoLargeCall(), *prob(cap)[1:], None, pairs)   # ... and at the cap nothing changes for it
