"""What the tests of icl_cluster_seeded share (test_cluster_seeded_large_cpu.py, test_cluster_seeded_large_gpu.py): the case lists of the
seeded call on the large-N engine (ward.hip, DESIGN.md "Seeded clustering": the large-N route) and the comparisons.  Checker, states and
problem generators are tests/seeded_cases.py's."""
import numpy as np

from tests import seeded_cases as SC
from tests import ward_cases as WC

# the smallest shapes that cross a seam of the engine: one 64-slot block (64 / 65), the 128-row distance tile (129), a log of at least
# 2 x 64 merges (300: the captured graph replays), d % 4 != 0 (3, 1037) and d above one k-chunk
SHAPES_M = (0, 1, 2, 3, 17, 64, 65, 129, 300)
SHAPES_D = (3, 8, 1037)
GRAPH_MERGES = 128  # 2 * GRAPH_STEPS of ward.hip: from this many merges asked for, the steps are replayed from a captured graph


def large(ctx, job, **kw):
    """One problem (C, seed_size, min, max[, k_target]) through Context.cluster_seeded -> (cid, rank, nc, status, log, C_out)"""
    return ctx.cluster_seeded(job[0], job[1], job[2], job[3], job[4] if len(job) > 4 else 0, **kw)


def many(ctx, job, **kw):
    """The same problem through icl_cluster_many_seeded (at most 2 048 seeds), the same tuple"""
    return ctx.cluster_many_seeded([job], want_merges=True, want_centroids=True, **kw)[0]


def shape_jobs(m, d):
    """Mixed sizes, frozen seeds, a seed of max_size and duplicated centroids with the default k; the same with exact ties and a k_target
    that asks for more merges than the sizes allow (the loop ends for want of pairs)"""
    C1, s1, mn, mx = SC.mixed_problem(m, d, 100 + m + d)
    C2, s2, _, _ = SC.mixed_problem(m, d, 200 + m + d, ties=True)
    return [(C1, s1, mn, mx, 0), (C2, s2, mn, mx, max(1, m // 8))]


def same_tuple(a, b, what):
    """two results of large() / many(): everything equal, C_out as bits"""
    assert a[3] == b[3], (what, a[3], b[3])
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y), what
    assert np.array_equal(a[4], b[4]), what
    assert SC.same_bits(a[5], b[5]), what


def restart_problem():
    """n = 4 200 rows, d = 8, min 3 / max 6: k = 1 050, 3 150 merges from singletons"""
    return WC.mog(4200, 8, 20261019), 3, 6


def fake_pair_log(m, T):
    """A valid log of T merges over m seeds, without a GPU: merge t joins the seeds 2t + 1 and 2t"""
    assert 2 * T <= m
    return np.array([(2 * t + 1, 2 * t) for t in range(T)], np.int32).reshape(-1, 2)
