"""dist_bound_i8_kernel's epilogue (distance_i8.hip) at the sizes where its two paths meet: every entry of the initial matrix -- the
flagged lower bound and the upper bound the scans derive from it -- against the exact kernel's value (icl_distance_bounds_check_dev, the
integer GEMM forced), for
  n = 255        one ragged diagonal tile;
  n = 256        one full diagonal tile;
  n = 257, 513   a last tile row of one row: the general path below the diagonal;
  n = 513, 768   full interior tiles (tile (1, 0); (1, 0), (2, 0), (2, 1)): the predicate-free path;
  n = 1000       interior tiles, a ragged last tile row;
each with D = 1, 64, 100 (padded) and 2048, on five inputs aimed at the terms of the bound: standard normal rows, a large common offset
(cancellation), exact duplicates (T = 0), rows of zeros (s = 0) and one huge coordinate (the scale of the fixed-point image).
One clustering case at n = 4096 -- from where ward.hip fills the initial matrix with bounds on its own (ward_rows_use_bound) --, D = 64:
ICL_DIST_BOUND and ICL_DIST_LWBOUND against ICL_DIST_EXACT, which exercises rowub (the thresholds the initial row minima start from)."""
import functools

import numpy as np
import pytest

from tests import ward_cases as WC

pytestmark = pytest.mark.gpu
NS = (255, 256, 257, 513, 768, 1000)
DS = (1, 64, 100, 2048)
INPUTS = ("normal", "offset", "duplicates", "zero_rows", "huge_coordinate")
I8 = 2  # icl_distance_bounds_check_dev: the integer GEMM whatever the shape


@functools.lru_cache(maxsize=4)
def inputs(n, d):
    rng = np.random.default_rng([20250614, n, d])
    g = rng.standard_normal((n, d)).astype(np.float32)
    dup = np.repeat(g[:(n + 7) // 8], 8, axis=0)[:n]
    zero = g.copy()
    zero[rng.random(n) < 0.5] = 0.0
    zero[0] = 0.0
    huge = g.copy()
    huge[:, -1] *= 1e4
    out = {"normal": g, "offset": (g + 100.0).astype(np.float32), "duplicates": np.ascontiguousarray(dup), "zero_rows": zero, "huge_coordinate": huge}
    assert tuple(out) == INPUTS
    return out


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_every_bound_of_both_epilogue_paths(ctx, n, d):
    for name, E in inputs(n, d).items():
        r = ctx.distance_bounds_check(E, I8)
        print("dist_i8 n %4d d %4d %-16s %s" % (n, d, name, r))
        assert r["below"] == 0 and r["above"] == 0 and r["unflagged"] == 0, (name, r)


@pytest.mark.parametrize("kind", [1, 2], ids=["f32_gemm", "i8_gemm"])
@pytest.mark.parametrize("n,d", [(300, 64), (1000, 100)])
def test_the_checker_counts_every_pair(ctx, n, d, kind):
    """The judge of the tests above is itself a GPU kernel: its sum of the exact values over all pairs must be the float64 sum of the lower
    triangle of icl_ward_distance_matrix (pinned to the oracle entry by entry).  Summing N positive doubles in any order errs by less than
    N * 2^-53 of the sum, 6e-11 here; one skipped entry of 500 000 moves it by about 1e-5 relative to its neighbours' share."""
    E = inputs(n, d)["normal"]
    r = ctx.distance_bounds_check(E, kind)
    want = float(np.tril(ctx.ward_distance_matrix(E).astype(np.float64), -1).sum())
    print("bounds check n %d d %d kind %d: sum_val %.17g, fp64 sum of the exact matrix %.17g, relative difference %.3g" % (n, d, kind, r["sum_val"], want, abs(r["sum_val"] - want) / want))
    assert r["below"] == 0 and r["above"] == 0 and r["unflagged"] == 0, r
    assert abs(r["sum_val"] - want) <= 1e-9 * want


def test_clustering_with_bounds_equals_exact_distances_at_n4096(ctx):
    E = WC.mog(4096, 64, 5)
    res = {}
    try:
        for mode in (1, 2, 4):  # ICL_DIST_EXACT, ICL_DIST_BOUND, ICL_DIST_LWBOUND
            ctx.set_ward_options(mode)
            cid, rank, nc = ctx.cluster(E, 5, 50)
            res[mode] = (cid.copy(), rank.copy(), nc, ctx.last_merges().copy(), ctx.last_merge_values().copy().view(np.uint32))
            if mode != 1:
                assert ctx.last_ward_layout()[2], "the initial matrix was not filled by the integer GEMM"
                assert ctx.last_ward_bound_violations() == 0
    finally:
        ctx.set_ward_options(0)
    for mode in (2, 4):
        for got, want, what in zip(res[mode], res[1], ("cluster ids", "member order", "cluster count", "merge log", "merge values (bits)")):
            assert np.array_equal(got, want), (mode, what)
