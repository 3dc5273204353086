"""GPU parity tests of the Ward engine (imageclust_amd/csrc/ward.hip) against the CPU oracle, called through the
C-ABI exactly as the reference's callers would use internal/clustering (clustering.go).  Bar: BIT-EXACT."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu

MAXF = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def CL(ctx):
    from imageclust_amd import clustering

    clustering.set_default_context(ctx)
    return clustering


def ids(n):
    return ["a%d" % i for i in range(n)]


def mog(n, d, seed, k=None, sigma=0.1):
    rng = np.random.default_rng(seed)
    k = k or max(1, n // 20)
    cen = rng.standard_normal((k, d)).astype(np.float32)
    lab = rng.integers(0, k, n)
    return (cen[lab] + sigma * rng.standard_normal((n, d))).astype(np.float32)


def same_as_oracle(ctx, E, mn, mx):
    r = O.cluster(E, mn, mx, want_log=True)
    cid, rank, nc = ctx.cluster(E, mn, mx)
    assert r["ok"]
    assert np.array_equal(cid, r["cluster_id"]), "cluster ids differ"
    assert np.array_equal(rank, r["member_rank"]), "member order differs"
    assert nc == r["n_clusters"]
    m = ctx.last_merges()
    assert len(m) == r["merges"]
    assert np.array_equal(m, r["log"][:, 2:4].astype(np.int32)), "merge sequence differs"


# ---- the reference-style known-answer tests through the mirrored API ------------------------
def test_kat1(CL):
    m, ok = CL.PerformClusteringWithConstraints([[0], [1], [3], [7], [8], [20]], ids(6), 1, 2)
    assert ok and m == {0: ["a2"], 1: ["a5"], 2: ["a1", "a0"], 3: ["a4", "a3"]}


def test_kat2_maxsize_skip(CL):
    m, ok = CL.PerformClusteringWithConstraints([[0], [1], [2], [10]], ids(4), 2, 2)
    assert ok and m == {0: ["a1", "a0"], 1: ["a3", "a2"]}


def test_kat3_ban_sequence(CL):
    m, ok = CL.PerformClusteringWithConstraints([[0], [1], [3], [7], [8], [20]], ids(6), 2, 2)
    assert ok and m == {0: ["a1", "a0"], 1: ["a4", "a3"], 2: ["a5", "a2"]}


def test_kat3b_minsize_drop(CL, ctx):
    m, ok = CL.PerformClusteringWithConstraints([[0], [1], [2], [100]], ids(4), 2, 3)
    assert ok and m == {0: ["a1", "a0", "a2"]}
    cid, rank, nc = ctx.cluster(np.array([[0], [1], [2], [100]], np.float32), 2, 3)
    assert cid.tolist() == [0, 0, 0, -1] and rank.tolist() == [1, 0, 2, -1] and nc == 1


def test_kat4_constraint_errors(CL):
    assert CL.PerformClusteringWithConstraints(np.zeros((2, 1)), ids(2), 3, 5) == (None, False)
    assert CL.PerformClusteringWithConstraints(np.zeros((10, 1)), ids(10), 4, 4) == (None, False)
    assert CL.PerformClusteringWithConstraints(np.zeros((10, 1)), ids(10), 0, 4) == (None, False)


def test_kat5_optimal_clusters(CL):
    assert CL.CalculateOptimalClusters(64, 3, 6) == (16, None)
    assert CL.CalculateOptimalClusters(250000, 5, 50) == (27500, None)
    assert CL.CalculateOptimalClusters(7, 1, 7) == (4, None)
    assert CL.CalculateOptimalClusters(2, 3, 5)[1] is not None


def test_kat6_find_closest(CL):
    assert CL.FindClosestClusters(np.full((5, 5), MAXF, np.float32)) == (-1, -1)
    assert CL.FindClosestClusters(np.zeros((1, 1), np.float32)) == (-1, -1)
    D = np.full((4, 4), 5.0, np.float32)
    D[2, 1] = np.nan
    D[3, 0] = np.inf
    D[3, 2] = 1.0
    D[2, 0] = 1.0
    D[0, 3] = -1.0  # upper triangle is never read
    assert CL.FindClosestClusters(D) == (2, 0)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 257, 700])
def test_find_closest_matches_oracle_with_ties(ctx, n):
    rng = np.random.default_rng(n)
    D = rng.integers(0, 50, (n, n)).astype(np.float32)  # heavy ties
    D[rng.random((n, n)) < 0.05] = np.nan
    D[rng.random((n, n)) < 0.05] = MAXF
    assert ctx.find_closest(D) == O.find_closest(D)


@pytest.mark.parametrize("n,d", [(1, 8), (2, 1), (33, 17), (128, 64), (129, 1000), (300, 2048), (257, 6),
                                 (1153, 6), (1153, 8)])  # ten tile rows: a second band of height 2, its cap, a ragged last tile; scalar and 16-byte loads
def test_kat7_distance_matrix_bit_exact(ctx, n, d):
    rng = np.random.default_rng(n * 1000 + d)
    E = rng.standard_normal((n, d)).astype(np.float32)
    D = ctx.ward_distance_matrix(E)
    R = O.initial_distance_matrix(E)
    assert np.all(np.diag(D) == 0)
    assert np.array_equal(D, D.T)
    assert np.array_equal(D.view(np.uint32), R.view(np.uint32))
    sizes = rng.integers(1, 60, n).astype(np.int32)
    D2 = ctx.ward_distance_matrix(E, sizes)
    R2 = O.initial_distance_matrix(E, sizes)
    assert np.array_equal(D2.view(np.uint32), R2.view(np.uint32))


def test_ward_distance_and_merge_helpers(CL):
    rng = np.random.default_rng(5)
    a = CL.Cluster([3, 1], 2, rng.standard_normal(300).astype(np.float32))
    b = CL.Cluster([7], 5, rng.standard_normal(300).astype(np.float32))
    assert CL.WardDistance(a, b) == O.ward_distance(a.Centroid, 2, b.Centroid, 5)
    m = CL.MergeClusters(a, b)
    assert m.Indices == [3, 1, 7] and m.Size == 7
    assert np.array_equal(m.Centroid, O.merge_centroid(a.Centroid, 2, b.Centroid, 5))


@pytest.mark.parametrize("n,d,mn,mx,seed", [(40, 8, 1, 40, 0), (64, 32, 3, 6, 20250217), (50, 4, 2, 5, 1), (30, 3, 1, 2, 2),
                                            (25, 5, 5, 5, 3), (48, 16, 1, 3, 4), (200, 64, 3, 6, 5), (333, 2048, 5, 50, 6),
                                            (130, 1000, 1, 130, 7), (2, 4, 1, 2, 8), (1, 4, 1, 1, 9), (65, 7, 1, 1, 10)])
def test_cluster_bit_identical_to_oracle(ctx, n, d, mn, mx, seed):
    same_as_oracle(ctx, mog(n, d, seed), mn, mx)


@pytest.mark.parametrize("seed", range(4))
def test_cluster_exact_ties_and_duplicates(ctx, seed):
    rng = np.random.default_rng(seed)
    E = rng.integers(0, 4, (48, 4)).astype(np.float32)
    for mn, mx in [(1, 48), (2, 6), (1, 2), (3, 4)]:
        same_as_oracle(ctx, E, mn, mx)


# ---- inputs aimed at the batched merge loop (ward.hip: up to WB_K tentative merges per step) ----------------------
def test_batch_dependent_chain(ctx):
    """A hub that absorbs one spoke after another (spokes on orthogonal axes, growing radii): almost every merge
    involves the cluster created by the merge before it, so every batch but its first pick must be rolled back by
    the validation in the finish kernel.  Plus 1-D points with growing gaps."""
    d = 48
    E = np.zeros((d + 1, d), np.float32)
    for i in range(d):
        E[i + 1, i] = 1.1 ** i
    r = O.cluster(E, 1, d + 1, want_log=True)
    L = r["log"][:, 2:4].astype(int)
    assert sum(1 for t in range(1, len(L)) if d + t in L[t]) >= len(L) - 2  # the input does what it is meant to
    for mn, mx in [(1, d + 1), (1, 12), (2, 5)]:
        same_as_oracle(ctx, E, mn, mx)
    x = np.cumsum(1.07 ** np.arange(150)).astype(np.float32)[:, None]
    for mn, mx in [(1, 150), (2, 9), (1, 3)]:
        same_as_oracle(ctx, x, mn, mx)


def test_batch_new_clusters_merge_with_each_other(ctx):
    """Tight quadruples (pairs of pairs): clusters created in one batch are each other's nearest neighbours, which
    exercises the virtual-slot distances and new-row picks."""
    rng = np.random.default_rng(11)
    base = (rng.standard_normal((60, 12)) * 50).astype(np.float32)
    off = np.zeros((4, 12), np.float32)
    off[1, 0] = 0.01
    off[2, 0] = 0.05
    off[3, 0] = 0.061
    E = (base[:, None, :] + off[None, :, :]).reshape(-1, 12)
    E = E[rng.permutation(len(E))]
    for mn, mx in [(1, 240), (2, 4), (3, 8), (1, 2)]:
        same_as_oracle(ctx, E, mn, mx)


@pytest.mark.parametrize("n,d,mn,mx", [(100, 4096, 2, 10), (90, 2052, 1, 7), (700, 6, 1, 9), (600, 5, 2, 40)])
def test_batch_paths_wide_and_odd_dims(ctx, n, d, mn, mx):
    # d > 2048 and d % 4 != 0 take the general (non-express) finish path; small d with many points makes batches full
    same_as_oracle(ctx, mog(n, d, n + d), mn, mx)


def test_batch_heavy_ties_at_scale(ctx):
    rng = np.random.default_rng(3)
    E = rng.integers(0, 3, (600, 5)).astype(np.float32)
    for mn, mx in [(1, 600), (2, 12)]:
        same_as_oracle(ctx, E, mn, mx)


def test_batch_target_reached_inside_a_batch(ctx):
    # few merges needed (k close to n): the loop must stop after exactly n-k merges, mid-batch
    for n, mn, mx in [(100, 1, 1), (100, 1, 2), (101, 1, 2), (37, 1, 3), (64, 5, 64)]:
        same_as_oracle(ctx, mog(n, 16, n), mn, mx)


def test_cluster_all_identical_points(ctx):
    same_as_oracle(ctx, np.ones((37, 5), np.float32), 2, 4)


def test_adversarial_batches_with_distance_bounds(ctx):
    """The inputs aimed at the batched loop again, with distance bounds in the initial matrix forced (ICL_DIST_BOUND; auto mode only
    uses them from n = 4096): rolled-back batches, new clusters that are each other's nearest neighbours, heavy ties (bands that
    overflow into the full refinement loop), targets reached inside a batch, identical points, NaN / Inf, D = 4096 and D % 4 != 0."""
    ctx.set_ward_options(2)
    try:
        test_batch_dependent_chain(ctx)
        test_batch_new_clusters_merge_with_each_other(ctx)
        for args in [(100, 4096, 2, 10), (90, 2052, 1, 7), (700, 6, 1, 9), (600, 5, 2, 40)]:
            test_batch_paths_wide_and_odd_dims(ctx, *args)
        test_batch_heavy_ties_at_scale(ctx)
        test_batch_target_reached_inside_a_batch(ctx)
        same_as_oracle(ctx, np.ones((37, 5), np.float32), 2, 4)
        E = mog(40, 6, 3)
        E[7, 2] = np.nan
        E[11, 0] = np.inf
        same_as_oracle(ctx, E, 1, 3)
    finally:
        ctx.set_ward_options(0)


def test_cluster_nan_and_inf_rows(ctx):
    E = mog(40, 6, 3)
    E[7, 2] = np.nan
    E[11, 0] = np.inf
    same_as_oracle(ctx, E, 1, 3)


def test_cluster_runs_out_of_pairs(ctx):
    # max_size = 1: every pair is oversize -> the reference bans them all and breaks with len > k
    E = mog(20, 3, 1)
    r = O.cluster(E, 1, 1)
    cid, rank, nc = ctx.cluster(E, 1, 1)
    assert np.array_equal(cid, r["cluster_id"]) and nc == 20


def test_cluster_mid_size_oracle_parity(ctx):
    # ~1.3e9 scan steps in the literal oracle: a few seconds
    same_as_oracle(ctx, mog(1200, 64, 42), 5, 50)


# ---- beyond the literal oracle: oracle/ward_fast.c (pinned to ward_ref.c in tests/test_oracle_ward_fast.py) ----------------
def same_as_fast_oracle(ctx, E, mn, mx):
    f = O.cluster_fast(E, mn, mx, lazy_ban=False)
    cid, rank, nc = ctx.cluster(E, mn, mx)
    assert f["ok"]
    m = ctx.last_merges()
    assert len(m) == f["merges"], "number of merges"
    want = f["log"][:, 2:4].astype(np.int32)
    if not np.array_equal(m, want):
        t = int(np.nonzero((m != want).any(axis=1))[0][0])
        raise AssertionError("merge sequence differs first at merge %d: engine %s, oracle %s" % (t, m[t].tolist(), want[t].tolist()))
    assert np.array_equal(ctx.last_merge_values().view(np.uint32), f["vals"].view(np.uint32)), "Ward values of the merged pairs"
    assert np.array_equal(cid, f["cluster_id"]), "cluster ids differ"
    assert np.array_equal(rank, f["member_rank"]), "member order differs"
    assert nc == f["n_clusters"]
    assert ctx.last_ward_bound_violations() == 0, "a row scan found an exact value below the lower bound it replaced"
    return f


@pytest.mark.parametrize("name,E,mn,mx", WC.small_cases(), ids=[c[0] for c in WC.small_cases()])
def test_every_small_case_against_both_oracles(ctx, name, E, mn, mx):
    same_as_oracle(ctx, E, mn, mx)
    same_as_fast_oracle(ctx, E, mn, mx)


def test_distance_bounds_mode_on_every_small_case(ctx):
    """ICL_DIST_BOUND forced on the small suite (auto mode only uses it from n = 4096): the initial matrix holds proven lower
    bounds from the f32 MFMA GEMM and entries are evaluated exactly on demand by the row scans -- ties, duplicates, NaN / Inf,
    tight constraints, D not a multiple of 4 or 32, D > 2048.  Ids, member order, merge log and every merge value against both oracles."""
    ctx.set_ward_options(2)
    try:
        for name, E, mn, mx in WC.small_cases():
            try:
                same_as_oracle(ctx, E, mn, mx)
                same_as_fast_oracle(ctx, E, mn, mx)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
    finally:
        ctx.set_ward_options(0)


@pytest.mark.parametrize("layout", ["complete_rows", "recycled_columns"])
def test_lance_williams_bound_rows_on_every_small_case_and_the_adversarial_batches(ctx, monkeypatch, layout):
    """Both layouts of the bound-rows loop's matrix (include/imageclust.h icl_last_ward_layout): one column per creation id with every row complete
    (what the engine picks up to n ~ 134 000) and the 4 n^2 layout with recycled columns (larger n; ICL_WARD_WIDE=0 here).
    ICL_DIST_LWBOUND forced (auto mode only uses it from n = 4096): the rows UpdateDistanceMatrix gives the new clusters are proven
    lower bounds from the Lance-Williams recurrence, every row may hold flagged entries, picks come from exactly re-minimised rows only
    and batches are validated against the new rows' lower bounds.  Ties, duplicates (bounds of 0: everything is evaluated), NaN / Inf,
    rolled-back batches, new clusters that are each other's nearest neighbours, targets reached inside a batch, D = 4096; ids, member
    order, merge log and every merge value against both oracles.  (D % 4 != 0 keeps exact rows: those cases run as ICL_DIST_BOUND.)"""
    from imageclust_amd import _lib

    monkeypatch.setenv("ICL_WARD_WIDE", "1" if layout == "complete_rows" else "0")
    ctx.set_ward_options(4)
    try:
        for name, E, mn, mx in WC.small_cases():
            try:
                same_as_oracle(ctx, E, mn, mx)
                same_as_fast_oracle(ctx, E, mn, mx)
                if E.shape[0] > 1 and ctx.last_ward_mode()[0] == _lib.ROWS_LW_BOUND:
                    assert ctx.last_ward_layout()[0] == (layout == "complete_rows"), "matrix layout"
            except AssertionError as e:
                raise AssertionError("%s: %s" % (name, e))
        test_batch_dependent_chain(ctx)
        test_batch_new_clusters_merge_with_each_other(ctx)
        for args in [(100, 4096, 2, 10), (90, 2052, 1, 7), (700, 6, 1, 9), (600, 8, 2, 40)]:
            test_batch_paths_wide_and_odd_dims(ctx, *args)
        test_batch_heavy_ties_at_scale(ctx)
        test_batch_target_reached_inside_a_batch(ctx)
        same_as_oracle(ctx, np.ones((37, 8), np.float32), 2, 4)
        E = mog(40, 8, 3)
        E[7, 2] = np.nan
        E[11, 0] = np.inf
        same_as_oracle(ctx, E, 1, 3)
        same_as_fast_oracle(ctx, WC.mog(3000, 2048, 4), 3, 6)
        same_as_fast_oracle(ctx, WC.ties(1100, 4, 2, levels=5), 2, 9)
        grid = np.random.default_rng(3).integers(0, 3, (600, 8)).astype(np.float32)  # thousands of exact ties and duplicates (bounds of 0)
        for mn, mx in [(1, 600), (2, 12)]:
            same_as_oracle(ctx, grid, mn, mx)
        same_as_fast_oracle(ctx, WC.quadruples(seed=5, groups=250), 1, 1000)
        assert ctx.last_ward_mode()[0] == _lib.ROWS_LW_BOUND and ctx.last_ward_layout()[0] == (layout == "complete_rows")
    finally:
        ctx.set_ward_options(0)


def test_randomised_sweep_bound_rows_and_exact_rows_against_the_oracle(ctx):
    """60 random inputs (tests/ward_cases.py random_case: sizes 300-6000, D 4-2048, five data shapes incl. exact ties, duplicates, a large common
    offset, heavy tails; min 1-5, max min..1000, unsatisfiable constraints included) through both ways of filling a new cluster's row, each against
    ward_fast.c: ids, member order, merge log, every merge value.  (scratch/lb_sweep.py ran 1 240 such cases and 12 at N = 12 000 ... 40 000 in round 4: no mismatch.)"""
    rng = np.random.default_rng(20250218)
    for case in range(60):
        kind, E, mn, mx = WC.random_case(rng)
        f = O.cluster_fast(E, mn, mx, lazy_ban=False)
        for mode in (4, 2):
            ctx.set_ward_options(mode)
            try:
                where = "case %d (%s, n=%d, d=%d, min=%d, max=%d), ward mode %d" % (case, kind, E.shape[0], E.shape[1], mn, mx, mode)
                if not f["ok"]:
                    with pytest.raises(Exception):
                        ctx.cluster(E, mn, mx)
                    continue
                cid, rank, nc = ctx.cluster(E, mn, mx)
                assert np.array_equal(cid, f["cluster_id"]) and np.array_equal(rank, f["member_rank"]) and nc == f["n_clusters"], where
                assert np.array_equal(ctx.last_merges(), f["log"][:, 2:4].astype(np.int32)), where
                assert np.array_equal(ctx.last_merge_values().view(np.uint32), f["vals"].view(np.uint32)), where
            finally:
                ctx.set_ward_options(0)


def test_exact_rows_and_bound_rows_agree_with_the_oracle_at_n24000(ctx, monkeypatch):
    """The two ways the exact mode fills a new cluster's row -- 3 D unfused operations per entry (ICL_DIST_BOUND) and Lance-Williams
    lower bounds evaluated on demand (ICL_DIST_LWBOUND, what auto picks here; in both layouts of its matrix) -- on one multi-block input
    against ward_fast.c."""
    E = WC.mog(24000, 16, 1)
    for mode, wide, i8 in ((2, "1", "1"), (4, "1", "1"), (4, "0", "1"), (4, "1", "0"), (2, "1", "0")):
        monkeypatch.setenv("ICL_WARD_WIDE", wide)
        monkeypatch.setenv("ICL_DIST_I8", i8)  # bounds of the initial matrix: integer GEMM (distance_i8.hip) / f32 fmaf-chain GEMM
        ctx.set_ward_options(mode)
        try:
            same_as_fast_oracle(ctx, E, 5, 50)
            complete_rows, _, int8_bounds = ctx.last_ward_layout()
            assert complete_rows == (mode == 4 and wide == "1") and int8_bounds == (i8 == "1")
        finally:
            ctx.set_ward_options(0)


def _bound_check_cases():
    rng = np.random.default_rng(7)
    return [
        ("mog_3000x2048", WC.mog(3000, 2048, 3)),
        ("offset_100", (WC.mog(3000, 512, 4) + 100.0).astype(np.float32)),
        ("gauss_d100_padded", rng.standard_normal((2500, 100)).astype(np.float32)),
        ("gauss_d7", rng.standard_normal((2000, 7)).astype(np.float32)),
        ("near_duplicates", (np.repeat(rng.standard_normal((30, 2048)), 100, axis=0) + 1e-5 * rng.standard_normal((3000, 2048))).astype(np.float32)),
        ("exact_duplicates", np.repeat(rng.standard_normal((30, 64)), 100, axis=0).astype(np.float32)),
        ("heavy_tail", (rng.standard_cauchy((3000, 1024)) * 1e-3).astype(np.float32)),
        ("one_huge_coordinate", np.concatenate([rng.standard_normal((3000, 255)), 1e4 * rng.standard_normal((3000, 1))], axis=1).astype(np.float32)),
        ("tiny_1e-20", (1e-20 * rng.standard_normal((2000, 128))).astype(np.float32)),
        ("huge_1e15", (1e15 * rng.standard_normal((2000, 128))).astype(np.float32)),
        ("relu_like", np.maximum(rng.standard_normal((3000, 2048)) - 1.0, 0).astype(np.float32)),
        ("small_integers", rng.integers(0, 3, (3000, 32)).astype(np.float32)),
        ("mostly_zero_rows", np.concatenate([np.zeros((2990, 64)), rng.standard_normal((10, 64))]).astype(np.float32)),
        ("ragged_2049x2048", rng.standard_normal((2049, 2048)).astype(np.float32)),
    ]


@pytest.mark.parametrize("kind", [1, 2], ids=["f32_fmaf_chain_gemm", "int8_fixed_point_gemm"])
def test_every_distance_bound_against_the_value_it_bounds(ctx, kind):
    """ALL n (n - 1) / 2 entries of the initial matrix, not only the ones a merge loop happens to evaluate (icl_distance_bounds_check_dev): the
    flagged lower bound of each production kernel -- the f32 fmaf-chain GEMM and the integer GEMM on the fixed-point image of the rows
    (distance_i8.hip) -- must not exceed the exact kernel's value, and the upper bound the row scans derive from it (wupper) must not fall
    below it.  Inputs aimed at each term of the error analysis: cancellation (a large common offset, near and exact duplicates), the scale of
    the fixed-point image (one huge coordinate, heavy tails, sparse rows, rows of zeros), the exponent range (1e-20, 1e15), padded D."""
    for name, E in _bound_check_cases():
        r = ctx.distance_bounds_check(E, kind)
        assert r["below"] == 0 and r["above"] == 0 and r["unflagged"] == 0, (name, r)
        assert r["mean_gap"] >= 0.0


def test_distance_bounds_equal_exact_distances_on_near_ties(ctx):
    """Bounds vs exact initial distances on inputs built to crowd the band: N = 6000 points that are tiny perturbations of 300
    centres (pairs inside a group differ in the last bits), D = 96, and an integer grid with thousands of exact ties.  The two
    modes must give the same merge log, values, ids and member order."""
    rng = np.random.default_rng(8)
    cen = rng.standard_normal((300, 96)).astype(np.float32)
    E1 = (cen[rng.integers(0, 300, 6000)] * (1 + 1e-6 * rng.standard_normal((6000, 1)))).astype(np.float32)
    for E, mn, mx in [(E1, 5, 50), (WC.ties(5000, 5, 9, levels=6), 2, 30)]:
        res = []
        for mode in (1, 2):  # every initial distance by the exact kernel / bounds in the initial matrix
            ctx.set_ward_options(mode)
            cid, rank, nc = ctx.cluster(E, mn, mx)
            res.append((cid.copy(), rank.copy(), nc, ctx.last_merges().copy(), ctx.last_merge_values().copy()))
        ctx.set_ward_options(0)
        a = res[0]
        for b in res[1:]:
            assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            assert np.array_equal(a[3], b[3]) and np.array_equal(a[4].view(np.uint32), b[4].view(np.uint32))


def test_large_n_creation_ids_past_40960(ctx):
    """N=24 000, D=16, min=5 max=50: 21 360 merges, creation ids up to 45 359 (rows and columns of the matrix recycled ~21 000 times).  The batched
    update's spare workgroups once dropped rows >= 40 960 silently (16-iteration hit mask); ids, member order, the merge
    log and every merge value must equal the oracle's."""
    f = same_as_fast_oracle(ctx, WC.mog(24000, 16, 1), 5, 50)
    assert f["merges"] == 21360 and 24000 + f["merges"] > 40960


def test_large_n_creation_ids_past_65536(ctx):
    """N=45 000, D=8: 40 050 merges, creation ids up to 85 049 (past 2^16), 8 GB distance matrix."""
    f = same_as_fast_oracle(ctx, WC.mog(45000, 8, 2), 5, 50)
    assert f["merges"] == 40050


def test_large_n_tie_heavy_integer_set(ctx):
    """N=26 000 points on a 7^5 integer grid: thousands of exactly tied distances and duplicate points, so scan-order
    tie-breaks (clustering.go:125 strict '<') decide most merges; creation ids reach ~49 000."""
    f = same_as_fast_oracle(ctx, WC.ties(26000, 5, 4, levels=7), 5, 50)
    assert 30000 + f["merges"] > 40960


def test_large_n_tight_constraints(ctx):
    """N=20 000, min=5 max=6: the loop ends with 'no pair left' handling of ~10^6 oversize pairs (static mask in the
    engine, :228-234 in the reference)."""
    same_as_fast_oracle(ctx, WC.mog(20000, 8, 3), 5, 6)


def test_large_n_wide_rows_workgroups_run_several_blocks(ctx):
    """N=26 000, D=1024: 407 blocks of 64 slots for 256 persistent workgroups and 8 ring stages per block, i.e. the update
    kernel's next-block hand-over and the ring that runs on across blocks (both need >= 8 stages and a second block) are on
    the path for the first ~9 000 merges, against the oracle: ids, member order, merge log, every merge value."""
    f = same_as_fast_oracle(ctx, WC.mog(26000, 1024, 5), 5, 50)
    assert f["merges"] == 26000 - O.calc_optimal_clusters(26000, 5, 50)[0]


def test_benchmark_regime_d2048_n20000_against_the_oracle(ctx):
    """The benchmark's regime pinned to the CPU restatement once: D = 2048 (16 ring stages of 32 k-groups per 64-cluster block,
    the express finish path) and N = 20 000 (313 blocks for 256 persistent workgroups: workgroups run several blocks; distance
    bounds in the initial matrix, n >= 4096) against ward_fast.c: cluster ids, member order, the merge log and EVERY merge value
    (clustering.go:198-284).  17 800 merges; the oracle takes about a minute on the box's cores."""
    f = same_as_fast_oracle(ctx, WC.mog(20000, 2048, 7), 5, 50)
    assert f["merges"] == 20000 - O.calc_optimal_clusters(20000, 5, 50)[0]


def test_config2_full_size_properties_100k(ctx):
    """BASELINE.json's metric size: N=100 000, D=2048, min=5 max=50 (k=11 000, 89 000 merges, 40 GB distance matrix).  No CPU
    oracle reaches this size: size-independent properties, spot-checked merge values, idempotence (tests/ward_props.py)."""
    from tests.ward_props import check_full_size_run

    merges, _ = check_full_size_run(ctx, 100000, 2048, 20250217, 5, 50)
    assert merges == 89000


def test_one_merge_per_step_pipeline_against_oracle_large_n(tmp_path):
    """The one-merge-per-step pipeline (ICL_WARD_BATCH=0, read once per process: child) on its own against the oracle at
    N=24 000 (creation ids past 40 960): it is the second witness of the 100 000-image test below."""
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    E = WC.mog(24000, 16, 1)
    np.save(tmp_path / "E.npy", E)
    f = O.cluster_fast(E, 5, 50, lazy_ban=False)
    env = dict(os.environ, ICL_WARD_BATCH="0")
    p = subprocess.run([sys.executable, os.path.join(here, "ward_pipeline_child.py"), "--npy", str(tmp_path / "E.npy"), str(tmp_path / "out.npz"), "5", "50"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = np.load(tmp_path / "out.npz")
    assert f["ok"] and len(r["merges"]) == f["merges"] == 21360
    assert np.array_equal(r["merges"], f["log"][:, 2:4].astype(np.int32))
    assert np.array_equal(r["values"].view(np.uint32), f["vals"].view(np.uint32))
    assert np.array_equal(r["cid"], f["cluster_id"]) and np.array_equal(r["rank"], f["member_rank"]) and int(r["nc"]) == f["n_clusters"]


def test_config2_full_size_two_pipelines_agree_100k(ctx):
    """N=100 000, D=2048 again, this time as a parity statement: the batched pipeline (up to 16 merges per step, the shipped
    path) and the one-merge-per-step pipeline (ICL_WARD_BATCH=0: other update / finish / preselection kernels, the structure
    whose equality with the oracle is tested up to N=45 000) must produce the same merge log, merge values, ids and member order.
    The switch is read once per process, so the slow pipeline runs in a child."""
    import json
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    from tests import ward_pipeline_child as C

    args = (100000, 2048, 20250218, 5, 50)
    mine = C.digests(ctx, C.make_E(*args[:3]), args[3], args[4])  # (auto: bounds in the initial matrix and in the new clusters' rows)
    ctx.set_ward_options(2)  # the batched pipeline with exact rows for the new clusters
    try:
        assert C.digests(ctx, C.make_E(*args[:3]), args[3], args[4]) == mine
    finally:
        ctx.set_ward_options(0)
    env = dict(os.environ, ICL_WARD_BATCH="0", ICL_CHILD_DIST="1")  # the witness also builds every initial distance with the exact kernel
    p = subprocess.run([sys.executable, os.path.join(here, "ward_pipeline_child.py"), *map(str, args)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    other = json.loads(p.stdout.strip().splitlines()[-1])
    assert other["E"] == mine["E"], "the two processes did not cluster the same input"
    assert mine["n_merges"] == 89000
    assert other == mine


def test_config2_full_size_pipelines_agree_100k_on_the_resnet_embeddings(ctx):
    """The same parity statement on the benchmark's OWN data (workflow.go:84-94: the reference clusters what it embedded): 100 000 bf16 ResNet50
    embeddings of the structured synthetic images (non-negative features, a large common mean, thousands of near-ties per row before centring).  The
    shipped pipeline (bound rows, 32 picks per step), the batched exact-rows pipeline and -- in a child process -- the one-merge-per-step pipeline
    with every initial distance from the exact kernel must agree on the merge log, every merge value, ids and member order."""
    import json
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    from tests import ward_pipeline_child as C

    n = 100000
    E = C.make_E_real(ctx, n)
    try:
        mine = C.digests(ctx, E, 5, 50)
        assert ctx.last_ward_bound_violations() == 0
        ctx.set_ward_options(2)  # the batched pipeline with exact rows for the new clusters
        try:
            assert C.digests(ctx, E, 5, 50) == mine
            assert ctx.last_ward_bound_violations() == 0
        finally:
            ctx.set_ward_options(0)
    finally:
        del E
    env = dict(os.environ, ICL_WARD_BATCH="0", ICL_CHILD_DIST="1")
    p = subprocess.run([sys.executable, os.path.join(here, "ward_pipeline_child.py"), str(n), "2048", "-1", "5", "50"], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    other = json.loads(p.stdout.strip().splitlines()[-1])
    assert other["E"] == mine["E"], "the two processes did not embed the same matrix"
    assert mine["n_merges"] == 89000
    assert other == mine


def test_context_reuse_different_shapes(ctx):
    for (n, d) in [(50, 8), (20, 16), (90, 4)]:
        same_as_oracle(ctx, mog(n, d, n), 2, 6)


def test_graph_replay_across_calls_on_one_context(ctx):
    """One context, one shape (n = 400, d = 8): the workspace and its captured graph of merge steps survive from call to call, and
    every call needs >= 128 merges (267, 278, 200, 330 for the constraints below), so each one replays a graph.  Consecutive calls
    change ONE field of the graph's key at a time -- max_size, the Ward options (row mode, bounds or values in the matrix), the
    embeddings, the update mode -- and a graph replayed under a stale key would cluster wrongly without any error: after every
    exact call ids, member order and merge log against the literal oracle, merge values bit for bit against the fast one."""
    from imageclust_amd import _lib

    single = os.environ.get("ICL_WARD_BATCH", "")[:1] == "0"
    E, E2 = WC.mog(400, 8, 7), WC.mog(400, 8, 8)
    want = {}

    def exact(X, mn, mx, opt):
        key = (X is E2, mn, mx)
        if key not in want:
            want[key] = (O.cluster(X, mn, mx, want_log=True), O.cluster_fast(X, mn, mx, lazy_ban=False))
        r, f = want[key]
        assert r["ok"] and f["ok"] and r["merges"] >= 128
        ctx.set_ward_options(opt)
        cid, rank, nc = ctx.cluster(X, mn, mx)
        what = "options %d, E%d, min %d, max %d" % (opt, 1 + (X is E2), mn, mx)
        m = ctx.last_merges()
        assert len(m) == r["merges"], what
        assert np.array_equal(m, r["log"][:, 2:4].astype(np.int32)), what + ": merge sequence differs"
        assert np.array_equal(ctx.last_merge_values().view(np.uint32), f["vals"].view(np.uint32)), what + ": Ward values of the merged pairs"
        assert np.array_equal(cid, r["cluster_id"]) and np.array_equal(rank, r["member_rank"]) and nc == r["n_clusters"], what
        assert ctx.last_ward_bound_violations() == 0, what
        rows = _lib.ROWS_SINGLE if single else _lib.ROWS_LW_BOUND if opt == 4 else _lib.ROWS_EXACT_BATCH
        assert ctx.last_ward_mode() == (rows, opt in (2, 4)), what

    try:
        for mx in (6, 9, 6):  # max_size
            exact(E, 2, mx, 0)
        for opt in (1, 2, 4, 0):  # exact rows on values, exact rows on bounds, bound rows, auto (values below n = 4096)
            exact(E, 2, 6, opt)
        for opt in (2, 4):  # other embeddings of the same shape, with bounds in the matrix (the scans then read E)
            exact(E, 2, 6, opt)
            exact(E2, 2, 6, opt)
            exact(E, 2, 6, opt)
        exact(E2, 1, 400, 0)
        exact(E, 3, 50, 0)
        ctx.set_ward_options(0)
        cid, rank, nc = ctx.cluster(E, 3, 50, _lib.UPDATE_LW)  # FAST mode: what tests/test_fast_mode_gpu.py asserts of it
        kept = cid[cid >= 0]
        counts = np.bincount(kept)
        assert counts.min() >= 3 and counts.max() <= 50
        assert sorted(set(kept.tolist())) == list(range(nc))
        assert ctx.last_ward_mode() == (_lib.ROWS_SINGLE if single else _lib.ROWS_LW_FAST, False)
        exact(E, 3, 50, 0)
        exact(E, 3, 50, 4)
    finally:
        ctx.set_ward_options(0)


def test_cluster_property_sizes_at_scale(ctx):
    """Config-2-sized clustering (N=10000, D=2048): size-independent properties."""
    E = mog(10000, 2048, 20250217, k=500)
    cid, rank, nc = ctx.cluster(E, 5, 50)
    kept = cid[cid >= 0]
    counts = np.bincount(kept)
    assert sorted(set(kept.tolist())) == list(range(nc))
    assert counts.min() >= 5 and counts.max() <= 50
    # ranks inside each cluster are a permutation of 0..size-1
    order = np.lexsort((rank, cid))
    o = order[cid[order] >= 0]
    starts = np.r_[0, np.cumsum(counts)[:-1]]
    assert np.array_equal(rank[o], np.arange(len(o)) - np.repeat(starts, counts))
    m = ctx.last_merges()
    assert len(m) == 10000 - 1100  # k = CalculateOptimalClusters(10000,5,50) = 1100
    # every merge joins two live clusters; ids are creation ids
    assert (m[:, 0] != m[:, 1]).all() and m.max() < 10000 + len(m)
    # idempotence: same input -> same result
    cid2, rank2, _ = ctx.cluster(E, 5, 50)
    assert np.array_equal(cid, cid2) and np.array_equal(rank, rank2)


def test_merge_values_and_dendrogram(ctx, CL, tmp_path):
    """icl_last_merge_values = WardDistance (clustering.go:84) of every merged pair, bit for bit: replay the merge log
    with the oracle's centroid / distance helpers."""
    import json

    n, d = 180, 24
    E = mog(n, d, 77, k=12)
    cid, rank, nc = ctx.cluster(E, 2, 9)
    m = ctx.last_merges()
    v = ctx.last_merge_values()
    assert len(v) == len(m) > 0
    cen = {i: E[i].copy() for i in range(n)}
    size = {i: 1 for i in range(n)}
    for t, (a, b) in enumerate(m.tolist()):
        want = O.ward_distance(cen[a], size[a], cen[b], size[b])
        assert np.float32(v[t]).view(np.uint32) == np.float32(want).view(np.uint32), "merge %d" % t
        cen[n + t] = O.merge_centroid(cen[a], size[a], cen[b], size[b])
        size[n + t] = size[a] + size[b]
    Z = CL.LastDendrogram(n, ctx)
    assert Z.shape == (len(m), 4) and np.array_equal(Z[:, :2].astype(np.int32), m)
    assert np.array_equal(Z[:, 2].astype(np.float32), v) and Z[-1, 3] == size[n + len(m) - 1]
    p = str(tmp_path / "dendro.json")
    CL.ExportDendrogram(p, Z, ids(n))
    J = json.load(open(p))
    assert J["n"] == n and len(J["merges"]) == len(m) and J["merges"][0][:2] == m[0].tolist()


def test_golden_fixtures(ctx):
    import os

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "ward_mog_n64_d32.npz"))
    cid, rank, nc = ctx.cluster(g["E"], int(g["min_size"]), int(g["max_size"]))
    assert np.array_equal(cid, g["cluster_id"]) and np.array_equal(rank, g["member_rank"]) and nc == int(g["n_clusters"])
    assert np.array_equal(ctx.last_merges(), g["merges"])
    t = np.load(os.path.join(gold, "ward_ties_n48_d4.npz"))
    for mn, mx in [(1, 48), (2, 6), (1, 2), (3, 4)]:
        cid, rank, _ = ctx.cluster(t["E"], mn, mx)
        assert np.array_equal(cid, t["cid_%d_%d" % (mn, mx)]) and np.array_equal(rank, t["rank_%d_%d" % (mn, mx)])
        assert np.array_equal(ctx.last_merges(), t["merges_%d_%d" % (mn, mx)])


def test_update_distance_matrix_three_step_replay(ctx, CL):
    """icl_update_distance_matrix == UpdateDistanceMatrix (clustering.go:76-96) + RemoveRowsAndColumns (:100-116): drive the
    reference's own loop (:220-246) for three merges, the engine's matrix against the literal procedure built from the
    oracle's WardDistance / MergeClusters helpers, bit for bit after every step."""
    rng = np.random.default_rng(12)
    n, d = 14, 9
    E = rng.standard_normal((n, d)).astype(np.float32)
    clusters = [CL.NewCluster(i, E[i]) for i in range(n)]
    D = CL.ComputeInitialDistanceMatrix(clusters, ctx)
    R = O.initial_distance_matrix(E)
    assert np.array_equal(D.view(np.uint32), R.view(np.uint32))
    ref_c = [(E[i].copy(), 1) for i in range(n)]
    for step in range(3):
        i, j = CL.FindClosestClusters(D, ctx)
        assert (i, j) == O.find_closest(R) and i > j
        new = CL.MergeClusters(clusters[i], clusters[j], ctx)                       # :237
        clusters = CL.RemoveClusters(clusters, i, j) + [new]                        # :240-241
        D = CL.UpdateDistanceMatrix(D, clusters, new, i, j, ctx)                     # :244
        # literal reference procedure on the oracle side
        (ca, sa), (cb, sb) = ref_c[i], ref_c[j]
        nc = (O.merge_centroid(ca, sa, cb, sb), sa + sb)
        ref_c = [c for k, c in enumerate(ref_c) if k not in (i, j)] + [nc]
        keep = [k for k in range(R.shape[0]) if k not in (i, j)]
        R2 = np.zeros((len(keep) + 1, len(keep) + 1), np.float32)
        R2[:-1, :-1] = R[np.ix_(keep, keep)]
        for k in range(len(keep)):
            R2[k, -1] = R2[-1, k] = O.ward_distance(ref_c[k][0], ref_c[k][1], nc[0], nc[1])
        R = R2
        assert D.shape == R.shape == (n - 1 - step, n - 1 - step)
        assert np.array_equal(D.view(np.uint32), R.view(np.uint32)), "step %d" % step
        assert np.array_equal(new.Centroid, nc[0]) and new.Size == nc[1]
    # positions given in either order, and the degenerate n = 2 case
    D2 = ctx.update_distance_matrix(np.array([[0, 3], [3, 0]], np.float32), np.array([[1.0, 2.0]], np.float32), [2], 1, 0)
    assert D2.shape == (1, 1) and D2[0, 0] == 0
    with pytest.raises(Exception):
        ctx.update_distance_matrix(np.zeros((3, 3), np.float32), np.zeros((2, 2), np.float32), [1, 1], 1, 1)


def test_dot_float32_mirror(CL):
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(333).astype(np.float32), rng.standard_normal(333).astype(np.float32)
    assert CL.DotFloat32(a, b).view(np.uint32) == np.float32(O.lib().icl_ref_dot(a, b, 333)).view(np.uint32)
    with pytest.raises(ValueError):
        CL.DotFloat32(a, b[:5])
