"""FAST mode (north_star's literal path): MFMA distance tile (distance_mfma.hip) + Lance-Williams updates.
It is NOT bit-identical to clustering.go by construction (GEMM-form distances, LW instead of the centroid recompute),
so against the reference these tests bound the distance error against fp64 and REPORT id agreement with the exact mode
(SURVEY.md 7-A/7-B).  Against its own definition FAST mode is held bit for bit: tests/lw_numpy.py restates the merge loop
on the matrix the MFMA tile produced, and merge log, heights, ids and member order of the engine -- the batched loop here,
the one-merge-per-step loop in a child process -- must EQUAL the restatement's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lw_numpy as LW
from tests import ward_cases as WC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def mog(n, d, seed, k=None, sigma=0.1):
    rng = np.random.default_rng(seed)
    k = k or max(1, n // 20)
    cen = rng.standard_normal((k, d)).astype(np.float32)
    lab = rng.integers(0, k, n)
    return (cen[lab] + sigma * rng.standard_normal((n, d))).astype(np.float32), lab


@pytest.mark.parametrize("n,d", [(1, 64), (130, 64), (257, 100), (300, 2048), (129, 1000)])
def test_mfma_distance_tile_error_bound(ctx, n, d):
    E, _ = mog(n, d, n + d)
    D = ctx.distance_mfma(E)
    E64 = E.astype(np.float64)
    sq = (E64 * E64).sum(1)
    ref = np.tril(0.5 * (sq[:, None] + sq[None, :]) - E64 @ E64.T, -1)
    scale = 0.5 * (sq[:, None] + sq[None, :])
    err = np.abs(np.tril(D, -1) - ref) / np.maximum(scale, 1e-30)
    print("n=%d d=%d max |err| / (0.5(|a|^2+|b|^2)) = %.3g" % (n, d, err.max() if n > 1 else 0.0))
    assert np.all(np.diag(D) == 0)
    if n > 1:
        assert err.max() < 2e-5  # bf16x3 split operands, fp32 accumulate


def rand_index(a, b):
    from itertools import combinations

    same = 0
    tot = 0
    idx = np.random.default_rng(0).choice(len(a), min(len(a), 400), replace=False)
    for i, j in combinations(idx, 2):
        tot += 1
        same += ((a[i] == a[j] and a[i] >= 0) == (b[i] == b[j] and b[i] >= 0))
    return same / max(tot, 1)


@pytest.mark.parametrize("n,d,mn,mx", [(300, 64, 3, 30), (1000, 256, 5, 50), (2000, 2048, 5, 50)])
def test_lw_mode_agrees_with_exact_on_separated_data(ctx, n, d, mn, mx):
    from imageclust_amd import _lib

    E, lab = mog(n, d, n, k=n // 20)
    cid_e, rank_e, nc_e = ctx.cluster(E, mn, mx, _lib.UPDATE_EXACT)
    cid_f, rank_f, nc_f = ctx.cluster(E, mn, mx, _lib.UPDATE_LW)
    kept = cid_f[cid_f >= 0]
    counts = np.bincount(kept)
    assert counts.min() >= mn and counts.max() <= mx
    assert sorted(set(kept.tolist())) == list(range(nc_f))
    ri = rand_index(cid_e, cid_f)
    print("n=%d: exact %d clusters, fast %d clusters, identical ids: %.4f, Rand index %.4f" % (n, nc_e, nc_f, float((cid_e == cid_f).mean()), ri))
    assert ri > 0.98 and abs(nc_e - nc_f) <= max(2, nc_e // 20)


def test_lw_mode_constraint_errors(ctx):
    from imageclust_amd import _lib

    with pytest.raises(_lib.ICLError) as ei:
        ctx.cluster(np.zeros((10, 4), np.float32), 4, 4, _lib.UPDATE_LW)
    assert ei.value.code == _lib.ICL_ERR_CONSTRAINT
    with pytest.raises(_lib.ICLError):
        ctx.cluster(np.zeros((10, 4), np.float32), 1, 4, 7)


# ---- FAST mode against its own definition (tests/lw_numpy.py), bit for bit ----------------------------------------------------
SINGLE = os.environ.get("ICL_WARD_BATCH", "")[:1] == "0"  # the one-merge-per-step loop in THIS process (read once per process by the engine)
STATS = []  # last_ward_stats() of every FAST call same_as_lw made


def first_difference(m, v, wm, wv):
    """The first merge at which the engine's log (m, v) and the restatement's (wm, wv) part, with both pairs and both heights."""
    for t in range(min(len(m), len(wm))):
        if tuple(m[t]) != tuple(wm[t]) or v[t:t + 1].view(np.uint32)[0] != wv[t:t + 1].view(np.uint32)[0]:
            return "merge %d: engine (%d, %d) at %r, restatement (%d, %d) at %r" % (t, m[t][0], m[t][1], float(v[t]), wm[t][0], wm[t][1], float(wv[t]))
    return "the first %d merges agree; engine made %d, restatement %d" % (min(len(m), len(wm)), len(m), len(wm))


def check_against_lw(D0, want, cid, rank, nc, m, v, what):
    """One clustering result (ids, member order, merge log m, heights v) against the restatement `want` of the raw matrix D0."""
    n = len(D0)
    wcid, wrank, wnc, wm, wv = want
    same_log = len(m) == len(wm) and np.array_equal(m, wm) and np.array_equal(v.view(np.uint32), wv.view(np.uint32))
    assert same_log, "%s: %s" % (what, first_difference(m, v, wm, wv))
    assert np.array_equal(cid, wcid) and np.array_equal(rank, wrank) and nc == wnc, what
    # the stand-alone matrix IS the matrix FAST clustered: a merge of two singletons has the height of its (clamped) entry
    first = (m[:, 0] < n) & (m[:, 1] < n)
    entry = LW.clamp0(D0)[np.maximum(m[first, 0], m[first, 1]), np.minimum(m[first, 0], m[first, 1])]
    assert np.array_equal(v[first].view(np.uint32), entry.view(np.uint32)), what + ": singleton merges do not have the heights of distance_mfma's entries"


def same_as_lw(ctx, E, mn, mx, D0=None):
    from imageclust_amd import _lib

    what = "n %d, d %d, min %d, max %d" % (E.shape[0], E.shape[1], mn, mx)
    if D0 is None:
        D0 = ctx.distance_mfma(E)
    want = LW.cluster_lw(D0, mn, mx)
    if want is None:
        with pytest.raises(_lib.ICLError) as ei:
            ctx.cluster(E, mn, mx, _lib.UPDATE_LW)
        assert ei.value.code == _lib.ICL_ERR_CONSTRAINT, what
        return D0, None
    cid, rank, nc = ctx.cluster(E, mn, mx, _lib.UPDATE_LW)
    STATS.append(ctx.last_ward_stats())
    check_against_lw(D0, want, cid, rank, nc, ctx.last_merges(), ctx.last_merge_values(), what)
    assert ctx.last_ward_mode()[0] == (_lib.ROWS_SINGLE if SINGLE else _lib.ROWS_LW_FAST), what
    return D0, want


SMALL = WC.small_cases()


@pytest.mark.parametrize("name,E,mn,mx", SMALL, ids=[c[0] for c in SMALL])
def test_fast_equals_restatement_on_small_cases(ctx, name, E, mn, mx):
    """Ties on integer grids (D~ is exact there: thousands of tied entries), identical points, NaN / Inf rows, no pair left, the hub (every batch
    rolled back), quadruples (new clusters that are each other's nearest neighbours: the nested recurrence of the new-vs-new workgroup), targets
    reached inside a batch."""
    same_as_lw(ctx, E, mn, mx)


def test_fast_unsatisfiable_constraints(ctx):
    assert same_as_lw(ctx, mog(10, 4, 1)[0], 4, 4)[1] is None
    assert same_as_lw(ctx, mog(7, 4, 1)[0], 8, 9)[1] is None


@pytest.mark.parametrize("n,d", [(2, 1), (128, 64), (129, 100), (257, 6), (300, 2048)])
def test_fast_equals_restatement_across_tile_geometry(ctx, n, d):
    """dist_mfma_kernel's shapes: one tile, a full tile, a second tile row, a ragged third one, d padded to 64 and K' = 3 * 2048."""
    E = mog(n, d, n + d)[0]
    D0, _ = same_as_lw(ctx, E, 1, n)
    same_as_lw(ctx, E, 2, 9, D0)


def duplicates(d, seed, offset=0.0):
    """30 distinct rows, 10 copies of each, shuffled: coordinates that bf16 does not represent, so D~ of a pair of copies is rounding noise around
    |lo|^2 -- positive, zero or NEGATIVE."""
    rng = np.random.default_rng(seed)
    E = (np.repeat(rng.standard_normal((30, d)), 10, axis=0) + offset).astype(np.float32)
    return E[rng.permutation(len(E))]


DUP_SEED = {4: 0, 8: 0, 16: 0}


def nonpositive_pairs(E, D0):
    """(pairs of copies, those of them whose entry is <= 0, entries <= 0 in the whole triangle).  The engine stores a non-positive estimate as +0, so
    on its matrix `<= 0` counts the entries whose raw value 0.5 (n_i + n_j) - c was zero or negative."""
    tri = np.tri(len(E), len(E), -1, dtype=bool)
    dup = tri & (E[:, None, :] == E[None, :, :]).all(2)
    return int(dup.sum()), int((dup & (D0 <= 0)).sum()), int((tri & (D0 <= 0)).sum())


def check_duplicates(ctx, E, what):
    D0 = ctx.distance_mfma(E)
    pairs, nonpos, anywhere = nonpositive_pairs(E, D0)
    print("%s: %d pairs of copies, D~ <= 0 for %d of them; %d entries <= 0 in the triangle, %d of them < 0" % (what, pairs, nonpos, anywhere, int((np.tril(D0, -1) < 0).sum())))
    assert anywhere >= 1  # or the input does not test what it is for
    assert not (np.tril(D0, -1) < 0).any() and not np.signbit(D0[D0 == 0]).any()  # stored as +0
    for mn, mx in [(1, 300), (2, 12), (5, 10)]:
        same_as_lw(ctx, E, mn, mx, D0)


@pytest.mark.parametrize("d", [4, 8, 16])
def test_fast_equals_restatement_on_duplicates(ctx, d):
    """Exact duplicates, the ordinary case of an image-deduplication workload.  The matrix must hold non-positive entries off the diagonal, or the
    case does not test how the merge loop orders them.  Measured on an MI355X with seed 0, before the kernel clamped them: of the 1350 pairs of
    copies, 405 had a raw D~ < 0 at d = 4, 405 at d = 8 and 90 at d = 16 (no pair of distinct rows had one); seeds 0..5 gave 270..495, 180..405
    and 0..180 (d = 16, seed 5: none).  The unclamped engine merged the most negative pair first, at a negative height: (48, 13) at -5.7e-6,
    (105, 16) at -2.1e-5 and (102, 49) at -2.3e-5, where the definition picks the first of the zeros, (23, 1), (18, 3) and (55, 16)."""
    check_duplicates(ctx, duplicates(d, DUP_SEED[d]), "d=%d seed %d" % (d, DUP_SEED[d]))


def test_fast_equals_restatement_on_duplicates_with_a_large_common_offset(ctx):
    """The same construction shifted by +100 at d = 16: norms of 1.6e5 cancel down to distances of order 10, and the noise of D~ grows with the
    norms.  Measured with seed 0 before the clamp: 135 of the 1350 pairs of copies had a raw D~ <= 0, 90 of them < 0, down to -0.156."""
    check_duplicates(ctx, duplicates(16, DUP_SEED[16], offset=100.0), "d=16 + 100 seed %d" % DUP_SEED[16])


def test_fast_graph_replay_across_calls_on_one_context(ctx):
    """One shape (n = 400, d = 8), three consecutive FAST calls that each replay the captured graph of merge steps (>= 128 merges): max_size changes,
    then the embeddings.  A graph replayed under a stale key would cluster wrongly without any error."""
    E, E2 = WC.mog(400, 8, 7), WC.mog(400, 8, 8)
    for X, mn, mx in [(E, 2, 6), (E, 2, 9), (E2, 2, 9)]:
        _, want = same_as_lw(ctx, X, mn, mx)
        assert len(want[3]) >= 128


CHILD_CASES = {"quads": lambda: (WC.quadruples(), 1, 240), "ties600": lambda: (WC.ties(600, 5, 3, levels=3), 2, 12), "dup8": lambda: (duplicates(8, DUP_SEED[8]), 2, 12)}


@pytest.mark.parametrize("case", list(CHILD_CASES))
def test_fast_one_merge_per_step_loop_equals_restatement(ctx, tmp_path, case):
    """DESIGN.md's claim that the batched FAST loop reproduces the one-merge-per-step Lance-Williams loop bit for bit: the one-merge loop
    (ICL_WARD_BATCH=0, read once per process: a child) against the same restatement the batched loop of this process is held to."""
    E, mn, mx = CHILD_CASES[case]()
    D0, want = same_as_lw(ctx, E, mn, mx)
    np.save(tmp_path / "E.npy", E)
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ICL_WARD_BATCH="0", ICL_CHILD_UPDATE="1")
    p = subprocess.run([sys.executable, os.path.join(here, "ward_pipeline_child.py"), "--npy", str(tmp_path / "E.npy"), str(tmp_path / "out.npz"), str(mn), str(mx)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = np.load(tmp_path / "out.npz")
    check_against_lw(D0, want, r["cid"], r["rank"], int(r["nc"]), r["merges"], r["values"], case + ", one merge per step")


def test_fast_tests_are_not_vacuous(ctx):
    """The calls above went through both kinds of step of the batched loop: batches that committed several picks, and single-pick steps."""
    if SINGLE:
        pytest.skip("ICL_WARD_BATCH=0: this process runs the one-merge-per-step loop")
    if not STATS:  # run on its own
        same_as_lw(ctx, WC.quadruples(), 1, 240)
        same_as_lw(ctx, WC.hub_and_spokes(), 1, 49)
    assert any(s["steps"] < s["merges"] for s in STATS)
    assert any(s["single_pick_steps"] > 0 for s in STATS)
