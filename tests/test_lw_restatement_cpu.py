"""Checks of tests/lw_numpy.py, the CPU restatement that the FAST-mode GPU tests (tests/test_fast_mode_gpu.py) hold the engine to.  No GPU here:
the restatement against the exact oracle where the two must agree, against a literal dictionary version of its own rules where ties decide, and one
assertion per rule."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import lw_numpy as LW
from tests import ward_cases as WC
from tests.ward_numpy import MAXF, calc_k

F = np.float32
GAPS_LINE = np.cumsum(1.07 ** np.arange(150)).astype(np.float32)[:, None]  # the growing-gaps line of WC.small_cases()


def smallest_gap64(E, mn, mx):
    """Ward's merge loop in float64 (Lance-Williams is an identity there) under the same constraints: the smallest relative gap
    (v2 - v1) / v2 between the two best candidates over all steps.  A property of the INPUT: above the fp32 error of either
    formulation, the exact oracle and the fp32 Lance-Williams loop must pick the same pairs."""
    E = np.asarray(E, np.float64)
    n = len(E)
    k = calc_k(n, mn, mx)
    M = 2 * n
    sq = (E * E).sum(1)
    V = np.full((M, M), np.nan)
    V[:n, :n] = 0.5 * np.maximum(sq[:, None] + sq[None, :] - 2.0 * E @ E.T, 0.0)
    K = np.full((M, M), np.inf)
    K[:n, :n] = np.where(np.tri(n, n, -1, dtype=bool) & (2 <= mx), V[:n, :n], np.inf)
    size = np.zeros(M, np.int64)
    size[:n] = 1
    live = np.zeros(M, bool)
    live[:n] = True
    gap = np.inf
    for t in range(n - k):
        flat = int(np.argmin(K))
        i, j = divmod(flat, M)
        v1 = K[i, j]
        if not np.isfinite(v1):
            break
        K[i, j] = np.inf
        v2 = K.min()
        if np.isfinite(v2) and v2 > 0:
            gap = min(gap, (v2 - v1) / v2)
        c, sa, sb = n + t, size[i], size[j]
        live[i] = live[j] = False
        K[i, :] = K[:, i] = K[j, :] = K[:, j] = np.inf
        xs = np.flatnonzero(live & (size + sa + sb <= mx))
        size[c] = sa + sb
        live[c] = True
        sx = size[xs]
        V[c, xs] = K[c, xs] = ((sa + sx) * V[np.maximum(i, xs), np.minimum(i, xs)] + (sb + sx) * V[np.maximum(j, xs), np.minimum(j, xs)] - sx * v1) / (sa + sb + sx)
    return gap


SEPARATED = ([("hub", WC.hub_and_spokes(), mn, mx) for mn, mx in [(1, 49), (1, 12), (2, 5)]]
             + [("gaps", GAPS_LINE, mn, mx) for mn, mx in [(1, 150), (2, 9), (1, 3)]]
             + [("mog200", WC.mog(200, 16, 5), mn, mx) for mn, mx in [(1, 200), (3, 6), (2, 20)]])


@pytest.mark.parametrize("name,E,mn,mx", SEPARATED, ids=["%s_%d_%d" % (c[0], c[2], c[3]) for c in SEPARATED])
def test_restatement_equals_exact_oracle_on_separated_inputs(name, E, mn, mx):
    gap = smallest_gap64(E, mn, mx)
    print("%s min %d max %d: smallest relative gap between the two best candidates %.3g" % (name, mn, mx, gap))
    assert gap > 1e-4  # a condition on the input
    r = O.cluster(E, mn, mx, want_log=True)
    f = O.cluster_fast(E, mn, mx, lazy_ban=False)
    assert r["ok"] and f["ok"]
    cid, rank, nc, merges, values = LW.cluster_lw(O.initial_distance_matrix(E), mn, mx)
    assert np.array_equal(merges, r["log"][:, 2:4].astype(np.int32)), "merge sequence differs"
    assert np.array_equal(cid, r["cluster_id"]) and np.array_equal(rank, r["member_rank"]) and nc == r["n_clusters"]
    want = f["vals"].astype(np.float64)
    rel = np.abs(values.astype(np.float64) - want) / np.maximum(want, 1e-300)
    print("largest relative height error %.3g over %d merges" % (rel.max() if len(rel) else 0.0, len(rel)))
    assert len(values) == len(want) and np.all(rel <= 1e-5)


def literal_lw(D0, mn, mx):
    """The rules of lw_numpy's docstring as dictionaries and scalar loops (the pattern of ward_numpy.cluster_creation_id)."""
    n = D0.shape[0]
    k = calc_k(n, mn, mx)
    if k is None:
        return None

    def clamp(v):
        v = F(v)
        return v if (v > 0 or np.isnan(v)) else F(0)

    size = {i: 1 for i in range(n)}
    members = {i: [i] for i in range(n)}
    alive = set(range(n))
    dist = {(i, j): clamp(D0[i, j]) for i in range(n) for j in range(i)}
    merges, values = [], []
    nxt = n
    with np.errstate(all="ignore"):
        while len(alive) > k:
            best = None
            for (i, j), v in dist.items():
                if i not in alive or j not in alive or size[i] + size[j] > mx or not (v < MAXF):
                    continue
                if best is None or (v, i, j) < best:
                    best = (v, i, j)
            if best is None:
                break
            dab, a, b = best
            c = nxt
            nxt += 1
            alive.discard(a)
            alive.discard(b)
            sa, sb = size[a], size[b]
            for x in alive:
                sx = size[x]
                if sx + sa + sb > mx:
                    continue
                dax, dbx = dist[(max(a, x), min(a, x))], dist[(max(b, x), min(b, x))]
                p1 = F(F(sa + sx) * dax)
                p2 = F(F(sb + sx) * dbx)
                p3 = F(F(sx) * dab)
                dist[(c, x)] = clamp(F(F(F(p1 + p2) - p3) / F(sa + sb + sx)))
            size[c] = sa + sb
            members[c] = members[a] + members[b]
            alive.add(c)
            merges.append((a, b))
            values.append(dab)
    cid = np.full(n, -1, np.int32)
    rank = np.full(n, -1, np.int32)
    nid = 0
    for c in sorted(alive):
        if size[c] < mn:
            continue
        for r, m in enumerate(members[c]):
            cid[m] = nid
            rank[m] = r
        nid += 1
    return cid, rank, nid, np.array(merges, np.int32).reshape(-1, 2), np.array(values, F)


def same(got, want):
    assert (got is None) == (want is None)
    if got is None:
        return
    assert np.array_equal(got[3], want[3]), "merge sequence differs"
    assert np.array_equal(got[4].view(np.uint32), want[4].view(np.uint32)), "heights differ"
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_literal_rules_on_ties(seed):
    D0 = O.initial_distance_matrix(WC.ties(48, 4, seed))
    assert (np.unique(D0[np.tri(48, 48, -1, dtype=bool)], return_counts=True)[1] > 20).any()  # tie-heavy indeed
    for mn, mx in [(1, 48), (2, 6), (1, 2), (3, 4), (5, 7)]:
        same(LW.cluster_lw(D0, mn, mx), literal_lw(D0, mn, mx))


def test_restatement_equals_literal_rules_with_negative_and_nan_entries():
    rng = np.random.default_rng(3)
    D0 = O.initial_distance_matrix(WC.mog(40, 6, 3))
    tri = np.argwhere(np.tri(40, 40, -1, dtype=bool))
    for (i, j) in tri[rng.choice(len(tri), 30, replace=False)]:
        D0[i, j] = rng.choice([-1e-3, -0.0, np.nan, np.inf, MAXF])
    for mn, mx in [(1, 40), (1, 3), (2, 6)]:
        same(LW.cluster_lw(D0, mn, mx), literal_lw(D0, mn, mx))


def line(n=8):
    return O.initial_distance_matrix(np.cumsum(1.5 ** np.arange(n)).astype(np.float32)[:, None])


def test_negative_initial_entry_is_picked_first_with_height_plus_zero():
    D0 = line()
    D0[6, 2] = -3e-4
    _, _, _, merges, values = LW.cluster_lw(D0, 1, 8)
    assert tuple(merges[0]) == (6, 2)
    assert values[0] == 0 and not np.signbit(values[0])
    D0[6, 2] = -0.0  # -0 as well: the first of the zeros in (row, column) order, stored as +0
    D0[7, 1] = 0.0
    _, _, _, merges, values = LW.cluster_lw(D0, 1, 8)
    assert tuple(merges[0]) == (6, 2) and not np.signbit(values[0])


def test_nan_entry_is_never_picked_and_its_rows_stay_nan():
    D0 = line(6)
    D0[1, 0] = np.nan  # the pair that would have been first
    cid, rank, nc, merges, values = LW.cluster_lw(D0, 1, 6)
    assert len(merges) == 3 and not np.isnan(values).any()
    assert tuple(merges[0]) == (2, 1)  # the next smallest; the new row (id 6) holds NaN against 0, not a +0 that would win the next pick
    assert np.isnan(LW.lw_row(F(np.nan), F(1), F(1), 1, 1, np.array([1]))[0])
    assert tuple(merges[1]) != (6, 0) and (values > 0).all()
    assert cid[0] != cid[1]  # 0 never joins a cluster that holds 1 (min_size 1: every cluster is kept)
    # every pair is NaN: nothing is ever a candidate
    assert len(LW.cluster_lw(np.full((5, 5), np.nan, F), 1, 5)[3]) == 0


def test_max_size_one_returns_no_merges():
    cid, rank, nc, merges, values = LW.cluster_lw(line(), 1, 1)
    assert merges.shape == (0, 2) and values.shape == (0,) and nc == 8
    assert np.array_equal(cid, np.arange(8)) and np.all(rank == 0)


def test_one_and_two_rows():
    cid, rank, nc, merges, values = LW.cluster_lw(np.zeros((1, 1), F), 1, 1)
    assert (cid.tolist(), rank.tolist(), nc, len(merges)) == ([0], [0], 1, 0)
    D0 = np.array([[0, 0], [2.5, 0]], F)
    cid, rank, nc, merges, values = LW.cluster_lw(D0, 2, 2)
    assert (cid.tolist(), rank.tolist(), nc, merges.tolist(), values.tolist()) == ([0, 0], [1, 0], 1, [[1, 0]], [2.5])
    cid, rank, nc, merges, values = LW.cluster_lw(D0, 1, 1)
    assert (cid.tolist(), nc, len(merges)) == ([0, 1], 2, 0)
    assert LW.cluster_lw(D0, 3, 3) is None and LW.cluster_lw(D0, 2, 1) is None  # unsatisfiable


@pytest.mark.parametrize("n,mn,mx", [(8, 1, 8), (12, 1, 4), (30, 1, 30), (30, 1, 2)])
def test_loop_stops_after_exactly_n_minus_k_merges(n, mn, mx):
    """Constraints under which mergeable pairs are left at the target (k >= 2 clusters, two of which still fit max_size): the target stops the loop."""
    cid, rank, nc, merges, values = LW.cluster_lw(line(n), mn, mx)
    assert np.sort(np.bincount(cid[cid >= 0]))[:2].sum() <= mx
    assert len(merges) == len(values) == n - calc_k(n, mn, mx)
    assert len(set(merges.ravel().tolist())) == 2 * len(merges)  # no id is merged twice
    assert merges.max() < n + len(merges) and (merges[:, 0] > merges[:, 1]).all()
