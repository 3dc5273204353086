"""Checks of tests/lw_seeded_numpy.py, the CPU restatement that tests/test_seeded_fast_gpu.py holds icl_cluster_seeded_fast to.  No GPU here: the
restatement from all-ones seeds against tests/lw_numpy.py, against a literal dictionary version of its own rules, against the exact seeded checker
where the two must agree, one planted mistake per rule, and the three new symbols of the C ABI."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import lw_numpy as LW
from tests import lw_seeded_numpy as LS
from tests import seeded_cases as SC
from tests import ward_cases as WC
from tests.test_lw_restatement_cpu import GAPS_LINE, SEPARATED, smallest_gap64
from tests.ward_numpy import MAXF, calc_k

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- all-ones seeds are lw_numpy's loop ---------------------------------------------------------------------------------------------------
def planted_matrix():
    """test_lw_restatement_cpu's matrix with negative, -0, NaN, Inf and MaxFloat32 entries"""
    rng = np.random.default_rng(3)
    D0 = O.initial_distance_matrix(WC.mog(40, 6, 3))
    tri = np.argwhere(np.tri(40, 40, -1, dtype=bool))
    for (i, j) in tri[rng.choice(len(tri), 30, replace=False)]:
        D0[i, j] = rng.choice([-1e-3, -0.0, np.nan, np.inf, MAXF])
    return D0


ONES = ([(name, O.initial_distance_matrix(E), mn, mx) for name, E, mn, mx in SEPARATED]
        + [("ties%d" % s, O.initial_distance_matrix(WC.ties(48, 4, s)), mn, mx) for s in range(4) for mn, mx in [(1, 48), (2, 6), (1, 2), (3, 4), (5, 7)]]
        + [("planted", planted_matrix(), mn, mx) for mn, mx in [(1, 40), (1, 3), (2, 6)]]
        + [("line", O.initial_distance_matrix(GAPS_LINE[:8]), mn, mx) for mn, mx in [(1, 8), (1, 1), (3, 3), (9, 9)]])


@pytest.mark.parametrize("name,D0,mn,mx", ONES, ids=["%s_%d_%d" % (c[0], c[2], c[3]) for c in ONES])
def test_all_ones_seeds_equal_the_unseeded_restatement(name, D0, mn, mx):
    n = len(D0)
    a = LW.cluster_lw(D0, mn, mx)
    for D in (D0, np.tril(LW.clamp0(D0))):  # the raw matrix, and the clamped one the engine's stand-alone call gives: the clamp commutes with the scale
        b = LS.cluster_lw_seeded(D, np.ones(n, np.int32), mn, mx)
        if a is None:
            assert b["status"] == LS.ERR_CONSTRAINT and (b["cluster_id"] == -1).all()
            continue
        assert b["status"] == LS.OK
        assert np.array_equal(b["log"], a[3]) and np.array_equal(bits(b["values"]), bits(a[4])), "log or heights differ"
        assert np.array_equal(b["cluster_id"], a[0]) and np.array_equal(b["seed_rank"], a[1]) and b["n_clusters"] == a[2]


def test_all_ones_entry_is_the_unsized_entry():
    """num / den = 1/2 and the factor 2 are exact for every finite entry below 2^127"""
    v = np.array([0.0, 1e-45, 1e-38, 3.3e-7, 1.0, 7.0 / 3.0, 1.6e38, np.inf, np.nan], F)
    D = np.zeros((len(v) + 1, len(v) + 1), F)
    D[len(v), :len(v)] = v
    got = LS.sized_matrix(D, np.ones(len(v) + 1, np.int32))[len(v), :len(v)]
    assert np.array_equal(bits(got[:-1]), bits(v[:-1])) and np.isnan(got[-1])
    assert LS.sized_matrix(np.full((2, 2), 1.8e38, F), [1, 1])[1, 0] == np.inf  # from 2^127 on the doubling overflows


# ---- a literal dictionary version, with one switch per planted mistake ----------------------------------------------------------------------
def literal(D, C, ss, mn, mx, kt=0, mistake=None, stale_frozen=None):
    """The rules of lw_seeded_numpy's docstring as dictionaries and scalar loops -> dict like cluster_lw_seeded's, plus C_out."""
    ss = [int(s) for s in ss]
    m = len(ss)
    C = np.asarray(C, F)
    items = {i: abs(s) for i, s in enumerate(ss)}
    N = sum(items.values())
    fail = lambda st: dict(status=st, cluster_id=np.full(m, -1, np.int32), seed_rank=np.full(m, -1, np.int32), n_clusters=0, log=np.zeros((0, 2), np.int32),
                           values=np.zeros(0, F), C_out=np.zeros_like(C))
    if N >= 1 << 30 or any(s > mx for s in ss):
        return fail(LS.ERR_UNSUPPORTED)
    k = kt if kt > 0 else calc_k(m if mistake == "k_from_seeds" else N, mn, mx)
    if k is None:
        return fail(LS.ERR_CONSTRAINT)
    kmax = min(max(mx, 1), max(N, 1))
    size = {i: (items[i] if ss[i] > 0 or mistake == "frozen_mergeable" else kmax) for i in range(m)}

    def clamp(v):
        v = F(v)
        return v if (v > 0 or np.isnan(v)) else F(0)

    dist = {}
    with np.errstate(all="ignore"):
        for i in range(m):
            for j in range(i):
                scale = F(0.5) if mistake == "scale_half" else F(F(items[i] * items[j]) / F(items[i] + items[j]))
                sq = F(D[i, j]) if mistake == "no_factor_2" else F(F(2) * F(D[i, j]))
                v = F(scale * sq)
                dist[(i, j)] = v if mistake == "no_clamp" else clamp(v)
    alive, seq, cen = set(range(m)), {i: [i] for i in range(m)}, {i: C[i] for i in range(m)}
    wsize = {i: (kmax if stale_frozen is not None and stale_frozen[i] else items[i]) for i in range(m)}  # the weights of C_out
    log, values = [], []
    with np.errstate(all="ignore"):
        while len(alive) > k:
            best = None
            for (i, j), v in dist.items():
                if i not in alive or j not in alive or size[i] + size[j] > kmax or not (v < MAXF):
                    continue
                if best is None or (v, i, j) < best:
                    best = (v, i, j)
            if best is None:
                break
            dab, a, b = best
            c = m + len(log)
            alive.discard(a)
            alive.discard(b)
            sa, sb = size[a], size[b]
            for x in alive:
                sx = size[x]
                if sx + sa + sb > kmax:
                    continue
                dax, dbx = dist[(max(a, x), min(a, x))], dist[(max(b, x), min(b, x))]
                p1, p2, p3 = F(F(sa + sx) * dax), F(F(sb + sx) * dbx), F(F(sx) * dab)
                dist[(c, x)] = clamp(F(F(F(p1 + p2) - p3) / F(sa + sb + sx)))
            size[c], items[c], wsize[c] = sa + sb, items[a] + items[b], wsize[a] + wsize[b]
            seq[c] = seq[a] + seq[b]
            cen[c] = np.array([F(F(F(F(wsize[a]) * x) + F(F(wsize[b]) * y)) / F(wsize[a] + wsize[b])) for x, y in zip(cen[a], cen[b])], F).reshape(C.shape[1:])
            alive.add(c)
            log.append((a, b))
            values.append(dab)
    cid, rank, C_out, nid = np.full(m, -1, np.int32), np.full(m, -1, np.int32), np.zeros_like(C), 0
    for c in sorted(alive):
        C_out[seq[c][0]] = cen[c]
        if (len(seq[c]) if mistake == "drop_by_seeds" else items[c]) < mn:
            continue
        for r, s in enumerate(seq[c]):
            cid[s], rank[s] = nid, r
        nid += 1
    return dict(status=LS.OK, cluster_id=cid, seed_rank=rank, n_clusters=nid, log=np.array(log, np.int32).reshape(-1, 2), values=np.array(values, F), C_out=C_out)


def restated(D, C, ss, mn, mx, kt=0):
    r = LS.cluster_lw_seeded(D, ss, mn, mx, kt)
    r["C_out"] = LS.centroids_from_log(C, ss, r["log"]) if r["status"] == LS.OK else np.zeros_like(np.asarray(C, F))
    return r


def differences(a, b):
    """The fields in which two results differ (C_out and heights as bits)"""
    out = [k for k in ("status", "n_clusters") if a[k] != b[k]]
    out += [k for k in ("cluster_id", "seed_rank", "log") if not np.array_equal(a[k], b[k])]
    out += [k for k in ("values", "C_out") if not SC.same_bits(a[k], b[k])]
    return out


def half_sqdist(C):
    """The exact singleton matrix of the rows, standing in for the engine's D~ on the CPU"""
    return np.tril(O.initial_distance_matrix(np.ascontiguousarray(C, F)), -1) if len(C) else np.zeros((0, 0), F)


def problems():
    """(name, D, C, seed_size, min, max, k_target): mixed sizes, frozen seeds (one below min_size, one above max_size), a seed of max_size, duplicated
    centroids; exact ties; a k_target beyond what the sizes allow; a raw matrix with negative and NaN entries; refused problems; m = 0, 1, 2."""
    out = []
    for m, d, seed in [(17, 3, 1), (40, 5, 2), (64, 8, 3)]:
        for ties in (False, True):
            C, ss, mn, mx = SC.mixed_problem(m, d, seed, ties=ties)
            D = half_sqdist(C)
            out += [("m%d%s" % (m, "t" if ties else ""), D, C, ss, mn, mx, 0), ("m%d%s_k" % (m, "t" if ties else ""), D, C, ss, mn, mx, max(1, m // 8))]
    C, ss, mn, mx = SC.mixed_problem(30, 4, 7)
    D = half_sqdist(C)
    rng = np.random.default_rng(5)
    tri = np.argwhere(np.tri(30, 30, -1, dtype=bool))
    for (i, j) in tri[rng.choice(len(tri), 25, replace=False)]:
        D[i, j] = rng.choice([-1e-3, -0.0, np.nan, np.inf])
    out.append(("raw", D, C, ss, mn, mx, 0))
    out.append(("small_frozen", D, C, np.where(np.arange(30) % 3 == 0, -np.abs(ss), np.abs(ss)).astype(np.int32), 2, mx, 0))
    C, ss, mn, mx = SC.mixed_problem(12, 3, 9, frozen_every=0)
    out.append(("unfrozen", half_sqdist(C), C, ss, mn, mx, 0))
    out.append(("oversized", half_sqdist(C), C, np.where(np.arange(12) == 5, mx + 1, ss).astype(np.int32), mn, mx, 0))
    out.append(("unsatisfiable", half_sqdist(C[:3]), C[:3], np.array([3, 3, 4], np.int32), 4, 4, 0))
    for m in (0, 1, 2):
        out.append(("m%d" % m, half_sqdist(C[:m]), C[:m], np.array([2, 1][:m], np.int32), 1, 4, 1 if m == 2 else 0))
    return out


PROBLEMS = problems()


@pytest.mark.parametrize("name,D,C,ss,mn,mx,kt", PROBLEMS, ids=[p[0] for p in PROBLEMS])
def test_restatement_equals_literal_rules(name, D, C, ss, mn, mx, kt):
    assert differences(restated(D, C, ss, mn, mx, kt), literal(D, C, ss, mn, mx, kt)) == []


def test_problems_hold_what_they_are_for():
    res = {p[0]: restated(*p[1:]) for p in PROBLEMS}
    assert res["oversized"]["status"] == LS.ERR_UNSUPPORTED and res["unsatisfiable"]["status"] == LS.ERR_CONSTRAINT and res["m0"]["status"] == LS.ERR_CONSTRAINT
    assert res["m1"]["status"] == LS.OK and res["m1"]["n_clusters"] == 1 and len(res["m2"]["log"]) == 1
    ok = [p for p in PROBLEMS if res[p[0]]["status"] == LS.OK]
    assert any((p[3] < 0).any() for p in ok) and any(len(set(np.abs(p[3]).tolist())) > 2 for p in ok)
    early = [p[0] for p in ok if len(res[p[0]]["log"]) < max(0, len(p[3]) - LS.admit(p[3], p[4], p[5], p[6])[2])]
    assert early and any(p[6] > 0 for p in ok)  # runs that end for want of pairs
    assert any(len(res[p[0]]["log"]) == len(p[3]) - LS.admit(p[3], p[4], p[5], p[6])[2] > 0 for p in ok)  # ... and runs that reach k
    for p in ok:  # a frozen seed is never merged, a dropped cluster has fewer than min_size ITEMS
        assert not set(np.flatnonzero(p[3] < 0).tolist()) & set(res[p[0]]["log"].ravel().tolist()), p[0]
        for c, seq, items in LS.final_list(p[3], p[4], res[p[0]]["log"])[3]:
            assert (res[p[0]]["cluster_id"][seq[0]] == -1) == (items < p[4]), p[0]


# ---- where FAST and exact must agree --------------------------------------------------------------------------------------------------------
def partition(cid):
    return {frozenset(np.flatnonzero(cid == c).tolist()) for c in set(cid.tolist()) if c >= 0}, frozenset(np.flatnonzero(cid < 0).tolist())


@pytest.mark.parametrize("mn,mx", [(1, 200), (3, 6), (2, 20)])
def test_resumed_from_an_exact_cut_equals_the_exact_seeded_checker_on_a_separated_mixture(mn, mx):
    """Seeds made by cutting an exact-oracle run of the separated mixture (test_lw_restatement_cpu's mog200: relative gap between the two best
    candidates above 1e-4 at every step): resumed in FAST mode, the final partition is the exact seeded checker's."""
    E = WC.mog(200, 16, 5)
    assert smallest_gap64(E, mn, mx) > 1e-4
    r = O.cluster(E, mn, mx, want_log=True)
    log = r["log"][:, 2:4].astype(np.int32)
    for t in SC.cuts(len(log)):
        C2, ss2, seeds, ids = SC.state_after(E, np.ones(200, np.int32), log, t)
        ref = SC.run(C2, ss2, mn, mx)
        got = LS.cluster_lw_seeded(half_sqdist(C2), ss2, mn, mx)
        assert ref["status"] == got["status"] == LS.OK and len(set(np.abs(ss2).tolist())) > 1
        assert partition(got["cluster_id"]) == partition(ref["cluster_id"]), "cut at %d" % t
        assert np.array_equal(got["log"], ref["log"]) and np.array_equal(got["seed_rank"], ref["seed_rank"]), "cut at %d" % t


# ---- planted mistakes -----------------------------------------------------------------------------------------------------------------------
MISTAKES = ["scale_half", "no_factor_2", "frozen_mergeable", "k_from_seeds", "drop_by_seeds", "no_clamp"]


@pytest.mark.parametrize("mistake", MISTAKES)
def test_planted_mistake_is_reported(mistake):
    """Each mistake, planted in the literal version, differs from the restatement on at least one of the problems above -- and on none without it
    (test_restatement_equals_literal_rules)."""
    seen = {p[0]: differences(restated(*p[1:]), literal(*p[1:], mistake=mistake)) for p in PROBLEMS}
    print(mistake, {k: v for k, v in seen.items() if v})
    assert any(seen.values()), mistake


def test_planted_mistake_c_out_weighted_by_effective_sizes_after_unfreezing():
    """A state whose frozen seeds are unfrozen for the next call: C_out must weigh them by their items.  An implementation that kept the effective
    size (max_size) of a seed that WAS frozen merges the same pairs and returns other centroids."""
    C, ss, mn, mx = SC.mixed_problem(40, 5, 2)
    was = ss < 0
    now = np.where(np.abs(ss) > mx, ss, np.abs(ss)).astype(np.int32)  # (the one above max_size stays frozen: unfrozen it is refused)
    D = half_sqdist(C)
    good = restated(D, C, now, mn, mx)
    merged = set(good["log"].ravel().tolist())
    assert good["status"] == LS.OK and any(i in merged for i in np.flatnonzero(was & (now > 0)))  # an unfrozen seed did merge
    assert differences(good, literal(D, C, now, mn, mx)) == []
    assert differences(good, literal(D, C, now, mn, mx, stale_frozen=was & (now > 0))) == ["C_out"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    from imageclust_amd import _lib
    from tests.test_abi import declared_symbols

    new = {"icl_cluster_seeded_fast", "icl_cluster_seeded_fast_dev", "icl_distance_mfma_seeded_dev"}
    assert new <= set(declared_symbols())
    assert new <= {s[0] for s in _lib.SYMBOLS}
    _lib.load()
    raw = ctypes.CDLL(_lib.SO_PATH)
    assert all(hasattr(raw, n) for n in new)
    sig = {s[0]: s[2] for s in _lib.SYMBOLS}
    assert sig["icl_cluster_seeded_fast"] == sig["icl_cluster_seeded"] and sig["icl_cluster_seeded_fast_dev"] == sig["icl_cluster_seeded_dev"]
