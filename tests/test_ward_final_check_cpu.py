"""The final-matrix checker (tests/ward_final_check.py) can fail: a dump built from the oracle alone passes, and each fault planted into it -- one
at a time -- is reported as exactly that finding.  CPU only; the GPU module (tests/test_ward_final_matrix_gpu.py) feeds the same checker with what
icl_ward_dump_pairs_dev reads out of the engine's workspace."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import test_lw_bound_cpu as LWB
from tests import ward_cases as WC
from tests import ward_final_check as WFC

SIGN = np.uint32(0x80000000)


def oracle_dump(E, mn, mx, rows=WFC.ROWS_LW_BOUND, complete=True, seed=0):
    """What a faultless engine would dump: the oracle's values for every pair of live clusters, a third of the entries the mode may flag replaced
    by a flagged lower bound R (1 - 1e-3), the mirror equal to the entries (complete rows) or absent, the restated constants."""
    n, d = E.shape
    f = O.cluster_fast(E, mn, mx, lazy_ban=False)
    assert f["ok"]
    log = f["log"][:, 2:4]
    cent, size, live = WFC.replay(E, log)
    R = O.initial_distance_matrix(cent[live], size[live].astype(np.int32))
    rng = np.random.default_rng(seed)
    pick = np.tril(rng.random(R.shape) < 1.0 / 3.0, -1)
    if rows != WFC.ROWS_LW_BOUND:
        pick &= (live[:, None] < n) & (live[None, :] < n)
    pick |= pick.T
    low = (R.astype(np.float64) * (1.0 - 1e-3)).astype(np.float32)
    ent = np.where(pick, low.view(np.uint32) | SIGN, R.view(np.uint32)).astype(np.uint32)
    np.fill_diagonal(ent, 0)
    g1, delta2 = LWB.consts(E, d, mx)
    lb = rows == WFC.ROWS_LW_BOUND
    dump = {"ids": live.astype(np.int32), "sizes": size[live].astype(np.int32), "centroids": cent[live].copy(), "row_filled": np.ones(len(live), bool),
            "entries": ent, "mirror": ent.copy() if complete and lb else np.zeros_like(ent), "lb_g1": g1 if lb else np.float32(0),
            "lb_delta2": delta2 if lb else np.float32(0), "row_mode": rows, "complete_rows": complete and lb, "n": n, "d": d, "merges": len(log),
            "max_size": mx, "init_bounds": True}
    return dump, log, R, live, size[live]


@pytest.fixture(scope="module")
def base():
    E = WC.mog(60, 16, 5)
    dump, log, R, live, sz = oracle_dump(E, 3, 12)
    # a pair the checker looks at (i > j, not oversize) with a merged cluster and a value well inside the fp32 range
    ok = np.tril(np.ones(R.shape, bool), -1) & ((sz[:, None] + sz[None, :]) <= 12) & (R > 0) & ((live[:, None] >= 60) | (live[None, :] >= 60))
    i, j = [int(x[0]) for x in np.nonzero(ok)]
    return E, dump, log, R, (i, j)


def run(base, edit, mn=3, mx=12):
    E, dump, log, R, ij = base
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dump.items()}
    edit(d, R, ij)
    return WFC.check(E, mn, mx, log, d)


def only(res, name, count=1):
    got = {k: v for k, v in res["counts"].items() if v}
    assert got == {name: count}, (got, res["offenders"])


def test_a_dump_made_by_the_oracle_passes_in_every_mode_and_layout():
    E = WC.mog(60, 16, 5)
    # (min 1, max 3 for the exact-rows modes: singletons stay alive, and only their pairs may be flagged there)
    for rows, complete, mn, mx in [(WFC.ROWS_LW_BOUND, True, 3, 12), (WFC.ROWS_LW_BOUND, False, 3, 12), (WFC.ROWS_EXACT_BATCH, False, 1, 3), (WFC.ROWS_SINGLE, False, 1, 3)]:
        dump, log, R, live, sz = oracle_dump(E, mn, mx, rows, complete)
        res = WFC.check(E, mn, mx, log, dump)
        WFC.assert_clean(res, "rows %d complete %s" % (rows, complete))
        assert res["checked"] + res["left_out"]["oversize"] + res["left_out"]["unfilled"] == res["pairs"] == len(live) * (len(live) - 1) // 2
        assert res["left_out"]["oversize"] > 0 and res["left_out"]["unfilled"] == 0 and res["flagged_nonzero"] > 0
        assert (res["flagged_nonzero_merged"] > 0) == (rows == WFC.ROWS_LW_BOUND)
        assert abs(res["gap"]["median"] - 1e-3) < 1e-6 and res["gap"]["worst"] < 1.001e-3
        if rows == WFC.ROWS_LW_BOUND:
            assert res["delta2"]["rel"] == 0.0 and res["max_norm"] <= res["M"]


def test_a_flagged_entry_one_ulp_above_the_value(base):
    def edit(d, R, ij):
        d["entries"][ij] = (R.view(np.uint32)[ij] + 1) | SIGN
    only(run(base, edit), "bound_above")


def test_a_flagged_entry_equal_to_the_value_is_a_valid_bound(base):
    def edit(d, R, ij):
        d["entries"][ij] = R.view(np.uint32)[ij] | SIGN
    WFC.assert_clean(run(base, edit))


@pytest.mark.parametrize("step", [1, -1])
def test_an_unflagged_entry_one_ulp_off_the_value(base, step):
    def edit(d, R, ij):
        d["entries"][ij] = np.uint32(int(R.view(np.uint32)[ij]) + step)
    only(run(base, edit), "exact_differs")


def test_the_same_two_in_the_mirror_only(base):
    def above(d, R, ij):
        d["mirror"][ij] = (R.view(np.uint32)[ij] + 1) | SIGN
    only(run(base, above), "mirror_bound_above")

    def off(d, R, ij):
        d["mirror"][ij] = R.view(np.uint32)[ij] - 1
    only(run(base, off), "mirror_exact_differs")


def test_one_centroid_element_one_ulp_off(base):
    def edit(d, R, ij):
        d["centroids"].view(np.uint32)[ij[0], 7] += 1
    only(run(base, edit), "centroid")


def test_one_wrong_size(base):
    def edit(d, R, ij):
        d["sizes"][ij[1]] += 1
    only(run(base, edit), "size")


def test_a_delta2_too_small_for_the_largest_centroid_norm(base):
    """M >= 1.001 x the largest norm in the restatement too, so a lb_delta2 below the largest norm is necessarily also off the restatement by more than
    the margin: both findings, nothing else."""
    E, dump, log, _, _ = base
    cent, _, _ = WFC.replay(E, log)
    top = np.sqrt((cent.astype(np.float64) ** 2).sum(axis=1)).max()

    def edit(d, R, ij):
        d["lb_delta2"] = np.float32(WFC._DELTA2_PER_M * top * 0.9999)
    res = run(base, edit)
    got = {k: v for k, v in res["counts"].items() if v}
    assert set(got) == {"norm_above_M", "delta2_rel"} and got["norm_above_M"] >= 1, got

    def near(d, R, ij):  # a few ulps off the restatement, inside the margin: no finding
        d["lb_delta2"] = np.nextafter(np.nextafter(d["lb_delta2"], np.float32(0)), np.float32(0))
    WFC.assert_clean(run(base, near))


def test_a_g1_one_ulp_low(base):
    def edit(d, R, ij):
        d["lb_g1"] = np.nextafter(np.float32(d["lb_g1"]), np.float32(0))
    only(run(base, edit), "g1")


def test_an_id_reported_unfilled_that_is_not_among_the_youngest(base):
    def edit(d, R, ij):
        assert d["ids"][0] < d["ids"][-1]
        d["row_filled"][0] = False
    res = run(base, edit)
    only(res, "unfilled_not_youngest")
    assert res["left_out"]["unfilled"] > 0

    def youngest(d, R, ij):  # the run's last cluster: allowed, its pairs are left out (here they are all oversize already)
        assert d["ids"][-1] == d["n"] + d["merges"] - 1
        d["row_filled"][-1] = False
    res = run(base, youngest)
    WFC.assert_clean(res)
    assert res["checked"] + res["left_out"]["oversize"] + res["left_out"]["unfilled"] == res["pairs"]


def test_more_unfilled_ids_than_one_step_creates():
    """One merge per step: one cluster at most may lack its row.  (min 1, max 2: every merged cluster stays alive, so the two youngest ids are live.)"""
    E = WC.mog(40, 8, 2)
    dump, log, R, live, sz = oracle_dump(E, 1, 2, rows=WFC.ROWS_SINGLE, complete=False)
    assert live[-1] == 40 + len(log) - 1 and live[-2] == live[-1] - 1
    dump["row_filled"][-2:] = False
    res = WFC.check(E, 1, 2, log, dump)
    got = {k: v for k, v in res["counts"].items() if v}
    assert got == {"unfilled_over_cap": 1}, got


def test_flags_a_mode_cannot_produce_nan_bounds_and_a_wrong_id_list(base):
    E, dump, log, _, _ = base
    ex, log2, R, live, sz = oracle_dump(E, 3, 12, rows=WFC.ROWS_EXACT_BATCH, complete=False)
    m = np.nonzero(np.tril((live[:, None] >= 60) & ((sz[:, None] + sz[None, :]) <= 12), -1))
    i, j = int(m[0][0]), int(m[1][0])
    ex["entries"][i, j] |= SIGN  # a merged cluster's row in exact-rows mode
    got = {k: v for k, v in WFC.check(E, 3, 12, log2, ex)["counts"].items() if v}
    assert got == {"flag_not_allowed": 1}, got

    def nan(d, R, ij):
        d["entries"][ij] = np.uint32(0xFFC00000)
    only(run(base, nan), "nan_entry")

    def ids(d, R, ij):
        d["ids"][0] += 1 if d["ids"][0] + 1 != d["ids"][1] else 2
    only(run(base, ids), "ids")
