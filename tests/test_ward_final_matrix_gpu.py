"""Every entry of the matrix the Ward merge loop leaves behind, against the oracle (imageclust_amd/csrc/ward.hip: ward_update_lb_kernel / ward_lb_value,
ward_update_batch2_kernel; include/imageclust.h icl_ward_dump_pairs_dev; checker: tests/ward_final_check.py).

The parity tests of test_ward_gpu.py see one entry per merge -- the pair that won -- and icl_last_ward_bound_violations only the entries a scan happened
to make exact.  Here each case clusters, asserts the result equal to ward_fast.c's (ids, member order, merge log, every merge value), dumps the pairs of
ALL clusters alive at the end and checks every stored entry on the host: a flagged entry (Lance-Williams or matrix-core lower bound) must not exceed
the oracle's WardDistance of the pair, an unflagged one must equal it bit for bit, in the mirror half of the complete-rows layout too; sizes and
centroids must equal the replay of the log; lb_g1 must equal the restatement's, lb_delta2 must agree with it within the error of the fp32 norms, and M
must bound the norm of every centroid the run ever made.

Shapes: the smallest at which the kernels can still go wrong (tests/ward_cases.py and the seeded inputs of test_ward_gpu.py); auto mode from n = 4096,
where production takes the bound-rows loop.  The CPU oracle takes ~1 s for the largest case."""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests import ward_cases as WC
from tests import ward_final_check as WFC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.set_ward_options(0)
    c.close()


def _ulps_apart():
    rng = np.random.default_rng(7)  # (test_lw_bound_cpu: the same construction)
    base = (100.0 + rng.standard_normal((1, 64))).astype(np.float32)
    return (base * (1 + 1e-7 * rng.integers(-3, 4, (30, 64)))).astype(np.float32)


# name -> (E, min, max, Gaussian mixture with bounds that must not all vanish)
def _inputs():
    out = {
        "mog_600x2048_5_50": (lambda: WC.mog(600, 2048, 11), 5, 50, True),         # g at the largest D
        "mog_1500x64_1_1000": (lambda: WC.mog(1500, 64, 12), 1, 1000, True),        # stops at ~n/2 clusters: many generations, mixed sizes
        "mog_1500x64_3_6": (lambda: WC.mog(1500, 64, 12), 3, 6, True),              # most pairs oversize
        "mog_1000x8_1_2": (lambda: WC.mog(1000, 8, 13), 1, 2, True),                # singleton merges only, 3n/4 clusters alive
        "mog_1200x64_plus100_5_50": (lambda: (WC.mog(1200, 64, 14) + 100.0).astype(np.float32), 5, 50, True),  # the Delta term decides
        "ulps_apart_near_100_5_50": (_ulps_apart, 5, 50, False),                    # bounds must come out 0
        "grid_600x8_1_600": (lambda: WC.ties(600, 8, 3, levels=3), 1, 600, False),  # ties and duplicates
        "grid_600x8_2_12": (lambda: WC.ties(600, 8, 3, levels=3), 2, 12, False),
        "cauchy_1000x128_5_50": (lambda: np.random.default_rng(21).standard_cauchy((1000, 128)).astype(np.float32), 5, 50, False),  # the constants' scale
        "mog_500x32_scale_1e-20": (lambda: (WC.mog(500, 32, 15).astype(np.float64) * 1e-20).astype(np.float32), 5, 50, False),  # the "no claim" clamps
        "mog_500x32_scale_1e15": (lambda: (WC.mog(500, 32, 15).astype(np.float64) * 1e15).astype(np.float32), 5, 50, False),
    }
    for n, mn, mx in [(100, 1, 1), (100, 1, 2), (101, 1, 2), (37, 1, 3), (64, 5, 64)]:  # test_batch_target_reached_inside_a_batch: rolled-back picks
        out["target_%d_%d_%d" % (n, mn, mx)] = (lambda n=n: WC.mog(n, 16, n), mn, mx, False)
    for mn, mx in [(1, 240), (2, 4), (3, 8), (1, 2)]:
        out["quads_%d_%d" % (mn, mx)] = (WC.quadruples, mn, mx, False)
    return out


INPUTS = _inputs()
AUTO = {
    "mog_4200x16_5_50": (lambda: WC.mog(4200, 16, 16), 5, 50, True),
    "mog_4608x256_1_1000": (lambda: WC.mog(4608, 256, 17), 1, 1000, True),
}
_cache = {}


def reference(name):
    """(E, min, max, mixture, ward_fast.c's result): computed once per input, shared by the modes, never written to"""
    if name not in _cache:
        make, mn, mx, mixture = (INPUTS.get(name) or AUTO[name])
        E = np.ascontiguousarray(make(), np.float32)
        f = O.cluster_fast(E, mn, mx, lazy_ban=False)
        assert f["ok"]
        E.setflags(write=False)
        _cache[name] = (E, mn, mx, mixture, f)
    return _cache[name]


def run_and_check(ctx, name, what, want_rows, want_complete):
    from imageclust_amd import _lib

    E, mn, mx, mixture, f = reference(name)
    n, d = E.shape
    cid, rank, nc = ctx.cluster(E, mn, mx)
    m = ctx.last_merges()
    vals = ctx.last_merge_values()
    viol = ctx.last_ward_bound_violations()
    mode, layout = ctx.last_ward_mode(), ctx.last_ward_layout()
    alive = np.ones(n + len(m), bool)  # who is alive: from the ENGINE's log alone
    alive[m.reshape(-1)] = False
    live = np.nonzero(alive)[0]
    dump = ctx.ward_dump_pairs(live, d)
    dump["init_bounds"] = mode[1]
    res = WFC.check(E, mn, mx, m, dump)
    line = {"case": name, "run": what, "n": n, "d": d, "min": mn, "max": mx, "live": len(live), "row_mode": dump["row_mode"], "complete_rows": dump["complete_rows"],
            "int8_bounds": layout[2], "violations": {k: v for k, v in res["counts"].items() if v}, "scan_violations": viol}
    line.update({k: res.get(k) for k in ("pairs", "checked", "left_out", "flagged", "flagged_nonzero", "merged_pairs", "flagged_nonzero_merged", "gap", "delta2", "M", "max_norm")})
    if res.get("merged_pairs"):
        line["flagged_fraction_merged"] = res["flagged_nonzero_merged"] / res["merged_pairs"]
    print("R20 " + json.dumps(line))
    # ---- the clustering itself: as same_as_fast_oracle (tests/test_ward_gpu.py)
    assert mode[0] == want_rows, "%s: the loop that ran (%s) is not the one this case is about" % (what, mode)
    assert dump["row_mode"] == want_rows and dump["complete_rows"] == want_complete == layout[0], (what, dump["row_mode"], dump["complete_rows"], layout)
    assert len(m) == f["merges"], "number of merges"
    want = f["log"][:, 2:4].astype(np.int32)
    if not np.array_equal(m, want):
        t = int(np.nonzero((m != want).any(axis=1))[0][0])
        raise AssertionError("merge sequence differs first at merge %d: engine %s, oracle %s" % (t, m[t].tolist(), want[t].tolist()))
    assert np.array_equal(vals.view(np.uint32), f["vals"].view(np.uint32)), "Ward values of the merged pairs"
    assert np.array_equal(cid, f["cluster_id"]) and np.array_equal(rank, f["member_rank"]) and nc == f["n_clusters"]
    assert viol == 0, "a row scan found an exact value below the lower bound it replaced"
    # ---- the matrix
    assert (dump["n"], dump["d"], dump["merges"], dump["max_size"]) == (n, d, len(m), mx)
    WFC.assert_clean(res, "%s, %s" % (name, what))
    L = len(live)
    assert res["pairs"] == L * (L - 1) // 2 == res["checked"] + res["left_out"]["oversize"] + res["left_out"]["unfilled"]
    assert dump["row_filled"].all(), "every loop ends with the rows of all committed clusters written (ward.hip, icl_ward_dump_pairs_dev)"
    if mixture and want_rows == _lib.ROWS_LW_BOUND:
        if res["merged_pairs"]:  # without flagged non-zero entries in merged clusters' rows the bound check would be vacuous
            assert res["flagged_nonzero_merged"] > 0, "no Lance-Williams bound left to check"
        else:  # (max_size 2: a merged cluster has size 2 and every pair with it is oversize -- no row of a merged cluster holds an entry)
            assert mx == 2 and res["flagged_nonzero"] > 0
    return res


@pytest.mark.parametrize("run", ["bound_rows_complete", "bound_rows_recycled", "exact_rows"])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_forced_modes_every_entry_of_the_final_matrix(ctx, monkeypatch, name, run):
    from imageclust_amd import _lib

    monkeypatch.setenv("ICL_WARD_WIDE", "0" if run == "bound_rows_recycled" else "1")
    ctx.set_ward_options(2 if run == "exact_rows" else 4)
    try:
        run_and_check(ctx, name, run, _lib.ROWS_EXACT_BATCH if run == "exact_rows" else _lib.ROWS_LW_BOUND, run == "bound_rows_complete")
    finally:
        ctx.set_ward_options(0)


@pytest.mark.parametrize("name,i8,wide", [("mog_4200x16_5_50", "1", "1"), ("mog_4200x16_5_50", "1", "0"), ("mog_4200x16_5_50", "0", "1"),
                                          ("mog_4200x16_5_50", "0", "0"), ("mog_4608x256_1_1000", "1", "1")])
def test_auto_mode_every_entry_of_the_final_matrix(ctx, monkeypatch, name, i8, wide):
    """What production runs (ICL_DIST_AUTO, n >= 4096): bounds of the initial matrix from the integer GEMM / the f32 GEMM, both layouts."""
    from imageclust_amd import _lib

    monkeypatch.setenv("ICL_WARD_WIDE", wide)
    monkeypatch.setenv("ICL_DIST_I8", i8)
    ctx.set_ward_options(0)
    run_and_check(ctx, name, "auto_i8=%s_wide=%s" % (i8, wide), _lib.ROWS_LW_BOUND, wide == "1")
    assert ctx.last_ward_layout()[2] == (i8 == "1")


def test_dump_refuses_what_it_does_not_cover(ctx):
    from imageclust_amd import _lib

    E = WC.mog(64, 8, 1)
    c2 = _lib.Context(0)
    try:
        with pytest.raises(_lib.ICLError) as ei:
            c2.ward_dump_pairs(np.arange(4), 8)  # no call yet
        assert ei.value.code == _lib.ICL_ERR_ARG
        c2.cluster(E, 2, 6)
        assert c2.ward_dump_pairs(np.arange(4), 8)["row_mode"] == _lib.ROWS_EXACT_BATCH
        for bad_ids, d in [([0, 64 + len(c2.last_merges())], 8), ([-1], 8), ([0, 1], 12)]:
            with pytest.raises(_lib.ICLError) as ei:
                c2.ward_dump_pairs(np.array(bad_ids), d)
            assert ei.value.code == _lib.ICL_ERR_ARG
        c2.distance_bounds_check(WC.mog(64, 8, 2), 1)  # re-initialises the workspace's tables
        with pytest.raises(_lib.ICLError) as ei:
            c2.ward_dump_pairs(np.arange(4), 8)
        assert ei.value.code == _lib.ICL_ERR_ARG
        c2.cluster(E, 2, 6, _lib.UPDATE_LW)  # FAST mode
        with pytest.raises(_lib.ICLError) as ei:
            c2.ward_dump_pairs(np.arange(4), 8)
        assert ei.value.code == _lib.ICL_ERR_UNSUPPORTED
    finally:
        c2.close()
