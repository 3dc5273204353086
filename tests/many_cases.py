"""What the icl_cluster_many tests share (test_cluster_many_gpu.py, test_cluster_many_mid_gpu.py and their child processes):
serving-shape problems and the three comparisons of a result (cluster_id, member_rank, n_clusters, status, merge log) --
against the CPU oracle, against icl_cluster on the problem alone, against another result."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as O


def serving_problems(count, seed, n_lo=2, n_hi=256, dup_every=0):
    """The reference's request shape (workflow.Run): n images, d = 1000 dense0 columns + L one-hot label columns, min 3 / max 6.
    Every other problem has an odd d; every dup_every-th problem is one row repeated."""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(count):
        n = int(rng.integers(n_lo, n_hi + 1))
        L = int(rng.integers(0, 201))
        if (1000 + L) % 2 != p % 2:
            L = L + 1 if L < 200 else L - 1
        d = 1000 + L
        dense = np.abs(rng.standard_normal((1, 1000))).astype(np.float32) + 0.3 * rng.standard_normal((n, 1000)).astype(np.float32)
        lab = np.zeros((n, L), np.float32)
        if L:
            lab[np.arange(n), rng.integers(0, L, n)] = 1.0
        E = np.concatenate([dense, lab], axis=1).astype(np.float32)
        if dup_every and p % dup_every == dup_every - 1:
            E[:] = E[0]
        out.append((np.ascontiguousarray(E), 3, 6))
    return out


def oracles(probs):
    with ThreadPoolExecutor(16) as ex:  # (the oracle's C call releases the GIL)
        return list(ex.map(lambda pr: O.cluster_fast(pr[0], pr[1], pr[2], want_log=True), probs))


def same_as_oracle(r, ref, what):
    cid, rank, nc, st, log = r
    if not ref["ok"]:
        from imageclust_amd import _lib

        assert st == _lib.ICL_ERR_CONSTRAINT, what
        assert (cid == -1).all() and (rank == -1).all() and nc == 0 and len(log) == 0, what
        return
    assert st == 0, what
    assert np.array_equal(cid, ref["cluster_id"]) and np.array_equal(rank, ref["member_rank"]) and nc == ref["n_clusters"], what
    assert np.array_equal(log, ref["log"][:, 2:4].astype(np.int32)), what


def same_as_cluster(ctx, pr, r, what):
    """r equals icl_cluster on the problem alone; a problem icl_cluster fails has that error code as its status."""
    from imageclust_amd import _lib

    try:
        cid, rank, nc = ctx.cluster(pr[0], pr[1], pr[2])
    except _lib.ICLError as e:
        assert e.code == r[3], what
        return
    assert r[3] == 0 and np.array_equal(cid, r[0]) and np.array_equal(rank, r[1]) and nc == r[2], what
    assert np.array_equal(ctx.last_merges(), r[4]), what


def same_results(a, b, what):
    for x, y in zip(a, b):
        assert np.array_equal(x, y), what


def not_as_oracle(probs, res, refs, names=None):
    """For a child process: the names (or indices) of the problems whose result is not the oracle's."""
    bad = []
    for p, (r, ref) in enumerate(zip(res, refs)):
        try:
            same_as_oracle(r, ref, p)
        except AssertionError:
            bad.append(names[p] if names else p)
    return bad


def ward_reports(ctx):
    """Every report of the last icl_cluster: merges, merge values, icl_last_ward_stats, _layout, _mode, _bound_violations."""
    stats = (C.c_int64 * 4)()
    assert ctx.L.icl_last_ward_stats(ctx.h, C.byref(stats, 0), C.byref(stats, 8), C.byref(stats, 16), C.byref(stats, 24)) == 0
    return (ctx.last_merges(), ctx.last_merge_values(), list(stats), tuple(ctx.last_ward_layout()), tuple(ctx.last_ward_mode()),
            ctx.last_ward_bound_violations())


def same_reports(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2:] == b[2:], (a[2:], b[2:])
