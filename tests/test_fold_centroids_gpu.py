"""icl_fold_centroids and its _dev form (imageclust_amd/csrc/fold.hip): the centroid of every cluster given as a member list,
MergeClusters folded over the members in list order.  Bar: every output equals the restatement of tests/fold_cases.py -- floats as
uint32 bit patterns (NaN by isnan), sizes as integers -- for every width and load path, every group length around the kernel's LDS
stage (256) and load batch (8), workgroups of one, two and four waves (enough groups that fold_plan.h keeps them wide), both forms,
NaN / Inf / -0.0 rows and item counts around 2^24.  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest

from tests import fold_cases as FC

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-1234.5)


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    """name -> (E, row_ptr, member, size, the rule's answer), the answers computed once"""
    return {name: (E, rp, mb, sz, FC.fold(E, rp, mb, sz)) for name, E, rp, mb, sz in FC.cases()}


NAMES = [c[0] for c in FC.cases(big=False)] + ["K=70000"] + [w[0] for w in FC.WAVES]


def test_the_cases_reach_workgroups_of_one_two_and_four_waves(ctx, cases):
    """The geometry fold_plan.h chooses on THIS device for the cases below (tests/fold_cases.geometry is the header's rule: the CPU
    suite holds the two against each other): the stage loop's barriers are met by one, two and four waves, in both forms, with and
    without dead lanes in the last chunk."""
    cus = ctx.device_info()[1]
    seen = set()
    for name, K, d, _ in FC.WAVES:
        assert len(cases[name][1]) - 1 == K and cases[name][0].shape[1] == d
        for aligned in (True, False):  # (the _dev test runs these cases 4 bytes off as well: one column per thread at every width)
            vec, threads, chunks = FC.geometry(K, d, aligned, cus)
            if aligned:
                assert threads == (256 if K == 1100 else 128), (name, cus, threads)
            seen.add((vec, threads, chunks * threads * (4 if vec else 1) > d))  # (16-byte form?, threads, dead lanes in the last chunk?)
    assert seen >= {(True, 256, False), (True, 256, True), (False, 256, False), (False, 256, True), (True, 128, False), (True, 128, True),
                    (False, 128, True)}, (cus, seen)
    assert FC.geometry(22, 2048, True, cus)[1] == 64 and FC.geometry(70000, 3, True, cus)[1] == 64  # ... and the other cases one wave


@pytest.mark.parametrize("name", NAMES)
def test_both_forms_equal_the_rule(ctx, cases, name):
    E, rp, mb, sz, want = cases[name]
    for dev in (False, True):
        got = ctx.fold_centroids(E, rp, mb, size=sz, dev=dev)
        assert FC.why(got, want) is None, "%s dev=%s: %s" % (name, dev, FC.why(got, want))
    st = ctx.last_fold_stats()
    K = len(rp) - 1
    assert (st["groups"], st["rows"]) == (K, int(rp[-1])) and st["longest"] == (int(np.diff(rp).max()) if K else 0), st
    assert (st["workspace_bytes"] > 0) == (K > 0), st


def test_one_member_groups_hold_their_rows_bits(ctx, cases):
    E, rp, mb, sz, _ = cases["special rows"]
    C, s = ctx.fold_centroids(E, np.arange(len(E) + 1), np.arange(len(E)))
    assert s.tolist() == [1] * len(E)
    assert FC.why((C, s), (E, s)) is None and np.array_equal(np.signbit(C), np.signbit(E))


def on_device(ctx, E, rp, mb, sz, offset, tail=64):
    """The _dev form with E and C_out `offset` bytes behind their allocations' starts and `tail` sentinel floats behind C_out ->
    (C, size_out, the tail as it is afterwards)."""
    K, d = len(rp) - 1, E.shape[1]
    pe, pc = ctx.malloc(E.nbytes + 32), ctx.malloc((K * d + tail) * 4 + 32)
    try:
        out = np.full(K * d + tail, SENTINEL, np.float32)
        ctx.h2d(pe + offset, E)
        ctx.h2d(pc + offset, out)
        so = ctx.fold_centroids_dev(pe + offset, E.shape[0], d, rp, mb, pc + offset, size=sz)
        ctx.sync()
        ctx.d2h(out, pc + offset)
    finally:
        ctx.free(pe)
        ctx.free(pc)
    return out[:K * d].reshape(K, d), so, out[K * d:]


@pytest.mark.parametrize("name", ["d=8 sized", "d=2048 unsized", "d=2052 sized", "d=1037 unsized", "K=2", "4 waves d=2048", "4 waves d=2052",
                                  "2 waves d=2052", "2 waves d=1037"])
@pytest.mark.parametrize("offset", [0, 4])
def test_dev_pointers_aligned_and_4_bytes_off(ctx, cases, name, offset):
    """offset 4: neither matrix is 16-byte aligned, so the one-column form runs where the width alone would allow 16-byte loads; the
    floats behind K * d stay as they were."""
    E, rp, mb, sz, want = cases[name]
    C, so, tail = on_device(ctx, np.ascontiguousarray(E), rp, mb, sz, offset)
    assert FC.why((C, so), want) is None, FC.why((C, so), want)
    assert (tail == SENTINEL).all()


def raw_host_call(ctx, E, sz, n, d, rp, mb, K, C, so):
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    return ctx.L.icl_fold_centroids(ctx.h, p(E), p(sz), n, d, p(rp), p(mb), K, p(C), p(so))


def test_host_form_leaves_the_tail_alone(ctx, cases):
    for name in ("d=3 sized", "d=2048 sized", "K=300"):
        E, rp, mb, sz, want = cases[name]
        K, d = len(rp) - 1, E.shape[1]
        out, so = np.full(K * d + 64, SENTINEL, np.float32), np.full(K + 8, -7, np.int32)
        assert raw_host_call(ctx, E, sz, E.shape[0], d, rp, mb, K, out, so) == 0
        assert FC.why((out[:K * d].reshape(K, d), so[:K]), want) is None, name
        assert (out[K * d:] == SENTINEL).all() and (so[K:] == -7).all(), name


def test_two_shapes_on_one_context_and_size_out_optional(cases):
    """A fresh context: a small call, a larger one (the workspace grows), the small one again (it stays)."""
    from imageclust_amd import _lib

    c = _lib.Context(0)
    try:
        seen = []
        for name in ("K=1", "one group of 5000", "K=1", "K=0", "d=2052 sized"):
            E, rp, mb, sz, want = cases[name]
            assert FC.why(c.fold_centroids(E, rp, mb, size=sz), want) is None, name
            seen.append(c.last_fold_stats()["workspace_bytes"])
        assert seen[1] > seen[0] and seen[2] == seen[0] and seen[3] == 0
        E, rp, mb, sz, want = cases["K=2"]
        out = np.empty((2, E.shape[1]), np.float32)
        assert raw_host_call(c, E, sz, E.shape[0], E.shape[1], rp, mb, 2, out, None) == 0  # size_out may be NULL
        assert FC.why((out, want[1]), want) is None
    finally:
        c.close()


def test_refusals_write_nothing(ctx):
    from imageclust_amd import _lib

    E = FC.rows(4, 3, np.random.default_rng(0))
    rp, mb, sz = np.array([0, 2, 2, 5], np.int64), np.array([0, 3, 3, 1, 2], np.int32), np.array([1, 2, 3, 4], np.int32)
    i64, i32 = lambda *v: np.array(v, np.int64), lambda *v: np.array(v, np.int32)
    good = dict(E=E, sz=sz, n=4, d=3, rp=rp, mb=mb, K=3)
    bad = [dict(n=-1), dict(K=-1), dict(d=0), dict(rp=None), dict(mb=None), dict(E=None), dict(C=None), dict(rp=i64(1, 2, 2, 5)),
           dict(rp=i64(0, 3, 2, 5)), dict(mb=i32(0, 3, -1, 1, 2)), dict(mb=i32(0, 3, 3, 1, 4)), dict(sz=i32(1, 0, 3, 4)), dict(sz=i32(1, 2, 3, -4)),
           dict(sz=i32(2**31 - 1, 1, 1, 2**31 - 1))]
    for change in bad:
        a = dict(good, **change)
        out, so = np.full(3 * 3 + 16, SENTINEL, np.float32), np.full(3, -7, np.int32)
        rc = raw_host_call(ctx, a["E"], a["sz"], a["n"], a["d"], a["rp"], a["mb"], a["K"], None if "C" in change else out, so)
        assert rc == _lib.ICL_ERR_ARG, (change, rc)
        assert (out == SENTINEL).all() and (so == -7).all(), change
    out, so = np.full(16, SENTINEL, np.float32), np.full(3, -7, np.int32)
    assert raw_host_call(ctx, None, None, 0, 3, None, None, 0, None, None) == 0  # K == 0: nothing is needed, nothing runs
    assert raw_host_call(ctx, E, sz, 4, 3, rp, mb, 3, out, so) == 0 and so.tolist() == [5, 0, 9]  # ... and the accepted call beside them
    assert ctx.L.icl_fold_centroids_dev(ctx.h, None, None, 4, 3, None, None, 3, None, None) == _lib.ICL_ERR_ARG
