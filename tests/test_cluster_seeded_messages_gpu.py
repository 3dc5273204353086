"""The two seeded engines refuse and accept the same problems in the same words: icl_cluster_seeded (ward.hip) and
icl_cluster_many_seeded (ward_many.hip) take status, k and the sizes their kernels see from one rule (ward_seed_admit, ward_seeds.h) and
put only their own prefix in front of its reason.  m = 5 seeds, d = 3: three refused problems and one accepted problem with nothing to
merge, each given to icl_cluster_seeded and, alone, to icl_cluster_many_seeded, on the host and on the device.  The expected texts are
literals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, D = 5, 3
MANY_PREFIX = "icl_cluster_many_seeded: problem 0: "
# (seed sizes, min_size, max_size, k_target, status name, the prefix icl_cluster_seeded puts in front, the reason)
REFUSED = [
    ([2, -9, 1, 7, 8], 1, 6, 0, "ICL_ERR_UNSUPPORTED", "icl_cluster_seeded: ", "seed 3 holds 7 items, above maxSize (6), and is not frozen"),
    ([1, 1, 1, 1, 1], 4, 4, 0, "ICL_ERR_CONSTRAINT", "",
     "cannot satisfy cluster size constraints with total items (5), minSize (4), and maxSize (4)"),
    ([1 << 29, -((1 << 29) - 3), 1, 1, 1], 1, 1 << 30, 2, "ICL_ERR_UNSUPPORTED", "icl_cluster_seeded: ", "1073741824 items in all"),
]
ACCEPTED = ([2, -3, 1, 4, 2], 1, 6, M)  # k_target = m: no merge is asked for


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def C():
    return np.random.default_rng(30).standard_normal((M, D)).astype(np.float32)


@pytest.mark.parametrize("dev", [False, True])
def test_refusals_are_the_same_words(ctx, C, dev):
    from imageclust_amd import _lib

    for sizes, mn, mx, kt, code, prefix, text in REFUSED:
        cid, rank, nc, st, log, co = ctx.cluster_seeded(C, sizes, mn, mx, kt, dev=dev)
        one = ctx.last_error()
        (mcid, mrank, mnc, mst, mlog, mco), = ctx.cluster_many_seeded([(C, sizes, mn, mx, kt)], want_merges=True, want_centroids=True, dev=dev)
        many = ctx.last_error()
        print("%s | %s" % (one, many))
        assert st == mst == getattr(_lib, code), (text, st, mst)
        assert one == prefix + text and many == MANY_PREFIX + text, (one, many)
        assert one[len(prefix):] == many[len(MANY_PREFIX):]
        for ids in (cid, rank, mcid, mrank):
            assert ids.tolist() == [-1] * M, text
        assert nc == mnc == 0 and len(log) == len(mlog) == 0, text
        for out in (co, mco):
            assert out.shape == (M, D) and not out.view(np.uint32).any(), text


@pytest.mark.parametrize("dev", [False, True])
def test_nothing_to_merge_is_accepted_by_both(ctx, C, dev):
    sizes, mn, mx, kt = ACCEPTED
    cid, rank, nc, st, log, co = ctx.cluster_seeded(C, sizes, mn, mx, kt, dev=dev)
    (mcid, mrank, mnc, mst, mlog, mco), = ctx.cluster_many_seeded([(C, sizes, mn, mx, kt)], want_merges=True, want_centroids=True, dev=dev)
    assert st == mst == 0 and nc == mnc == M
    for ids, ranks in ((cid, rank), (mcid, mrank)):
        assert ids.tolist() == list(range(M)) and ranks.tolist() == [0] * M  # every seed its own cluster, in seed order
    assert len(log) == len(mlog) == 0 and ctx.last_many_stats() == {"small": 0, "mid": 0, "large": 0, "mid_groups": 0}
    for out in (co, mco):
        assert np.array_equal(out.view(np.uint32), C.view(np.uint32))
