"""icl_cluster_many's host side without a GPU: how Context.cluster_many packs its problems (offsets, alignment, image ranges), and
the argument check of the entry point."""
import numpy as np


def test_pack_many_offsets_and_alignment():
    from imageclust_amd import _lib

    rng = np.random.default_rng(0)
    probs = [(rng.standard_normal((n, d)).astype(np.float32), mn, mx) for n, d, mn, mx in
             [(5, 7, 1, 2), (0, 4, 1, 1), (3, 1001, 3, 6), (1, 8, 1, 1), (12, 16, 2, 5), (2, 3, 3, 6)]]
    pk = _lib.pack_many(probs)
    assert pk["E"].dtype == np.float32 and pk["e_off"].dtype == np.int64
    assert list(pk["n"]) == [5, 0, 3, 1, 12, 2] and list(pk["d"]) == [7, 4, 1001, 8, 16, 3]
    assert list(pk["min_size"]) == [1, 1, 3, 1, 2, 3] and list(pk["max_size"]) == [2, 1, 6, 1, 5, 6]
    assert list(pk["img_off"]) == [0, 5, 5, 8, 9, 21, 23]
    assert all(o % 4 == 0 for o in pk["e_off"])  # every problem starts on a 16-byte boundary
    for (E, _, _), o in zip(probs, pk["e_off"]):
        assert np.array_equal(pk["E"][o:o + E.size].reshape(E.shape), E)
    ends = [o + E.size for (E, _, _), o in zip(probs, pk["e_off"])]
    assert all(e <= s for e, s in zip(ends[:-1], pk["e_off"][1:])) and ends[-1] <= pk["E"].size


def test_pack_many_of_nothing():
    from imageclust_amd import _lib

    pk = _lib.pack_many([])
    assert pk["E"].size >= 1 and len(pk["n"]) == 0 and list(pk["img_off"]) == [0]


def test_cluster_many_rejects_a_null_context():
    from imageclust_amd import _lib

    L = _lib.load()
    out = np.full(4, 777, np.int32)
    rc = L.icl_cluster_many(None, 1, out.ctypes.data, 4, np.zeros(1, np.int64).ctypes.data, np.ones(1, np.int32).ctypes.data,
                            np.ones(1, np.int32).ctypes.data, np.ones(1, np.int32).ctypes.data, np.ones(1, np.int32).ctypes.data,
                            out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, None, out.ctypes.data)
    assert rc == _lib.ICL_ERR_ARG and (out == 777).all()
    assert L.icl_cluster_many_dev(None, 0, None, 0, None, None, None, None, None, None, None, None, None, None, None) == _lib.ICL_ERR_ARG
