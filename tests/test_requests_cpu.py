"""Host-only parts of icl_cluster_requests (imageclust_amd/csrc/requests.hip): the layout of the combined rows, the packing of the
per-image label lists, and workflow.RunRequests' label mapping.  No GPU."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    _lib.load()
    return _lib


def layout_numpy(n, n_labels, head):
    n, n_labels = np.asarray(n, np.int64), np.asarray(n_labels, np.int64)
    d = head + n_labels
    e_off = np.concatenate([[0], np.cumsum(n * d)])
    return e_off[:-1], d, int(e_off[-1])


@pytest.mark.parametrize("head", [1000, 2048])
def test_layout_equals_numpy(L, head):
    rng = np.random.default_rng(5)
    n = rng.integers(0, 70, 200).astype(np.int32)
    nl = rng.integers(0, 201, 200).astype(np.int32)
    n[[0, 17, 199]] = 0  # requests without images
    nl[[1, 17, 100]] = 0  # requests without labels
    e_off, d, e_len = L.requests_layout(n, nl, head)
    we, wd, wl = layout_numpy(n, nl, head)
    assert e_off.dtype == np.int64 and d.dtype == np.int32
    assert np.array_equal(e_off, we) and np.array_equal(d, wd) and e_len == wl
    assert (d % 2 == 0).any() and (d % 2 == 1).any()


def test_layout_is_64_bit_and_checks_its_arguments(L):
    # 3 requests of 2^20 images and 2048 + 2^20 columns: offsets far beyond 2^31 floats
    n = np.full(3, 1 << 20, np.int32)
    nl = np.full(3, 1 << 20, np.int32)
    e_off, d, e_len = L.requests_layout(n, nl, 2048)
    we, wd, wl = layout_numpy(n, nl, 2048)
    assert np.array_equal(e_off, we) and np.array_equal(d, wd) and e_len == wl and e_len > 1 << 41
    assert L.requests_layout([], [], 1000)[2] == 0

    lib = L.load()
    n = np.array([3, 4], np.int32)
    nl = np.array([5, 0], np.int32)
    ptr = lambda a: a.ctypes.data
    e_len = C.c_int64(-7)
    assert lib.icl_requests_layout(2, ptr(n), ptr(nl), 1000, None, None, C.byref(e_len)) == 0 and e_len.value == 3 * 1005 + 4 * 1000
    assert lib.icl_requests_layout(2, ptr(n), ptr(nl), 1000, None, None, None) == 0  # every output may be NULL
    outs = [np.full(2, 777, np.int64), np.full(2, 777, np.int32)]
    e_len = C.c_int64(777)

    def bad(nreq=2, n_=n, nl_=nl, head=1000):
        rc = lib.icl_requests_layout(nreq, ptr(n_) if n_ is not None else None, ptr(nl_) if nl_ is not None else None, head, ptr(outs[0]),
                                     ptr(outs[1]), C.byref(e_len))
        return rc, all((o == 777).all() for o in outs) and e_len.value == 777

    assert bad(nreq=-1) == (L.ICL_ERR_ARG, True)
    assert bad(n_=None) == (L.ICL_ERR_ARG, True)
    assert bad(nl_=None) == (L.ICL_ERR_ARG, True)
    assert bad(n_=np.array([3, -1], np.int32)) == (L.ICL_ERR_ARG, True)
    assert bad(nl_=np.array([5, -2], np.int32)) == (L.ICL_ERR_ARG, True)
    assert bad(head=-1) == (L.ICL_ERR_ARG, True)
    assert bad(nl_=np.array([5, 2**31 - 1], np.int32)) == (L.ICL_ERR_ARG, True)  # head + n_labels beyond int32
    assert bad() == (0, False)
    with pytest.raises(L.ICLError):
        L.requests_layout([1, -1], [0, 0], 1000)


def test_pack_requests(L):
    reqs = [(["a", "b", "c"], [[0, 2], [], [1, 1, -1]], 3, 3, 6),  # an image without labels, a duplicate, an unknown label
            ([], [], 4, 3, 6),                                    # a request without images
            (["d"], [[]], 0, 1, 1)]                               # a request without labels
    pk = L.pack_requests(reqs, 1000)
    assert pk["paths"] == ["a", "b", "c", "d"]
    assert pk["n"].tolist() == [3, 0, 1] and pk["n_labels"].tolist() == [3, 4, 0]
    assert pk["label_off"].tolist() == [0, 2, 2, 5, 5] and pk["label_off"].dtype == np.int64
    assert pk["label_idx"].tolist() == [0, 2, 1, 1, -1] and pk["label_idx"].dtype == np.int32
    assert pk["min_size"].tolist() == [3, 3, 1] and pk["max_size"].tolist() == [6, 6, 1]
    assert pk["img_off"].tolist() == [0, 3, 3, 4]
    assert pk["d"].tolist() == [1003, 1004, 1000] and pk["e_off"].tolist() == [0, 3009, 3009] and pk["e_len"] == 4009
    empty = L.pack_requests([], 2048)
    assert empty["n"].size == 0 and empty["label_off"].tolist() == [0] and empty["e_len"] == 0
    with pytest.raises(ValueError):
        L.pack_requests([(["a"], [[3]], 3, 3, 6)])  # a column outside the label set
    with pytest.raises(ValueError):
        L.pack_requests([(["a"], [[-2]], 3, 3, 6)])
    with pytest.raises(ValueError):
        L.pack_requests([(["a", "b"], [[0]], 3, 3, 6)])  # one label list per path


def test_run_requests_label_mapping(L):
    from imageclust_amd import embeddings, workflow

    labelSet = {"cat": 0, "dog": 1, "tree": 2, "car": 3}
    assert workflow.LabelIndices(["dog", "cat"], labelSet) == [1, 0]
    assert workflow.LabelIndices(["bird", "car", "car"], labelSet) == [-1, 3, 3]  # absent from the set: -1
    assert workflow.LabelIndices([], labelSet) == []
    reqs = [(["p0", "p1"], ["id0", "id1"], [["dog", "bird"], []], labelSet, 3, 6), (["q"], ["idq"], [["x"]], {}, 1, 2)]
    packed = workflow.PackRequests(reqs)
    assert packed == [(["p0", "p1"], [[1, -1], []], 4, 3, 6), (["q"], [[-1]], 0, 1, 2)]
    pk = L.pack_requests(packed, 1000)
    assert pk["label_idx"].tolist() == [1, -1, -1] and pk["label_off"].tolist() == [0, 2, 2, 3] and pk["d"].tolist() == [1004, 1000]
    # the columns the engine sets are those GenerateLabelVector sets
    for labels in (["dog", "bird"], ["tree", "tree", "cat"], []):
        v = np.zeros(len(labelSet), np.float32)
        for j in workflow.LabelIndices(labels, labelSet):
            if j >= 0:
                v[j] = 1.0
        assert np.array_equal(v, embeddings.GenerateLabelVector(labels, labelSet))
    with pytest.raises(ValueError):
        workflow.PackRequests([(["p0"], ["id0", "id1"], [[]], labelSet, 3, 6)])
    with pytest.raises(L.ICLError) as ei:
        workflow.RunRequests(embeddings.AppContext(), reqs)  # no Net: an error, never a host fallback
    assert ei.value.code == L.ICL_ERR_NOMODEL
