"""The four grow-only workspaces a context keeps between calls (icl_pairs_within, icl_nearest, icl_cluster_many, icl_cluster_requests:
one icl_dev_grow each) across a small call, a call that forces the buffer to grow, and the small call again on ONE context.  Every
result is bit-equal (np.array_equal) to the same call on a context that has never made such a call, the pairs and nearest results also
to the host rule (*_from_matrix) on the exact distance matrix, and the workspace sizes the statistics report are the fresh context's:
a buffer that is larger than a call needs, or was replaced since the last call, changes nothing.
Shapes: n = 130 and n = 700 rows of d = 8 (two and six tile rows); 3 and 44 problems of 150 to 250 rows (the large call's triangles
hold about 3.5 MB, above the workspace's 1 MiB floor); 8 images with the 1000-wide head and 3 x 30 images with the 2048-wide one (about
1.5 MB of rows)."""
import io

import numpy as np
import pytest
from PIL import Image

from tests.jpeg_entropy_cases import picture

pytestmark = pytest.mark.gpu

D = 8
SIZES = {"small": 130, "large": 700}


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


def rows(n, seed):
    """n rows of D floats in a few loose groups, so that a threshold picks a moderate share of the pairs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)) + 3.0 * rng.integers(0, 6, (n, 1))).astype(np.float32)


def sizes(n, seed):
    return np.random.default_rng(seed + 1000).integers(1, 9, n).astype(np.int32)


def fresh(L, call, model=False):
    """call(ctx) on a context of its own."""
    c = L.Context(0)
    try:
        if model:
            c.load_synthetic(1)
        return call(c)
    finally:
        c.close()


def same(a, b):
    """Bit-equality of nested tuples / lists of arrays and scalars."""
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a == b


@pytest.fixture(scope="module")
def exact(L):
    """size name -> (E, size, the exact Ward distance matrix), computed once on a context of its own."""
    def run(c):
        out = {}
        for name, n in SIZES.items():
            E, sz = rows(n, n), sizes(n, n)
            out[name] = (E, sz, c.ward_distance_matrix(E, sz))
        return out

    return fresh(L, run)


@pytest.fixture
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def test_pairs_workspace(L, ctx, exact):
    def call(name):
        E, sz, Dm = exact[name]
        thr = float(np.quantile(Dm[np.tril_indices(len(E), -1)], 0.02))
        return lambda c: (c.pairs_within(E, thr, sz), c.last_pairs_stats()), L.pairs_within_from_matrix(Dm, thr)

    for name in ("small", "large", "small"):
        run, host = call(name)
        (got, stats), (want, wstats) = run(ctx), fresh(L, run)
        assert len(got[1]) > 0 and same(got, want), name
        assert same(got, host), name
        assert stats["workspace_bytes"] == wstats["workspace_bytes"] > 0 and stats == wstats, (name, stats, wstats)


def test_nearest_workspace(L, ctx, exact):
    K = 5

    def call(name):
        E, sz, Dm = exact[name]
        ex = np.arange(len(E))

        def run(c):
            c.set_nearest_options(2)  # two column splits: the partial lists live in the workspace
            return c.nearest(E, E, K, q_size=sz, e_size=sz, max_size=12, exclude=ex), c.last_nearest_stats()

        return run, L.nearest_from_matrix(Dm, K, q_size=sz, e_size=sz, max_size=12, exclude=ex)

    for name in ("small", "large", "small"):
        run, host = call(name)
        (got, stats), (want, wstats) = run(ctx), fresh(L, run)
        assert same(got, want), name
        assert same(got, host), name
        assert stats["splits"] == 2 and stats["workspace_bytes"] == wstats["workspace_bytes"] > 0 and stats == wstats, (name, stats, wstats)


def many_problems(count, seed):
    rng = np.random.default_rng(seed)
    return [(rows(int(n), seed + i), 3, 12) for i, n in enumerate(rng.integers(150, 251, count))]


def test_many_workspace(L, ctx):
    calls = {"small": many_problems(3, 1), "large": many_problems(44, 2)}  # 44 triangles of about 80 KB: above the 1 MiB floor
    for name in ("small", "large", "small"):
        run = lambda c: (c.cluster_many(calls[name], want_merges=True), c.last_many_stats())
        (got, stats), (want, wstats) = run(ctx), fresh(L, run)
        assert all(r[3] in (L.ICL_OK, L.ICL_ERR_CONSTRAINT) for r in got) and any(r[3] == L.ICL_OK for r in got), name
        assert same(got, want) and stats == wstats, name


def jpeg(seed):
    buf = io.BytesIO()
    Image.fromarray(picture(64, 48, seed)).save(buf, "JPEG", quality=85)
    return buf.getvalue()


def requests_of(bufs, per, nl, seed):
    rng = np.random.default_rng(seed)
    reqs = []
    for at in range(0, len(bufs), per):
        labels = [sorted(int(j) for j in rng.integers(0, nl, 2)) for _ in range(per)]
        reqs.append((bufs[at:at + per], labels, nl, 3, 6))
    return reqs


def test_requests_workspace(L):
    bufs = [jpeg(300 + i) for i in range(90)]
    # 8 rows of 1000 + 3 floats; then 90 rows of 2048 + 5 floats beside their 2048 dense floats: about 1.5 MB, above the 1 MiB floor
    calls = {"small": (requests_of(bufs[:8], 8, 3, 5), L.HEAD_DENSE0), "large": (requests_of(bufs, 30, 5, 6), L.HEAD_POOLED)}
    ctx = L.Context(0)
    try:
        ctx.load_synthetic(1)
        want = {}
        for name in ("small", "large", "small"):
            reqs, head = calls[name]
            run = lambda c: (c.cluster_requests_mem(reqs, head, L.PREC_FP32, 4, want_merges=True, want_E=True), c.last_file_status, c.last_requests_rc)
            if name not in want:
                want[name] = fresh(L, run, model=True)
            got = run(ctx)
            assert all(r[3] in (L.ICL_OK, L.ICL_ERR_CONSTRAINT) for r in got[0]) and any(r[3] == L.ICL_OK for r in got[0]), (name, got[2])
            assert same(got, want[name]), name
    finally:
        ctx.close()
