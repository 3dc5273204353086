"""4:4:0 (luma 1x2) and 4:1:1 (luma 4x1 / 1x4) JPEGs on the batched GPU ingest path (jpeg_gpu.hip, jpeg_huff_gpu.hip): rows, coefficients,
embeddings and a whole clustering request against the host path, in both entropy modes.  The counters are part of every check: equality
alone would also pass if such a file quietly took the host route.  Fixtures: tests/jpeg_sampling_cases.py (the largest is 470x315)."""
import faulthandler

import numpy as np
import pytest

from tests import jpeg_sampling_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.load_synthetic(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return SC.corpus(tmp_path_factory.mktemp("sampling_gpu"))


@pytest.fixture(scope="module")
def paths(cases):
    return [c["path"] for c in cases]


@pytest.fixture(scope="module")
def host_rows(L, paths):
    """icl_load_image_224 of every fixture (computed once, shared, never written to)."""
    rows = np.stack([L.load_image_224(p) for p in paths])
    rows.setflags(write=False)
    return rows


class entropy_gpu:
    def __init__(self, L, ctx):
        self.L, self.ctx = L, ctx

    def __enter__(self):
        self.ctx.set_ingest_options(self.L.ENTROPY_GPU)

    def __exit__(self, *a):
        self.ctx.set_ingest_options(self.L.ENTROPY_HOST)


def test_rows_host_entropy(L, ctx, cases, paths, host_rows):
    got, status = ctx.load_images_224(paths, threads=4)
    assert (status == 0).all(), status
    bad = [p for i, p in enumerate(paths) if not np.array_equal(got[i], host_rows[i])]
    assert not bad, "rows differ from icl_load_image_224: %s" % bad
    ing, ent = ctx.last_ingest_stats(), ctx.last_entropy_stats()
    assert ing["gpu_jpegs"] == len(paths) and ing["host_files"] == 0, ing
    assert ent["gpu_entropy_jpegs"] == 0 and ent["host_entropy_jpegs"] == len(paths) and ent["redone_on_host"] == 0, ent


def test_coefficients_and_rows_gpu_entropy(L, ctx, cases, paths, host_rows):
    nprog = sum(1 for c in cases if c["progressive"])
    assert nprog == 3
    want, wstate = ctx.jpeg_coefs_files(paths, L.ENTROPY_HOST)
    assert (wstate == 1).all()
    got, state = ctx.jpeg_coefs_files(paths, L.ENTROPY_GPU)
    for i, c in enumerate(cases):
        if c["progressive"]:
            assert state[i] == -1, c
            continue
        assert state[i] == 1, "not accepted: %s" % c["path"]
        assert want[i].size == 64 * sum(SC.blocks_of(c)) and np.array_equal(got[i], want[i]), c["path"]
    with entropy_gpu(L, ctx):
        rows, status = ctx.load_images_224(paths, threads=4)
        ing, ent = ctx.last_ingest_stats(), ctx.last_entropy_stats()
    assert (status == 0).all(), status
    bad = [p for i, p in enumerate(paths) if not np.array_equal(rows[i], host_rows[i])]
    assert not bad, "rows differ from icl_load_image_224: %s" % bad
    assert ing["gpu_jpegs"] == len(paths) and ing["host_files"] == 0, ing
    assert ent["gpu_entropy_jpegs"] == len(paths) - nprog and ent["redone_on_host"] == 0 and ent["host_entropy_jpegs"] == nprog, ent
    assert ent["stream_bytes"] > 0


def test_damaged_files_both_modes(L, ctx, cases, paths, tmp_path):
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    try:
        bad = SC.damaged(tmp_path, cases)
        assert len(bad) == 4
        mixed = [paths[0]] + bad + [paths[-1]]
        # what the check must decide, from the host loop over the same subsequences (test_jpeg_sampling_cpu.py)
        state = np.array([L.jpeg_coefs_file_host(p, 1024)[1]["state"] for p in mixed])
        assert (state >= 0).all() and (state == 0).sum() >= 2, state
        want, wstatus = ctx.load_images_224(mixed, threads=3)
        werr = ctx.last_error() if wstatus.any() else None
        assert ctx.last_entropy_stats()["gpu_entropy_jpegs"] == 0
        for i, p in enumerate(mixed):  # the host path alone says the same
            try:
                row, code = L.load_image_224(p), 0
            except L.ICLError as e:
                row, code = np.zeros((224, 224, 3), np.uint8), e.code
            assert code == wstatus[i] and np.array_equal(row, want[i]), p
        with entropy_gpu(L, ctx):
            got, status = ctx.load_images_224(mixed, threads=3)  # the damaged set goes through the GPU once
            gerr = ctx.last_error() if status.any() else None
            ent = ctx.last_entropy_stats()
        assert list(status) == list(wstatus) and np.array_equal(got, want) and gerr == werr
        assert ent["redone_on_host"] == int((state == 0).sum()) and ent["gpu_entropy_jpegs"] == int((state == 1).sum()), (ent, state)
    finally:
        faulthandler.cancel_dump_traceback_later()


@pytest.mark.parametrize("prec", ["PREC_BF16", "PREC_FP32"])
def test_embed_files_equal_embed_u8(L, ctx, cases, host_rows, prec):
    prec = getattr(L, prec)
    pick = [[i for i, c in enumerate(cases) if c["luma"] == luma and max(c["size"]) > 40 and not c["progressive"]][0] for luma in ((1, 2), (4, 1), (1, 4))]
    three = [cases[i]["path"] for i in pick]
    ref = ctx.embed_u8(host_rows[pick], L.HEAD_POOLED, prec)
    E, status = ctx.embed_files(three, L.HEAD_POOLED, prec, 2)
    assert (status == 0).all() and np.array_equal(E.view(np.uint32), ref.view(np.uint32))
    assert ctx.last_ingest_stats()["gpu_jpegs"] == 3 and ctx.last_ingest_stats()["host_files"] == 0
    with entropy_gpu(L, ctx):
        E, status = ctx.embed_files(three, L.HEAD_POOLED, prec, 2)
        ent = ctx.last_entropy_stats()
    assert (status == 0).all() and np.array_equal(E.view(np.uint32), ref.view(np.uint32))
    assert ent["gpu_entropy_jpegs"] == 3 and ent["redone_on_host"] == 0, ent


def test_a_request_with_rotated_uploads(L, ctx, cases, tmp_path):
    """One request of 8 images, one of them 4:4:0 and one 4:1:1 (what a losslessly rotated 4:2:2 photo and a DV still are): it clusters,
    and equals embed_files -> host combine -> cluster_many on the same paths."""
    from tests.test_requests_gpu import composition, same_as_composition, save_jpeg

    plain = [save_jpeg(tmp_path / ("f%d.jpg" % i), w, h, 700 + i, quality=80, subsampling=i % 3) for i, (w, h) in enumerate([(37, 53), (17, 9), (31, 8), (16, 24), (8, 8), (41, 50)])]
    v2 = [c["path"] for c in cases if c["luma"] == (1, 2) and c["orient"] == 6][0]
    h4 = [c["path"] for c in cases if c["luma"] == (4, 1) and c["size"] == (45, 59) and c["orient"] == 1][0]
    ps = plain[:2] + [v2] + plain[2:5] + [h4] + plain[5:]
    labels = [[i % 3] for i in range(8)]
    reqs = [(ps, labels, 3, 2, 4)]
    got = ctx.cluster_requests(reqs, L.HEAD_DENSE0, L.PREC_FP32, threads=4, want_merges=True, want_E=True)
    assert ctx.last_requests_rc == L.ICL_OK and (ctx.last_file_status == 0).all(), ctx.last_error()
    ing = ctx.last_ingest_stats()
    assert ing["gpu_jpegs"] == 8 and ing["host_files"] == 0, ing
    cid, rank, nc, status = got[0][:4]
    assert status == 0 and nc >= 2 and (cid >= 0).all()
    Es, res, fst = composition(ctx, L, reqs, L.HEAD_DENSE0, L.PREC_FP32)
    assert (fst == 0).all()
    same_as_composition(got, Es, res, "request with 4:4:0 and 4:1:1 files")
