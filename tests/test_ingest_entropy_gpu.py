"""ICL_ENTROPY_GPU (jpeg_huff_gpu.hip): the Huffman decoder of qualifying baseline JPEGs on the GPU, against host stage A and the host path.
Coefficients, rows, embeddings, status codes and messages must equal the host mode's; the statistics show that the GPU decoder ran and
accepted every clean qualifying file (equality alone would also pass with a fallback)."""
import faulthandler

import numpy as np
import pytest
from PIL import Image

from tests.jpeg_entropy_cases import corpus, damaged, is_progressive, picture, save_jpeg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.load_synthetic(1)
    c.set_ingest_options(L.ENTROPY_GPU)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return corpus(tmp_path_factory.mktemp("entropy_gpu"))


def host_rows(L, paths):
    return np.stack([L.load_image_224(p) for p in paths])


def test_coefficients_equal_stage_a_and_all_accepted(L, ctx, files):
    got, state = ctx.jpeg_coefs_files(files, L.ENTROPY_GPU)
    want, wstate = ctx.jpeg_coefs_files(files, L.ENTROPY_HOST)
    assert (wstate == 1).all()
    for i, p in enumerate(files):
        if is_progressive(p):
            assert state[i] == -1, p
            continue
        assert state[i] == 1, "not accepted: %s" % p
        assert np.array_equal(got[i], want[i]), p


def test_rows_and_stats(L, ctx, files):
    want = host_rows(L, files)
    got, status = ctx.load_images_224(files, threads=8)
    assert (status == 0).all()
    bad = [files[i] for i in range(len(files)) if not np.array_equal(got[i], want[i])]
    assert not bad, "rows differ from icl_load_image_224: %s" % bad
    nprog = sum(1 for p in files if is_progressive(p))
    st = ctx.last_entropy_stats()
    assert st["gpu_entropy_jpegs"] == len(files) - nprog and st["redone_on_host"] == 0 and st["host_entropy_jpegs"] == nprog, st
    assert st["stream_bytes"] > 0
    assert ctx.last_ingest_stats()["gpu_jpegs"] == len(files)


@pytest.mark.parametrize("head", [2048, 1000])
@pytest.mark.parametrize("prec", ["PREC_BF16", "PREC_BF16X3", "PREC_FP32"])
def test_embed_files_equal_embed_u8(L, ctx, files, head, prec):
    prec = getattr(L, prec)
    paths = files[::3]
    ref = ctx.embed_u8(host_rows(L, paths), head, prec)
    E, status = ctx.embed_files(paths, head, prec, 4)
    assert (status == 0).all() and np.array_equal(E, ref)
    st = ctx.last_entropy_stats()
    assert st["gpu_entropy_jpegs"] == sum(1 for p in paths if not is_progressive(p)) and st["redone_on_host"] == 0, st
    d = ctx.malloc(len(paths) * head * 4)
    try:
        status = ctx.embed_files_dev(paths, d, head, prec, 4)
        Ed = np.empty((len(paths), head), np.float32)
        ctx.d2h(Ed, d)
    finally:
        ctx.free(d)
    assert (status == 0).all() and np.array_equal(Ed, ref)


@pytest.mark.parametrize("threads", [1, 4, 16])
def test_ragged_slabs(L, ctx, files, threads):
    small = [p for p in files if "1920" not in p and "4000" not in p and "1080" not in p]
    paths = (small * (301 // len(small) + 1))[:301]
    want = host_rows(L, small)
    idx = {p: i for i, p in enumerate(small)}
    got, status = ctx.load_images_224(paths, threads=threads)
    assert (status == 0).all()
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], want[idx[p]]), (threads, i, p)
    st = ctx.last_entropy_stats()
    assert st["gpu_entropy_jpegs"] == sum(1 for p in paths if not is_progressive(p)) and st["redone_on_host"] == 0, st


def test_mixed_list_equals_host_mode(L, ctx, tmp_path):
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    try:
        pic = picture(97, 61, 7)
        jpg = save_jpeg(tmp_path / "a.jpg", 97, 61, 7, quality=85)
        png = str(tmp_path / "b.png")
        Image.fromarray(pic).save(png)
        ppm = str(tmp_path / "c.ppm")
        open(ppm, "wb").write(b"P6\n97 61\n255\n" + pic.tobytes())
        paths = [jpg, png, str(tmp_path / "missing.jpg"), ppm] + damaged(tmp_path) + [jpg]
        host = L.Context(0)
        try:
            want, wstatus = host.load_images_224(paths, threads=3)
            werr = host.last_error()
            assert host.last_entropy_stats()["gpu_entropy_jpegs"] == 0
        finally:
            host.close()
        # what the check must decide, from the host loop over the same subsequences (validated on this set by test_jpeg_entropy_cpu.py)
        state = np.array([L.jpeg_coefs_file_host(p, 1024)[1]["state"] if p.endswith(".jpg") and "missing" not in p else -1 for p in paths])
        got, status = ctx.load_images_224(paths, threads=3)  # the damaged set goes through the GPU once
        assert list(status) == list(wstatus)
        assert np.array_equal(got, want)
        assert ctx.last_error() == werr
        st = ctx.last_entropy_stats()
        assert st["redone_on_host"] == int((state == 0).sum()) and st["redone_on_host"] > 0, (st, state)
        assert st["gpu_entropy_jpegs"] == int((state == 1).sum()), (st, state)
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_switching_back_to_host_mode(L, ctx, files):
    paths = files[:12]
    ctx.set_ingest_options(L.ENTROPY_HOST)
    try:
        got, status = ctx.load_images_224(paths, threads=4)
        st = ctx.last_entropy_stats()
        assert st["gpu_entropy_jpegs"] == 0 and st["redone_on_host"] == 0 and st["stream_bytes"] == 0 and st["host_entropy_jpegs"] == len(paths), st
        assert (status == 0).all() and np.array_equal(got, host_rows(L, paths))
        assert ctx.last_ingest_stats()["gpu_jpegs"] == len(paths)
    finally:
        ctx.set_ingest_options(L.ENTROPY_GPU)
