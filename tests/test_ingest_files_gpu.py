"""Batched file ingest (jpeg_gpu.hip): icl_load_images_224_dev / icl_embed_files[_dev] against the host path.

Host workers run stage A of the JPEG decoder (parsing + entropy decoding); the GPU rebuilds the pixels (dequantisation, islow IDCT,
fancy upsampling, colour conversion), applies the EXIF orientation and resizes.  Every row must equal icl_load_image_224's output
for its file byte for byte, and every embedding row must equal icl_embed_u8 on those images bit for bit."""
import ctypes
import faulthandler
import os

import numpy as np
import pytest
from PIL import Image, ImageFile

pytestmark = pytest.mark.gpu
ImageFile.MAXBLOCK = 1 << 26  # Pillow's progressive encoder needs the whole file in one buffer


def picture(w, h, seed):
    """A smooth photo-like image plus noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (7 + 13 * c) + y / (11 + 5 * c) + c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def save_jpeg(path, w, h, seed, **kw):
    im = Image.fromarray(picture(w, h, seed))
    if kw.pop("grey", False):
        im = im.convert("L")
    im.save(str(path), "JPEG", **kw)
    return str(path)


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
def corpus(tmp_path_factory):
    """JPEGs only: every size, subsampling, progressive, restart intervals, greyscale, RGB transform, EXIF orientations 1-8."""
    d = tmp_path_factory.mktemp("ingest")
    paths = []
    seed = 0
    for w, h in [(1, 1), (8, 8), (17, 9), (37, 53), (224, 224), (448, 448), (481, 322), (1920, 1080)]:
        for sub in (0, 1, 2):  # 4:4:4, 4:2:2, 4:2:0
            seed += 1
            paths.append(save_jpeg(d / ("b%d_%dx%d_s%d.jpg" % (seed, w, h, sub)), w, h, seed, quality=80, subsampling=sub))
        seed += 1
        paths.append(save_jpeg(d / ("p%d_%dx%d.jpg" % (seed, w, h)), w, h, seed, quality=75, subsampling=2, progressive=True))
        seed += 1
        paths.append(save_jpeg(d / ("g%d_%dx%d.jpg" % (seed, w, h)), w, h, seed, quality=85, grey=True))
    paths.append(save_jpeg(d / "big_4000x3000.jpg", 4000, 3000, 99, quality=75))
    paths.append(save_jpeg(d / "pg_481x322.jpg", 481, 322, 100, quality=70, progressive=True, grey=True))
    paths.append(save_jpeg(d / "rst_blocks.jpg", 481, 322, 101, quality=75, subsampling=2, restart_marker_blocks=3))
    paths.append(save_jpeg(d / "rst_rows.jpg", 37, 53, 102, quality=75, subsampling=1, restart_marker_rows=1))
    paths.append(save_jpeg(d / "rst_prog.jpg", 481, 322, 103, quality=75, subsampling=2, progressive=True, restart_marker_blocks=5))
    paths.append(save_jpeg(d / "q95_444.jpg", 1920, 1080, 104, quality=95, subsampling=0))
    try:  # RGB components without colour transform (Adobe transform 0), where this Pillow can write one
        paths.append(save_jpeg(d / "keep_rgb.jpg", 481, 322, 105, quality=90, keep_rgb=True))
    except (TypeError, ValueError, OSError):
        pass
    for orient in range(1, 9):
        for (w, h), sub in (((37, 53), 2), ((481, 322), 1), ((448, 448), 0)):
            exif = Image.Exif()
            exif[0x0112] = orient
            seed += 1
            paths.append(save_jpeg(d / ("o%d_%dx%d.jpg" % (orient, w, h)), w, h, seed, quality=85, subsampling=sub, exif=exif.tobytes()))
    return paths


def host_rows(L, paths):
    return np.stack([L.load_image_224(p) for p in paths])


def test_load_images_bit_identical_to_host(L, ctx, corpus):
    want = host_rows(L, corpus)
    got, status = ctx.load_images_224(corpus, threads=8)
    assert (status == 0).all()
    bad = [corpus[i] for i in range(len(corpus)) if not np.array_equal(got[i], want[i])]
    assert not bad, "rows differ from icl_load_image_224: %s" % bad
    st = ctx.last_ingest_stats()
    # the GPU path ran for every file: byte equality alone would also pass with a host fallback
    assert st["gpu_jpegs"] == len(corpus) and st["host_files"] == 0, st
    assert st["upload_bytes"] > 0 and st["host_decode_s"] > 0


@pytest.mark.parametrize("threads", [1, 4, 16])
def test_threads_and_ragged_slabs_do_not_change_rows(L, ctx, corpus, threads):
    small = [p for p in corpus if "1920" not in p and "4000" not in p]
    paths = (small * (301 // len(small) + 1))[:301]  # more than one slab of 256 rows, not a multiple of it
    want = host_rows(L, small)
    idx = {p: i for i, p in enumerate(small)}
    got, status = ctx.load_images_224(paths, threads=threads)
    assert (status == 0).all()
    for i, p in enumerate(paths):
        assert np.array_equal(got[i], want[idx[p]]), (threads, i, p)
    assert ctx.last_ingest_stats()["gpu_jpegs"] == len(paths)
    E, status = ctx.embed_files(paths, L.HEAD_POOLED, L.PREC_BF16, threads)
    ref = ctx.embed_u8(np.stack([want[idx[p]] for p in paths]), L.HEAD_POOLED, L.PREC_BF16)
    assert (status == 0).all() and np.array_equal(E, ref)


@pytest.mark.parametrize("head", [2048, 1000])
@pytest.mark.parametrize("prec", ["PREC_BF16", "PREC_BF16X3", "PREC_FP32"])
def test_embed_files_equal_two_step_path(L, ctx, corpus, head, prec):
    prec = getattr(L, prec)
    paths = corpus[::3]
    imgs = host_rows(L, paths)
    ref = ctx.embed_u8(imgs, head, prec)
    E, status = ctx.embed_files(paths, head, prec, 4)
    assert (status == 0).all() and np.array_equal(E, ref)
    assert ctx.last_ingest_stats()["gpu_jpegs"] == len(paths)
    d = ctx.malloc(len(paths) * head * 4)
    try:
        status = ctx.embed_files_dev(paths, d, head, prec, 4)
        Ed = np.empty((len(paths), head), np.float32)
        ctx.d2h(Ed, d)
    finally:
        ctx.free(d)
    assert (status == 0).all() and np.array_equal(Ed, ref)


def test_mixed_list_statuses_and_failed_rows(L, ctx, tmp_path):
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    try:
        pic = picture(97, 61, 7)
        jpg = save_jpeg(tmp_path / "a.jpg", 97, 61, 7, quality=85)
        png = str(tmp_path / "b.png")
        Image.fromarray(pic).save(png)
        ppm = str(tmp_path / "c.ppm")
        open(ppm, "wb").write(b"P6\n97 61\n255\n" + pic.tobytes())
        missing = str(tmp_path / "missing.jpg")
        trunc = str(tmp_path / "trunc.jpg")
        data = open(save_jpeg(tmp_path / "full.jpg", 300, 200, 8, quality=90), "rb").read()
        open(trunc, "wb").write(data[: len(data) // 3])
        cmyk = str(tmp_path / "cmyk.jpg")
        Image.fromarray(pic).convert("CMYK").save(cmyk, "JPEG")
        paths = [jpg, png, missing, ppm, trunc, cmyk, jpg]
        want_status, want_rows = [], []
        for p in paths:
            try:
                want_rows.append(L.load_image_224(p))
                want_status.append(0)
            except L.ICLError as e:
                want_rows.append(None)
                want_status.append(e.code)
        assert want_status[2] == L.ICL_ERR_IO and want_status[5] != 0  # the list does hold failures
        lowest = next(i for i, s in enumerate(want_status) if s)

        got, status = ctx.load_images_224(paths, threads=3)
        assert list(status) == want_status
        for i, w in enumerate(want_rows):
            assert np.array_equal(got[i], w if w is not None else np.zeros_like(got[i])), paths[i]
        assert "file %d of %d" % (lowest, len(paths)) in ctx.last_error()
        st = ctx.last_ingest_stats()
        n_gpu = sum(1 for p, s in zip(paths, want_status) if s == 0 and p.endswith(".jpg"))
        assert st["gpu_jpegs"] == n_gpu and st["host_files"] == 2, st

        # the raw entry point's code names the lowest failed file
        enc = [os.fsencode(p) for p in paths]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        out = np.zeros((len(paths), 2048), np.float32)
        st32 = np.zeros(len(paths), np.int32)
        rc = L.load().icl_embed_files(ctx.h, arr, len(paths), 2048, L.PREC_FP32, 2, out.ctypes.data, st32.ctypes.data)
        assert rc == want_status[lowest] and list(st32) == want_status
        ok = [i for i, s in enumerate(want_status) if s == 0]
        ref = ctx.embed_u8(np.stack([want_rows[i] for i in ok]), 2048, L.PREC_FP32)
        assert np.array_equal(out[ok], ref)
        for i, s in enumerate(want_status):
            if s:
                assert np.isnan(out[i]).all(), i
        d = ctx.malloc(len(paths) * 1000 * 4)
        try:
            status = ctx.embed_files_dev(paths, d, 1000, L.PREC_BF16, 0)
            Ed = np.empty((len(paths), 1000), np.float32)
            ctx.d2h(Ed, d)
        finally:
            ctx.free(d)
        assert list(status) == want_status
        assert np.array_equal(Ed[ok], ctx.embed_u8(np.stack([want_rows[i] for i in ok]), 1000, L.PREC_BF16))
        assert all(np.isnan(Ed[i]).all() for i, s in enumerate(want_status) if s)
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_empty_list_and_bad_arguments(L, ctx):
    out, status = ctx.load_images_224([], threads=0)
    assert out.shape == (0, 224, 224, 3) and status.shape == (0,)
    assert ctx.last_ingest_stats()["gpu_jpegs"] == 0
    with pytest.raises(L.ICLError):
        ctx.embed_files(["x.jpg"], 777, L.PREC_BF16)
    with pytest.raises(L.ICLError):
        ctx.embed_files(["x.jpg"], 2048, 9)
