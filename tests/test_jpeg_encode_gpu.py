"""The GPU JPEG encoder (jpeg_encode_gpu.hip): icl_jpeg_encode_rgb_dev encodes a batch of resident RGB images of different sizes in one
call; every file must equal the host encoder's (icl_jpeg_encode_rgb, itself pinned to Pillow in test_jpeg_encode_cpu.py) byte for byte."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

from tests.downsize_cases import CONTENTS, SIZES, content

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch():
    """1x1 first and last (the scans cross image boundaries with the smallest images at the ends), the CPU sizes and contents in between."""
    mid = [content(CONTENTS[i % len(CONTENTS)], w, h, seed=i) for i, (w, h) in enumerate(SIZES[1:])]
    return [content("noise", 1, 1, 50)] + mid + [content("primaries", 1, 1)]


@pytest.fixture(scope="module")
def host_files(L, batch):
    """The reference, computed once per quality."""
    return {q: [L.jpeg_encode(a, q) for a in batch] for q in (95, 30)}


def check(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: file %d: %d bytes against the host encoder's %d" % (what, i, len(g), len(w))


def test_batch_equals_host_encoder(L, ctx, batch, host_files):
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    try:
        assert len(batch) == 9
        check(ctx.jpeg_encode_dev(batch, 95), host_files[95], "quality 95")
        check(ctx.jpeg_encode_dev(batch[::-1], 95), host_files[95][::-1], "reversed")
        check(ctx.jpeg_encode_dev(batch, 30), host_files[30], "quality 30")
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_large_noise_image_and_every_content(L, ctx):
    """640x480 noise at quality 95: a stream of several hundred KB over many packing and stuffing chunks; then each content at 37x53."""
    faulthandler.dump_traceback_later(300, exit=True)
    try:
        big = content("noise", 640, 480, 9)
        want = L.jpeg_encode(big, 95)
        assert len(want) > 300000 and want.count(b"\xff\x00") > 100
        imgs = [content("flat", 17, 33), big] + [content(k, 37, 53) for k in CONTENTS]
        check(ctx.jpeg_encode_dev(imgs, 95), [L.jpeg_encode(imgs[0], 95), want] + [L.jpeg_encode(a, 95) for a in imgs[2:]], "large batch")
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_one_image_and_none(L, ctx, batch, host_files):
    check(ctx.jpeg_encode_dev([batch[5]], 95), [host_files[95][5]], "n = 1")
    assert ctx.jpeg_encode_dev([], 95) == []


def test_more_images_than_one_batch_holds(L, ctx):
    """66 000 one-pixel images: more than the 65 535 a batch takes (its per-image kernels index the image by gridDim.y), so the call splits."""
    faulthandler.dump_traceback_later(300, exit=True)
    try:
        kinds = [np.full((1, 1, 3), v, np.uint8) for v in ((0, 0, 0), (255, 0, 0), (10, 200, 30), (255, 255, 255))]
        want = [L.jpeg_encode(a, 95) for a in kinds]
        n = 66000
        got = ctx.jpeg_encode_dev([kinds[i % 4] for i in range(n)], 95)
        assert len(got) == n and all(got[i] == want[i % 4] for i in range(n))
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_arguments_and_small_buffer(L, ctx):
    lib = L.load()
    a = content("gradient", 16, 16)
    want = L.jpeg_encode(a, 95)
    d = ctx.malloc(a.nbytes)
    try:
        ctx.h2d(d, a)
        offs, w, h = np.zeros(1, np.int64), np.array([16], np.int32), np.array([16], np.int32)
        out, oo = np.zeros(len(want), np.uint8), np.zeros(2, np.int64)
        args = (ctx.h, C.c_void_p(d), offs.ctypes.data, w.ctypes.data, h.ctypes.data, 1)
        assert lib.icl_jpeg_encode_rgb_dev(*args, 95, out.ctypes.data, 0, len(want) - 1, oo.ctypes.data) == L.ICL_ERR_ARG and oo[1] == len(want)
        assert lib.icl_jpeg_encode_rgb_dev(*args, 95, out.ctypes.data, 0, len(want), oo.ctypes.data) == L.ICL_OK and out.tobytes() == want
        assert lib.icl_jpeg_encode_rgb_dev(*args, 0, out.ctypes.data, 0, len(want), oo.ctypes.data) == L.ICL_ERR_ARG
        assert lib.icl_jpeg_encode_rgb_dev(*args, 95, out.ctypes.data, 0, len(want), None) == L.ICL_ERR_ARG
        bad = np.array([0], np.int32)
        assert lib.icl_jpeg_encode_rgb_dev(ctx.h, C.c_void_p(d), offs.ctypes.data, bad.ctypes.data, h.ctypes.data, 1, 95, out.ctypes.data, 0, len(want),
                                           oo.ctypes.data) == L.ICL_ERR_ARG
    finally:
        ctx.free(d)
