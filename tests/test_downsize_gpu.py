"""The batched downsizer (jpeg_gpu.hip driver, encoder kernels of jpeg_encode_gpu.hip): icl_downsize_images[_mem] over a mixed list must
give, image by image, the bytes icl_downsize_image_mem gives (pinned to Pillow in test_downsize_cpu.py), in both entropy modes and for
any number of host threads; a failed image fails alone."""
import faulthandler

import numpy as np
import pytest

from tests.downsize_cases import _save, noise_ppm, sources, truncated_jpeg
from tests.jpeg_entropy_cases import picture
from tests.jpeg_sampling_cases import make

pytestmark = pytest.mark.gpu
MAX_BYTES, MAX_DIM = 7000, 96


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
def inputs(L, tmp_path_factory):
    """(paths, buffers, expected files or None, expected status): about 14 inputs from the CPU cases."""
    d = tmp_path_factory.mktemp("downsize")
    S = sources()
    c440 = make(d, "y440.jpg", (1, 2), (400, 304), seed=41, quality=95)
    small = _save(picture(97, 61, 40), "JPEG", quality=85)
    items = [
        ("small.jpg", small),  # passthrough
        ("jpeg_420.jpg", S["jpeg_420"]),
        ("jpeg_444.jpg", S["jpeg_444"]),
        ("text.bin", b"not an image " * 40),  # passthrough of a non-image
        ("jpeg_422.jpg", S["jpeg_422"]),
        ("jpeg_440.jpg", open(c440["path"], "rb").read()),
        ("trunc.jpg", truncated_jpeg()),
        ("jpeg_gray.jpg", S["jpeg_gray"]),
        ("jpeg_progressive.jpg", S["jpeg_progressive"]),
        ("jpeg_orient6.jpg", S["jpeg_orient6"]),
        ("png_alpha.png", S["png_alpha"]),
        ("ppm.ppm", S["ppm"]),
        ("second.jpg", _save(np.random.default_rng(3).integers(0, 256, (300, 300, 3), dtype=np.uint8), "JPEG", quality=95)),  # noise: a second attempt
        ("second.ppm", noise_ppm(260, 260, 4)),  # ... of a host-decoded image
    ]
    paths, bufs, want, status = [], [], [], []
    for name, data in items:
        p = d / name
        p.write_bytes(data)
        paths.append(str(p))
        bufs.append(data)
        try:
            want.append(L.downsize_image_mem(data, MAX_BYTES, MAX_DIM))
            status.append(0)
        except L.ICLError as e:
            want.append(None)
            status.append(e.code)
    paths.insert(5, str(d / "missing.jpg"))
    bufs.insert(5, None)
    want.insert(5, None)
    status.insert(5, L.ICL_ERR_IO)
    assert len(S["jpeg_420"]) > MAX_BYTES >= len(small) and sum(1 for s in status if s) == 2
    infos = [L.downsize_image_mem(b, MAX_BYTES, MAX_DIM, want_info=True)[1] for b, s in zip(bufs, status) if s == 0]
    assert sum(i["attempts"] == 2 for i in infos) >= 2 and sum(i["passthrough"] for i in infos) == 2
    return paths, bufs, want, status


def check(L, ctx, got, status, want, want_status, what):
    assert list(status) == want_status, what
    for i, w in enumerate(want):
        assert got[i] == (w if w is not None else b""), "%s: image %d: %d bytes against the host call's %d" % (what, i, len(got[i]), len(w or b""))
    st = ctx.last_downsize_stats()
    failed = sum(1 for s in want_status if s)
    assert st["passthrough"] + st["gpu_rebuilt"] + st["host_decoded"] == len(want) - failed, st
    assert st["passthrough"] == 2 and st["gpu_rebuilt"] > 0 and st["host_decoded"] >= 3 and st["second_attempts"] >= 2, st
    assert st["bytes_out"] == sum(len(g) for g in got)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("entropy", ["host", "gpu"])
def test_mixed_list_equals_host_call(L, ctx, inputs, entropy, threads):
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    paths, bufs, want, want_status = inputs
    try:
        ctx.set_ingest_options(L.ENTROPY_GPU if entropy == "gpu" else L.ENTROPY_HOST)
        got, status = ctx.downsize_images_mem(bufs, MAX_BYTES, MAX_DIM, threads)
        check(L, ctx, got, status, want, want_status, "memory")
        lowest = next(i for i, s in enumerate(want_status) if s)
        assert "file %d of %d" % (lowest, len(want)) in ctx.last_error()
        if entropy == "gpu":
            assert ctx.last_downsize_stats()["gpu_rebuilt"] >= 5
        got, status = ctx.downsize_images(paths, MAX_BYTES, MAX_DIM, threads)
        check(L, ctx, got, status, want, want_status, "paths")
    finally:
        ctx.set_ingest_options(L.ENTROPY_HOST)
        faulthandler.cancel_dump_traceback_later()


def test_return_code_and_small_buffer(L, ctx, inputs):
    import ctypes as C

    paths, bufs, want, want_status = inputs
    lib = L.load()
    data, size, n, keep = L._byte_arrays(bufs)
    total = sum(len(w) for w in want if w)
    st, oo = np.zeros(n, np.int32), np.zeros(n + 1, np.int64)
    out = np.zeros(total, np.uint8)
    rc = lib.icl_downsize_images_mem(ctx.h, data, size, n, MAX_BYTES, MAX_DIM, 2, out.ctypes.data, total - 1, oo.ctypes.data, st.ctypes.data)
    assert rc == L.ICL_ERR_ARG and oo[n] == total
    rc = lib.icl_downsize_images_mem(ctx.h, data, size, n, MAX_BYTES, MAX_DIM, 2, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data)
    lowest = next(i for i, s in enumerate(want_status) if s)
    assert rc == want_status[lowest] and list(st) == want_status
    assert [out[oo[i]:oo[i + 1]].tobytes() for i in range(n)] == [w or b"" for w in want]
    assert lib.icl_downsize_images_mem(ctx.h, data, size, 0, MAX_BYTES, MAX_DIM, 2, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data) == L.ICL_OK and oo[0] == 0
    assert lib.icl_downsize_images_mem(ctx.h, data, size, n, MAX_BYTES, 0, 2, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data) == L.ICL_ERR_ARG
    del keep
