"""The host JPEG encoder (jpeg_encode.hip, arithmetic in jpeg_encode_pixels.h): icl_jpeg_encode_rgb must write, byte for byte, the file
Pillow (libjpeg-turbo) writes with nothing but the quality set -- what cv::imwrite(".jpg") asks libjpeg for.  No tolerance.  No GPU."""
import numpy as np
import pytest

from tests.downsize_cases import CONTENTS, QUALITIES, SIZES, content, pillow_jpeg, pillow_pixels, scan_of


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


# natural-order index of the k-th coefficient in zig-zag order (T.81 figure A.6)
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43,
          36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def zrl_symbols(L, path):
    """0xF0 symbols the file's blocks need: zero runs of 16 or more in front of a non-zero AC coefficient, in zig-zag order."""
    coefs, info = L.jpeg_coefs_file_host(path)
    blocks = np.asarray(coefs).reshape(-1, 64)[:, ZIGZAG]
    n = 0
    for b in blocks:
        nz = np.flatnonzero(b[1:]) + 1
        prev = 0
        for k in nz:
            n += (k - prev - 1) // 16
            prev = k
    return n


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_bytes_equal_pillow(L, size, kind, tmp_path):
    w, h = size
    rgb = content(kind, w, h)
    for q in QUALITIES:
        ours, ref = L.jpeg_encode(rgb, q), pillow_jpeg(rgb, q)
        assert len(ours) <= L.jpeg_encode_bound(w, h), (size, kind, q)
        if ours != ref:
            first = next((i for i in range(min(len(ours), len(ref))) if ours[i] != ref[i]), min(len(ours), len(ref)))
            raise AssertionError("%dx%d %s q%d: %d bytes against Pillow's %d, first difference at byte %d" % (w, h, kind, q, len(ours), len(ref), first))
        if kind == "noise" and w * h >= 64 * 48 and q >= 95:
            assert b"\xff\x00" in scan_of(ours), "no stuffed 0xFF in a noise stream: stuffing was not exercised"
        if kind == "sparse_hf" and q == 30 and w >= 8 and h >= 8:
            p = tmp_path / "hf.jpg"
            p.write_bytes(ours)
            assert zrl_symbols(L, str(p)) >= 1, "no ZRL symbol in the sparse high-frequency image"
        if q in (95, 30):  # Pillow reads our file without a warning, and our decoder agrees with it on the pixels
            assert np.array_equal(L.decode_image_mem(ours), pillow_pixels(ours, transposed=False)), (size, kind, q)


def test_arguments(L):
    import ctypes as C

    lib = L.load()
    px = np.zeros((4, 4, 3), np.uint8)
    n = C.c_int64(0)
    E = L.ICL_ERR_ARG
    assert lib.icl_jpeg_encode_rgb(None, 4, 4, 95, None, 0, C.byref(n)) == E
    assert lib.icl_jpeg_encode_rgb(px.ctypes.data, 4, 4, 95, None, 0, None) == E
    for w, h in [(0, 4), (4, 0), (-1, 4), (65536, 1), (1, 65536)]:
        assert lib.icl_jpeg_encode_rgb(px.ctypes.data, w, h, 95, None, 0, C.byref(n)) == E, (w, h)
        assert lib.icl_jpeg_encode_bound(w, h) == 0
    for q in (0, 101, -5):
        assert lib.icl_jpeg_encode_rgb(px.ctypes.data, 4, 4, q, None, 0, C.byref(n)) == E, q
    # the size query, then a buffer one byte short
    assert lib.icl_jpeg_encode_rgb(px.ctypes.data, 4, 4, 95, None, 0, C.byref(n)) == L.ICL_OK and n.value == len(pillow_jpeg(px, 95))
    out = np.zeros(n.value, np.uint8)
    m = C.c_int64(0)
    assert lib.icl_jpeg_encode_rgb(px.ctypes.data, 4, 4, 95, out.ctypes.data, n.value - 1, C.byref(m)) == E and m.value == n.value
    assert lib.icl_jpeg_encode_rgb(px.ctypes.data, 4, 4, 95, out.ctypes.data, n.value, C.byref(m)) == L.ICL_OK
    assert out.tobytes() == pillow_jpeg(px, 95)


def test_bound_holds_at_the_worst_quality(L):
    """quality 100 (every divisor 8) on noise and on the checkerboard: the longest streams the encoder writes stay under the bound."""
    for kind in ("noise", "checker"):
        for w, h in SIZES:
            assert len(L.jpeg_encode(content(kind, w, h), 100)) <= L.jpeg_encode_bound(w, h)
    assert L.jpeg_encode_bound(65535, 65535) > 0
