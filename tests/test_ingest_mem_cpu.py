"""Images from memory on the host (icl_decode_image_mem, icl_load_image_224_mem, icl_preprocess_mem): the bytes of a file give exactly
what the path call gives for the file -- pixels, size, floats, status code -- and a message that names the image as
"image 0 (in memory, N bytes)" where the path call names the path.  No GPU."""
import ctypes as C

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_entropy_cases, jpeg_sampling_cases
from tests.jpeg_entropy_cases import picture, save_jpeg
from tests.test_png_decode import adam7_png


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The decode, PNG and sampling corpora as files: baseline and progressive JPEG at 1x1 / 2x1 / 2x2 (Pillow) and 1x2 / 4x1 / 1x4
    (rewritten frame headers), grey, restart intervals, the EXIF orientations, PNG colour types 0 / 2 / 3 / 4 / 6, Adam7, PPM."""
    d = tmp_path_factory.mktemp("mem_cpu")
    paths = [p for p in jpeg_entropy_cases.corpus(d, big=False) if "1920" not in p and "1080" not in p]
    paths.append(save_jpeg(d / "one_1920x1080.jpg", 1920, 1080, 31, quality=75, subsampling=2))
    for sub in (0, 1):  # (the entropy corpus holds progressive files at 4:2:0 only)
        paths.append(save_jpeg(d / ("prog_s%d.jpg" % sub), 97, 61, 40 + sub, quality=80, subsampling=sub, progressive=True))
    paths += [c["path"] for c in jpeg_sampling_cases.corpus(d)]
    pic = picture(67, 45, 50)
    for mode in ("L", "RGB", "P", "LA", "RGBA"):  # colour types 0, 2, 3, 4, 6
        p = d / ("ct_%s.png" % mode)
        Image.fromarray(pic).convert(mode).save(str(p))
        paths.append(str(p))
    p = d / "adam7.png"
    p.write_bytes(adam7_png(pic[:29, :37].astype(int), 8, 2))
    paths.append(str(p))
    p = d / "c.ppm"
    p.write_bytes(b"P6\n# a comment\n67 45\n255\n" + pic.tobytes())
    paths.append(str(p))
    return paths


def test_the_corpus_covers_what_it_should(files):
    lumas = {(jpeg_sampling_cases.frame(open(p, "rb").read())[2][0], jpeg_entropy_cases.is_progressive(p)) for p in files if p.endswith(".jpg")
             and len(jpeg_sampling_cases.frame(open(p, "rb").read())[2]) == 3}
    for luma in ((1, 1), (2, 1), (2, 2), (1, 2), (4, 1), (1, 4)):
        assert (luma, False) in lumas and (luma, True) in lumas, luma
    names = " ".join(files)
    for part in ("/g", "/pg_", "rst_", "/o1_", "/o8_", "ct_P.png", "ct_LA.png", "adam7.png", ".ppm"):
        assert part in names, part


def test_decode_parity(L, files):
    for p in files:
        data = open(p, "rb").read()
        want = L.decode_image_file(p)
        for buf in (data, bytearray(data), memoryview(data), np.frombuffer(data, np.uint8)):
            got = L.decode_image_mem(buf)
            assert got.shape == want.shape and np.array_equal(got, want), p
        assert np.array_equal(L.load_image_224_mem(data), L.load_image_224(p)), p
        assert np.array_equal(L.preprocess_mem(data), L.preprocess_file(p)), p


def test_size_only_and_small_buffer(L, files):
    data = open(files[0], "rb").read()
    lib = L.load()
    w, h = C.c_int32(), C.c_int32()
    assert lib.icl_decode_image_mem(data, len(data), None, 0, C.byref(w), C.byref(h)) == L.ICL_OK
    assert (w.value, h.value) == L.decode_image_file(files[0]).shape[1::-1]
    small = np.zeros(2, np.uint8)
    assert lib.icl_decode_image_mem(data, len(data), small.ctypes.data, 2, C.byref(w), C.byref(h)) == L.ICL_ERR_ARG
    assert lib.icl_decode_image_mem(data, len(data), None, 0, None, C.byref(h)) == L.ICL_ERR_ARG
    assert lib.icl_load_image_224_mem(data, len(data), None) == L.ICL_ERR_ARG
    assert lib.icl_preprocess_mem(data, len(data), None) == L.ICL_ERR_ARG


def _code_and_message(call, *args):
    try:
        call(*args)
    except Exception as e:  # ICLError
        return e.code, str(e).split(": ", 1)[1]
    return 0, ""


@pytest.mark.parametrize("kind", ["truncated_jpeg", "truncated_png", "truncated_ppm", "zeros", "jpeg_magic_only"])
def test_errors_equal_the_path_calls(L, files, tmp_path, kind):
    src = {"truncated_jpeg": ".jpg", "truncated_png": ".png", "truncated_ppm": ".ppm"}.get(kind)
    if src:
        data = open([p for p in files if p.endswith(src)][0], "rb").read()
        data = data[: len(data) // 2]
    else:
        data = bytes(4096) if kind == "zeros" else b"\xff\xd8"
    p = tmp_path / "bad.bin"
    p.write_bytes(data)
    name = "image 0 (in memory, %d bytes)" % len(data)
    for mem, path in ((L.decode_image_mem, L.decode_image_file), (L.load_image_224_mem, L.load_image_224), (L.preprocess_mem, L.preprocess_file)):
        wcode, wmsg = _code_and_message(path, str(p))
        code, msg = _code_and_message(mem, data)
        assert wcode != 0 and code == wcode
        assert str(p) in wmsg and msg == wmsg.replace(str(p), name), (msg, wmsg)


@pytest.mark.parametrize("buf", [b"", None, bytearray()])
def test_an_empty_buffer_is_the_images_own_failure(L, tmp_path, buf):
    p = tmp_path / "empty.jpg"
    p.write_bytes(b"")
    for mem, path in ((L.decode_image_mem, L.decode_image_file), (L.load_image_224_mem, L.load_image_224), (L.preprocess_mem, L.preprocess_file)):
        wcode, _ = _code_and_message(path, str(p))
        code, msg = _code_and_message(mem, buf)
        assert code == wcode == L.ICL_ERR_IO
        assert msg == "failed to read image: image 0 (in memory, 0 bytes). empty image buffer"
    # data == NULL with bytes == 0, and a pointer with a length that is not positive, through the C ABI itself
    lib = L.load()
    w, h = C.c_int32(), C.c_int32()
    assert lib.icl_decode_image_mem(None, 0, None, 0, C.byref(w), C.byref(h)) == L.ICL_ERR_IO
    assert lib.icl_decode_image_mem(b"\xff\xd8", -1, None, 0, C.byref(w), C.byref(h)) == L.ICL_ERR_IO
    assert lib.icl_decode_image_mem(None, 100, None, 0, C.byref(w), C.byref(h)) == L.ICL_ERR_IO


def test_buffers_are_not_copied(L):
    """What the batched calls hand the library is the address of the caller's own buffer."""
    data = open(__file__, "rb").read()
    arr = np.frombuffer(data, np.uint8)
    ba = bytearray(data)
    for buf, addr in ((arr, arr.ctypes.data), (ba, C.addressof(C.c_char.from_buffer(ba))), (memoryview(ba)[5:], C.addressof(C.c_char.from_buffer(ba)) + 5)):
        p, n, keep = L._byte_view(buf)
        assert p == addr and n == len(buf) and keep is not None
    ptrs, sizes, n, keep = L._byte_arrays([arr, None, b""])
    assert n == 3 and ptrs[0] == arr.ctypes.data and ptrs[1] is None and ptrs[2] is None and list(sizes) == [arr.size, 0, 0]
    with pytest.raises(TypeError):
        L._byte_view(np.zeros(4, np.float32))
    with pytest.raises(TypeError):
        L._byte_view(np.zeros((4, 4), np.uint8)[:, ::2])


def test_jpeg_coefs_file_host_stays_a_path_call(L, files):
    """The host coefficient hook keeps its path interface and its results: the CPU tests need no memory twin of it."""
    p = [q for q in files if "/b" in q and "37x53_s2" in q][0]
    a, ia = L.jpeg_coefs_file_host(p, 0)
    b, ib = L.jpeg_coefs_file_host(p, 1024)
    assert ia["state"] == 1 and ib["state"] == 1 and a.size > 0 and np.array_equal(a, b)
    assert not hasattr(L.load(), "icl_jpeg_coefs_mem_host")
