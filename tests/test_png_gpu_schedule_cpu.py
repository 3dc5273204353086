"""The GPU PNG route rehearsed on the host (icl_png_raw_file_host: host stage P0 + the kernels' schedule of png_gpu.hip run as a plain loop
over the same __host__ __device__ functions, png_inflate.h).  For every clean case of tests/png_gpu_cases.py: the inflated stream is
zlib's, the unfiltered scanlines are those of the numpy unfilter below, the sample-to-RGB rule gives icl_decode_image_file's pixels.
Every reject case is rejected (and fails on the host with the stated message); files the route does not take report -1.  The corpus as
a whole must have reached the hard paths.  Runs without a GPU."""
import zlib

import numpy as np
import pytest

from imageclust_amd import _lib
from tests import png_gpu_cases


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return png_gpu_cases.write_all(tmp_path_factory.mktemp("png_gpu_cases"))


def unfilter(raw, h, rowb, bpp):
    """PNG 9.2 on h scanlines of 1 + rowb bytes; the filter bytes stay."""
    a = np.frombuffer(raw, np.uint8).reshape(h, rowb + 1).astype(np.int32)
    prev = np.zeros(rowb, np.int32)
    for y in range(h):
        ft, cur = a[y, 0], a[y, 1:]
        if ft == 2:
            cur[:] = (cur + prev) & 255
        elif ft in (1, 3, 4):
            for i in range(rowb):
                left = cur[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + prev[i]) >> 1
                else:
                    ul = prev[i - bpp] if i >= bpp else 0
                    p = left + prev[i] - ul
                    pa, pb, pc = abs(p - left), abs(p - prev[i]), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else (prev[i] if pb <= pc else ul)
                cur[i] = (cur[i] + pred) & 255
        prev = cur
    return a.astype(np.uint8).tobytes()


def test_bindings_exist():
    L = _lib.load()
    for name in ("icl_set_png_options", "icl_last_png_stats", "icl_png_raw_files", "icl_png_raw_file_host"):
        assert hasattr(L, name)
    assert (_lib.PNG_HOST, _lib.PNG_GPU) == (0, 1)


def test_clean_cases_stage_by_stage(corpus):
    clean = [c for c in corpus if c["kind"] == "clean"]
    assert len(clean) >= 50
    for c in clean:
        want = zlib.decompress(png_gpu_cases.idat_stream(c["data"]))
        raw, info = _lib.png_raw_file_host(c["path"], 0)
        assert info["state"] == 1 and raw.tobytes() == want, (c["name"], info)
        channels = png_gpu_cases.CHANNELS[info["ctype"]]
        rowb = png_gpu_cases.row_bytes(info["w"], info["depth"], info["ctype"])
        bpp = max(1, channels * info["depth"] // 8)
        lines, info1 = _lib.png_raw_file_host(c["path"], 1)
        assert info1["state"] == 1 and lines.tobytes() == unfilter(want, info["h"], rowb, bpp), c["name"]
        rgb, info2 = _lib.png_raw_file_host(c["path"], 2)
        ref = _lib.decode_image_file(c["path"])
        assert info2["state"] == 1 and ref.shape == (info["h"], info["w"], 3) and np.array_equal(rgb.reshape(ref.shape), ref), c["name"]


def test_reject_cases_are_rejected_and_fail_on_the_host(corpus):
    rejects = [c for c in corpus if c["kind"] == "reject"]
    assert len(rejects) == 11
    for c in rejects:
        raw, info = _lib.png_raw_file_host(c["path"], 1)
        assert info["state"] == 0 and raw.size == 0, (c["name"], info)
        with pytest.raises(_lib.ICLError) as e:
            _lib.decode_image_file(c["path"])
        assert ("PNG: " + c["message"]) in str(e.value), (c["name"], str(e.value))
    # the inflate stage alone accepts what only the later stages refuse
    by = {c["name"]: c for c in rejects}
    assert _lib.png_raw_file_host(by["reject_filter_5"]["path"], 0)[1]["state"] == 1
    assert _lib.png_raw_file_host(by["reject_palette_index"]["path"], 0)[1]["state"] == 1
    assert _lib.png_raw_file_host(by["reject_adler"]["path"], 0)[1]["state"] == 0


def test_files_the_route_does_not_take(corpus):
    for c in (c for c in corpus if c["kind"] == "unqualified"):
        for stage in (0, 1, 2):
            raw, info = _lib.png_raw_file_host(c["path"], stage)
            assert info["state"] == -1 and raw.size == 0, c["name"]
        if c["message"]:
            with pytest.raises(_lib.ICLError) as e:
                _lib.decode_image_file(c["path"])
            assert c["message"] in str(e.value)
        else:
            _lib.decode_image_file(c["path"])  # (Adam7: the host decoder reads it)


def test_corpus_reaches_the_hard_paths(corpus):
    """A test cannot pass by never reaching them: all three block kinds, a 15-bit code (longer than any primary table), a distance of
    32768, a match that overlaps its own output, a match across the ring's wrap."""
    infos = [_lib.png_raw_file_host(c["path"], 0)[1] for c in corpus if c["kind"] == "clean"]
    assert max(i["stored"] for i in infos) >= 2 and max(i["fixed"] for i in infos) >= 1 and max(i["dynamic"] for i in infos) >= 2
    assert max(i["max_code_len"] for i in infos) == 15
    assert max(i["max_dist"] for i in infos) == 32768
    assert sum(i["overlaps"] for i in infos) >= 1
    assert sum(i["ring_wraps"] for i in infos) >= 1
    by = {c["name"]: _lib.png_raw_file_host(c["path"], 0)[1] for c in corpus if c["name"] in ("match_straddles_wrap", "codes_single_distance", "blocks_rle")}
    assert by["match_straddles_wrap"]["ring_wraps"] >= 1 and by["match_straddles_wrap"]["max_dist"] == 32760
    assert by["codes_single_distance"]["overlaps"] == 3 and by["codes_single_distance"]["max_dist"] == 1
    assert by["blocks_rle"]["overlaps"] >= 1 and by["blocks_rle"]["max_dist"] == 1
