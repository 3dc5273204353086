"""4:4:0 (luma 1x2) and 4:1:1 (luma 4x1 / 1x4) JPEGs on the host path: pixels against Pillow's bundled libjpeg-turbo (h1v2_fancy_upsample
and int_upsample of jdsample.c, restated in ingest_pixels.h), the resize and preprocessing on top of them, and host stage A against the
GPU entropy decoder's schedule run as a host loop (icl_jpeg_coefs_file_host).  Fixtures: tests/jpeg_sampling_cases.py.  Runs without a GPU."""
import numpy as np
import pytest

from tests import jpeg_sampling_cases as SC


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return SC.corpus(tmp_path_factory.mktemp("sampling"))


@pytest.fixture(scope="module")
def pixels(cases):
    """Pillow's pixels of every fixture, the EXIF orientation applied (computed once, shared, never written to)."""
    out = {c["path"]: SC.pillow_rgb(c["path"], transposed=True) for c in cases}
    for a in out.values():
        a.setflags(write=False)
    return out


def test_the_corpus_covers_what_it_should(cases):
    for luma in ((1, 2), (4, 1), (1, 4)):
        mine = [c for c in cases if c["luma"] == luma]
        assert any(c["progressive"] for c in mine) and any(c["orient"] >= 5 for c in mine), luma
        assert any(c["size"] == (1, 1) for c in mine) and any(max(c["size"]) > 400 for c in mine), luma
        for c in mine:
            assert SC.frame(open(c["path"], "rb").read()) == (c["size"] + ([luma, (1, 1), (1, 1)],)), c


def test_pixels_equal_libjpeg_turbo(L, cases, pixels):
    bad = []
    for c in cases:
        got, ref = L.decode_image_file(c["path"]), pixels[c["path"]]
        w, h = c["size"][::-1] if c["orient"] >= 5 else c["size"]
        assert ref.shape == (h, w, 3), c
        if got.shape != ref.shape or not np.array_equal(got, ref):
            bad.append(c["path"])
    assert not bad, "pixels differ from Pillow's: %s" % bad


def test_load_image_224_is_the_resize_of_those_pixels(L, cases, pixels):
    for c in cases:
        assert np.array_equal(L.load_image_224(c["path"]), L.resize_u8(pixels[c["path"]], 224, 224)), c["path"]


@pytest.mark.parametrize("luma", [(1, 2), (4, 1), (1, 4)])
def test_preprocess_file(L, cases, pixels, luma):
    c = [c for c in cases if c["luma"] == luma and c["size"][0] > 40 and c["orient"] == 1][0]
    blob = L.preprocess_file(c["path"])
    want = L.resize_u8(pixels[c["path"]], 224, 224).transpose(2, 0, 1).astype(np.float32) * np.float32(1.0 / 255.0)
    assert blob.shape == (1, 3, 224, 224) and np.array_equal(blob[0], want)


def test_stage_a_equals_the_gpu_schedule(L, cases):
    nbase = 0
    for c in cases:
        want, wi = L.jpeg_coefs_file_host(c["path"], 0)
        assert wi["state"] == 1 and wi["ncomp"] == 3 and [wi["blocks0"], wi["blocks1"], wi["blocks2"]] == SC.blocks_of(c), (c, wi)
        assert want.size == 64 * sum(SC.blocks_of(c))
        got, gi = L.jpeg_coefs_file_host(c["path"], 1024)
        if c["progressive"]:
            assert gi["state"] == -1, (c, gi)
            continue
        nbase += 1
        assert gi["state"] == 1, "clean file rejected: %s %s" % (c["path"], gi)
        assert gi["ncomp"] == 3 and [gi["blocks0"], gi["blocks1"], gi["blocks2"]] == SC.blocks_of(c), (c, gi)
        assert np.array_equal(got, want), c["path"]
        if max(c["size"]) > 400:
            assert gi["nsub"] > 256, gi  # more than one workgroup of subsequences: the chain check crosses a launch boundary
    assert nbase == len(cases) - 3


def test_other_samplings_stay_unsupported(L, tmp_path):
    for p, sampling in SC.rejected(tmp_path):
        with pytest.raises(L.ICLError) as ei:
            L.decode_image_file(p)
        assert ei.value.code == L.ICL_ERR_UNSUPPORTED and "failed to read image" in str(ei.value) and ("Sampling " + sampling) in str(ei.value), str(ei.value)
        with pytest.raises(L.ICLError) as ei:
            L.load_image_224(p)
        assert ei.value.code == L.ICL_ERR_UNSUPPORTED
        assert L.jpeg_coefs_file_host(p, 1024)[1]["state"] == -1  # and the GPU entropy decoder does not take it either


def test_damaged_streams(L, cases, tmp_path):
    paths = SC.damaged(tmp_path, cases)
    assert len(paths) == 4
    for p in paths:
        try:
            rgb = L.decode_image_file(p)  # a status code or an image, never a crash
            assert rgb.shape[2] == 3
        except L.ICLError as e:
            assert e.code in (L.ICL_ERR_IO, L.ICL_ERR_UNSUPPORTED), (p, e)
        got, info = L.jpeg_coefs_file_host(p, 1024)
        assert info["state"] in (0, 1), (p, info)
        if info["state"] == 1:  # an accepted file is one stage A reads, with these coefficients
            want, _ = L.jpeg_coefs_file_host(p, 0)
            assert np.array_equal(got, want), p
    for p in paths:
        if "trunc_" in p:  # half the MCUs are missing: the block total cannot come out right
            assert L.jpeg_coefs_file_host(p, 1024)[1]["state"] == 0, p
