"""Batched file ingest (jpeg_gpu.hip) across every seam of its driver at once: a list of 520 files, i.e. slabs of 256 + 256 + 8 rows, of
two small baseline JPEGs plus one PNG, one progressive JPEG, one damaged JPEG that the GPU entropy check rejects (the repair pass), and a
missing path at the first and last row of the list and on both sides of the first slab boundary.  The three sinks (u8 rows on the
device, embeddings on the host, embeddings on the device) run in both entropy modes; rows, embeddings, statuses, the call's code and
message and the statistics must be what the one-file host path gives."""
import ctypes
import os

import numpy as np
import pytest
from PIL import Image

from tests.jpeg_entropy_cases import damaged, picture, save_jpeg

pytestmark = pytest.mark.gpu

N, HEAD = 520, 1000
MISSING = (0, 255, 256, 519)
PNG_ROW, PROG_ROW, BAD_ROW = 1, 300, 513  # one special file in each slab


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
def want(L, ctx, tmp_path_factory):
    """The list and what the one-file host path says about it: status, rows, embeddings of the good rows."""
    d = tmp_path_factory.mktemp("seams")
    a = save_jpeg(d / "a_37x53.jpg", 37, 53, 1, quality=80, subsampling=2)
    b = save_jpeg(d / "b_17x9.jpg", 17, 9, 2, quality=80, subsampling=0)
    png = str(d / "c.png")
    Image.fromarray(picture(97, 61, 3)).save(png)
    prog = save_jpeg(d / "p_37x53.jpg", 37, 53, 4, quality=75, subsampling=2, progressive=True)
    bad = next(p for p in damaged(d) if L.jpeg_coefs_file_host(p, 1024)[1]["state"] == 0)  # qualifies, and the check rejects it
    paths = [a if i % 2 else b for i in range(N)]
    paths[PNG_ROW], paths[PROG_ROW], paths[BAD_ROW] = png, prog, bad
    for i in MISSING:
        paths[i] = str(d / ("missing%d.jpg" % i))
    one = {}
    for p in set(paths):
        try:
            one[p] = (0, L.load_image_224(p))
        except L.ICLError as e:
            one[p] = (e.code, np.zeros((224, 224, 3), np.uint8))
    status = np.array([one[p][0] for p in paths], np.int32)
    rows = np.stack([one[p][1] for p in paths])
    good = np.flatnonzero(status == 0)
    assert all(status[i] == L.ICL_ERR_IO for i in MISSING) and status[PNG_ROW] == 0 and status[PROG_ROW] == 0
    emb = ctx.embed_u8(rows[good], HEAD, L.PREC_BF16)
    return {"paths": paths, "status": status, "rows": rows, "good": good, "emb": emb, "bad_ok": int(status[BAD_ROW] == 0)}


def _call(L, ctx, want, sink):
    """One raw entry point over the list -> (return code, message, status, output rows, ingest stats, entropy stats)."""
    enc = [os.fsencode(p) for p in want["paths"]]
    arr = (ctypes.c_char_p * N)(*enc)
    status = np.full(N, -1, np.int32)
    lib = L.load()
    if sink == "emb_host":
        out = np.zeros((N, HEAD), np.float32)
        rc = lib.icl_embed_files(ctx.h, arr, N, HEAD, L.PREC_BF16, 8, out.ctypes.data, status.ctypes.data)
    else:
        out = np.zeros((N, 224, 224, 3), np.uint8) if sink == "u8_dev" else np.zeros((N, HEAD), np.float32)
        d = ctx.malloc(out.nbytes)
        try:
            if sink == "u8_dev":
                rc = lib.icl_load_images_224_dev(ctx.h, arr, N, 8, ctypes.c_void_p(d), status.ctypes.data)
            else:
                rc = lib.icl_embed_files_dev(ctx.h, arr, N, HEAD, L.PREC_BF16, 8, ctypes.c_void_p(d), status.ctypes.data)
            ctx.d2h(out, d)
        finally:
            ctx.free(d)
    return rc, ctx.last_error(), status, out, ctx.last_ingest_stats(), ctx.last_entropy_stats()


@pytest.fixture(scope="module")
def runs(L, ctx, want):
    out = {}
    try:
        for mode in ("host", "gpu"):
            ctx.set_ingest_options(L.ENTROPY_GPU if mode == "gpu" else L.ENTROPY_HOST)
            for sink in ("u8_dev", "emb_host", "emb_dev"):
                out[mode, sink] = _call(L, ctx, want, sink)
    finally:
        ctx.set_ingest_options(L.ENTROPY_HOST)
    return out


MODES = pytest.mark.parametrize("mode", ["host", "gpu"])


@MODES
def test_good_rows_bit_identical(want, runs, mode):
    good = want["good"]
    assert len(good) == N - len(MISSING) - 1 + want["bad_ok"]
    assert np.array_equal(runs[mode, "u8_dev"][3][good], want["rows"][good])
    assert np.array_equal(runs[mode, "emb_host"][3][good], want["emb"])
    assert np.array_equal(runs[mode, "emb_dev"][3][good], want["emb"])


@MODES
def test_failed_rows(want, runs, mode):
    failed = np.flatnonzero(want["status"])
    assert set(MISSING) <= set(failed.tolist())
    assert not runs[mode, "u8_dev"][3][failed].any()
    assert np.isnan(runs[mode, "emb_host"][3][failed]).all()
    assert np.isnan(runs[mode, "emb_dev"][3][failed]).all()


def test_status_equal_across_sinks_and_modes(want, runs):
    for key, r in runs.items():
        assert np.array_equal(r[2], want["status"]), key


def test_code_and_message_name_row_0(L, want, runs):
    for key, r in runs.items():
        assert r[0] == L.ICL_ERR_IO == want["status"][0], key
        assert "file 0 of %d" % N in r[1] and "missing0.jpg" in r[1], (key, r[1])
    assert len({r[1].split(": ", 1)[1] for r in runs.values()}) == 1  # the same text behind each entry point's name


@MODES
def test_stats_add_up(want, runs, mode):
    nfail = int((want["status"] != 0).sum())
    jpegs = N - len(MISSING) - 1  # every readable file but the PNG
    for sink in ("u8_dev", "emb_host", "emb_dev"):
        ing, ent = runs[mode, sink][4], runs[mode, sink][5]
        assert ing["host_files"] == 1 and ing["gpu_jpegs"] == jpegs - 1 + want["bad_ok"], (sink, ing)
        assert ing["gpu_jpegs"] + ing["host_files"] + nfail == N
        if mode == "gpu":  # the progressive file by host stage A, the rejected one redone (and counted there alone)
            assert (ent["gpu_entropy_jpegs"], ent["host_entropy_jpegs"], ent["redone_on_host"]) == (jpegs - 2, 1, 1), (sink, ent)
            assert ent["stream_bytes"] > 0
        else:
            assert (ent["gpu_entropy_jpegs"], ent["host_entropy_jpegs"], ent["redone_on_host"], ent["stream_bytes"]) == (0, jpegs, 0, 0), (sink, ent)
        assert ent["gpu_entropy_jpegs"] + ent["host_entropy_jpegs"] + ent["redone_on_host"] + 1 + len(MISSING) == N
