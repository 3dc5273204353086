"""The batched downsizer's driver (jpeg_gpu.hip, icl_downsize_images[_mem]) across its round boundaries: a round closes when the slab
holds SLAB_IMAGES = 256 GPU-rebuilt JPEGs, so a list of 520 sources runs as three rounds.  The filler alternates two over-limit baseline
JPEGs, one done in one attempt and one that needs the second; a passthrough, a host-decoded image that needs a second attempt, a
progressive JPEG, a missing source and a damaged JPEG that the GPU entropy check rejects stand at the first and last row and directly
before and after the 256th and the 512th GPU-rebuilt JPEG (positions found by counting the rows that occupy a slab row, per entropy
mode: passthrough, host-decoded and failed rows do not).  Bytes, statuses, the call's code and message and the statistics must be what
the one-image host call (icl_downsize_image_mem, pinned to Pillow in test_downsize_cpu.py) gives, in both entropy modes, for paths and
for memory sources.

Not covered: a round also closes after 2 * SLAB_PAYLOAD (256 MiB) of finished results (passthroughs, whole-on-host outputs); no
few-second test reaches that."""
import faulthandler

import numpy as np
import pytest

from tests.downsize_cases import _save, noise_ppm, sources
from tests.jpeg_entropy_cases import damaged, picture

pytestmark = pytest.mark.gpu
MAX_BYTES, MAX_DIM = 7000, 96
N, SLAB_IMAGES, THREADS = 520, 256, 8
FILL = ("one", "two")
# what stands at the first row, before / after the 256th, before / after the 512th GPU-rebuilt JPEG, and at the last row
SPECIALS = ("missing", "small", "second_ppm", "damaged", "progressive", "missing")


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def _layout(occupies):
    """The list as source names, and the rows of the specials.  occupies[name]: the source takes a slab row (a GPU-rebuilt JPEG)."""
    names, at, g = [], [], 0

    def put(name):
        nonlocal g
        names.append(name)
        g += occupies[name]

    def special(k):
        at.append(len(names))
        put(SPECIALS[k])

    def fill_to(count):
        while g < count:
            put(FILL[len(names) % 2])

    special(0)
    for k, boundary in ((1, SLAB_IMAGES), (3, 2 * SLAB_IMAGES)):
        fill_to(boundary - 1)
        special(k)  # directly before the boundary's JPEG (or, where the special takes a slab row, that JPEG itself)
        fill_to(boundary)
        special(k + 1)
    while len(names) < N - 1:
        put(FILL[len(names) % 2])
    special(5)
    assert len(names) == N and g > 2 * SLAB_IMAGES and at[0] == 0 and at[5] == N - 1, (len(names), g, at)
    return names, at


@pytest.fixture(scope="module")
def want(L, tmp_path_factory):
    """Every distinct source with what the one-image host call makes of it, and per entropy mode the list built from them."""
    d = tmp_path_factory.mktemp("dzseams")
    S = sources()
    bad = next(p for p in damaged(d) if L.jpeg_coefs_file_host(p, 1024)[1]["state"] == 0)  # qualifies, and the check rejects it
    data = {
        "one": S["jpeg_420"],
        "two": _save(np.random.default_rng(3).integers(0, 256, (300, 300, 3), dtype=np.uint8), "JPEG", quality=95),
        "small": _save(picture(97, 61, 40), "JPEG", quality=85),
        "second_ppm": noise_ppm(260, 260, 4),
        "progressive": S["jpeg_progressive"],
        "damaged": open(bad, "rb").read(),
        "missing": None,
    }
    path, out, code, info = {}, {}, {}, {}
    for name, b in data.items():
        path[name] = str(d / (name + ".bin"))
        if b is not None:
            open(path[name], "wb").write(b)
        try:
            if b is None:  # (the missing source: the host call on its path)
                out[name], info[name] = L.downsize_image(path[name], MAX_BYTES, MAX_DIM, want_info=True)
            else:
                out[name], info[name] = L.downsize_image_mem(b, MAX_BYTES, MAX_DIM, want_info=True)
            code[name] = 0
        except L.ICLError as e:
            out[name], info[name], code[name] = b"", None, e.code
    assert info["one"]["attempts"] == 1 and info["two"]["attempts"] == 2 and info["second_ppm"]["attempts"] == 2
    assert info["small"]["passthrough"] and len(data["small"]) <= MAX_BYTES and code["progressive"] == 0 and code["missing"] == L.ICL_ERR_IO
    assert all(len(data[k]) > MAX_BYTES for k in ("one", "two", "second_ppm", "progressive", "damaged"))
    bad_ok = code["damaged"] == 0  # (whichever it is, the host call's result is what the batched call must give)
    assert (len(out["damaged"]) > 0) == bad_ok
    lists = {}
    for mode in ("host", "gpu"):
        occ = {k: 1 for k in ("one", "two", "progressive")}
        occ.update({k: 0 for k in ("missing", "small", "second_ppm")})
        occ["damaged"] = 1 if mode == "gpu" or bad_ok else 0  # its stream goes to the GPU check; host stage A takes it or fails it
        lists[mode] = _layout(occ)
    return {"data": data, "path": path, "out": out, "code": code, "info": info, "bad_ok": bad_ok, "lists": lists}


@pytest.fixture(scope="module")
def runs(L, ctx, want):
    """(entropy mode, entry point) -> (files, status, message, statistics) of one batched call over the mode's list."""
    got = {}
    faulthandler.dump_traceback_later(300, exit=True)  # a hang fails the run instead of stalling it
    try:
        for mode in ("host", "gpu"):
            ctx.set_ingest_options(L.ENTROPY_GPU if mode == "gpu" else L.ENTROPY_HOST)
            names = want["lists"][mode][0]
            files, status = ctx.downsize_images([want["path"][k] for k in names], MAX_BYTES, MAX_DIM, THREADS)
            got[mode, "paths"] = (files, status, ctx.last_error(), ctx.last_downsize_stats())
            files, status = ctx.downsize_images_mem([want["data"][k] for k in names], MAX_BYTES, MAX_DIM, THREADS)
            got[mode, "mem"] = (files, status, ctx.last_error(), ctx.last_downsize_stats())
    finally:
        ctx.set_ingest_options(L.ENTROPY_HOST)
        faulthandler.cancel_dump_traceback_later()
    return got


CASES = pytest.mark.parametrize("mode,entry", [(m, e) for m in ("host", "gpu") for e in ("paths", "mem")])


def test_specials_stand_at_the_round_boundaries(want):
    for mode, (names, at) in want["lists"].items():
        occ = [k in ("one", "two", "progressive") or (k == "damaged" and (mode == "gpu" or want["bad_ok"])) for k in names]
        nth = np.cumsum(occ)  # nth[i]: GPU-rebuilt JPEGs in rows 0 .. i
        assert [names[i] for i in at] == list(SPECIALS)
        for k, boundary in ((1, SLAB_IMAGES), (3, 2 * SLAB_IMAGES)):
            j = int(np.flatnonzero(nth == boundary)[0])  # the row of the boundary's JPEG
            assert at[k] in (j - 1, j) and at[k + 1] == j + 1, (mode, boundary, j, at)
        assert nth[-1] > 2 * SLAB_IMAGES  # three rounds


@CASES
def test_every_image_equals_host_call(want, runs, mode, entry):
    names = want["lists"][mode][0]
    files = runs[mode, entry][0]
    assert len(files) == N
    for i, k in enumerate(names):
        assert files[i] == want["out"][k], "row %d (%s): %d bytes against the host call's %d" % (i, k, len(files[i]), len(want["out"][k]))


@CASES
def test_status_code_and_message(want, runs, mode, entry):
    names = want["lists"][mode][0]
    _, status, msg, _ = runs[mode, entry]
    codes = [want["code"][k] for k in names]
    assert list(status) == codes
    lowest = next(i for i, c in enumerate(codes) if c)
    assert lowest == 0 and "file %d of %d" % (lowest, N) in msg, msg


def test_return_code_is_the_lowest_failed_rows(L, ctx, want):
    """The raw call over the list with its first row made good: the code and the message name the next failed row."""
    names = list(want["lists"]["host"][0])
    names[0] = "small"
    codes = [want["code"][k] for k in names]
    lowest = next(i for i, c in enumerate(codes) if c)
    data, size, n, keep = L._byte_arrays([want["data"][k] for k in names])
    total = sum(len(want["out"][k]) for k in names)
    st, oo, out = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(total, np.uint8)
    faulthandler.dump_traceback_later(300, exit=True)
    try:
        rc = L.load().icl_downsize_images_mem(ctx.h, data, size, n, MAX_BYTES, MAX_DIM, THREADS, out.ctypes.data, total, oo.ctypes.data, st.ctypes.data)
    finally:
        faulthandler.cancel_dump_traceback_later()
    del keep
    assert lowest > 0 and rc == codes[lowest] and list(st) == codes and oo[n] == total
    assert "file %d of %d" % (lowest, N) in ctx.last_error()


@CASES
def test_stats_add_up(want, runs, mode, entry):
    names = want["lists"][mode][0]
    files, _, _, st = runs[mode, entry]
    failed = sum(1 for k in names if want["code"][k])
    assert st["passthrough"] + st["gpu_rebuilt"] + st["host_decoded"] + failed == N, st
    assert st["bytes_out"] == sum(len(f) for f in files)
    assert st["bytes_in"] == sum(len(want["data"][k] or b"") for k in names)
    redone = 1 if mode == "gpu" and want["bad_ok"] else 0  # the rejected file: the host call redid it, so it counts as host-decoded
    on_gpu = sum(1 for k in names if k in ("one", "two", "progressive")) + (1 if mode == "host" and want["bad_ok"] else 0)
    assert st["passthrough"] == names.count("small")
    assert st["host_decoded"] == names.count("second_ppm") + redone, st
    assert st["gpu_rebuilt"] == on_gpu, st
    assert st["second_attempts"] == sum(1 for k in names if want["info"][k] and want["info"][k]["attempts"] == 2), st
