"""PNG on the GPU in batched file ingest (ICL_PNG_GPU; png_gpu.hip behind jpeg_gpu.hip): rows, status codes and messages are those of the
host mode for every file of tests/png_gpu_cases.py, good or bad; the counters show that the GPU route really ran (no image of a clean
case may fall back) and that every reject went through the repair pass; the test hook names the stage when something differs."""
import numpy as np
import pytest

from tests import png_gpu_cases
from tests.jpeg_entropy_cases import picture, save_jpeg

pytestmark = pytest.mark.gpu


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
    return png_gpu_cases.write_all(tmp_path_factory.mktemp("png_gpu_cases"))


def in_mode(ctx, L, png, fn, entropy=None):
    """fn() with the context in the given PNG (and entropy) mode -> (its result, last_error, png stats, ingest stats)"""
    ctx.set_png_options(png)
    if entropy is not None:
        ctx.set_ingest_options(entropy)
    try:
        r = fn()
        return r, ctx.last_error(), ctx.last_png_stats(), ctx.last_ingest_stats()
    finally:
        ctx.set_png_options(L.PNG_HOST)
        ctx.set_ingest_options(L.ENTROPY_HOST)


@pytest.fixture(scope="module")
def clean(L, ctx, corpus):
    """the clean cases and their rows in host mode (computed once)"""
    cs = [c for c in corpus if c["kind"] == "clean"]
    paths = [c["path"] for c in cs]
    (rows, status), _, st, ing = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.load_images_224(paths, threads=8))
    assert (status == 0).all() and st["gpu_pngs"] == 0 and st["host_pngs"] == len(cs) and ing["host_files"] == len(cs), (st, ing)
    rows.setflags(write=False)
    return cs, paths, rows


def test_clean_cases_rows_and_counters(L, ctx, clean):
    cs, paths, want = clean
    (got, status), _, st, ing = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224(paths, threads=8))
    assert (status == 0).all()
    bad = [cs[i]["name"] for i in range(len(cs)) if not np.array_equal(got[i], want[i])]
    assert not bad, "rows differ from the host mode: %s" % bad
    # a silent fallback would hide a wrong kernel: no image may fall back
    assert st["gpu_pngs"] == len(cs) and st["redone_on_host"] == 0 and st["host_pngs"] == 0 and st["stream_bytes"] > 0, st
    assert ing["gpu_jpegs"] == 0 and ing["host_files"] == 0, ing


@pytest.mark.parametrize("stage", [0, 1])
def test_stages_equal_the_host_schedule(L, ctx, clean, stage):
    cs, paths, _ = clean
    got, state = ctx.png_raw_files(paths, stage)
    for i, c in enumerate(cs):
        want, info = L.png_raw_file_host(c["path"], stage)
        assert info["state"] == 1
        assert state[i] == 1 and np.array_equal(got[i], want), "stage %d of %s" % (stage, c["name"])


def test_reject_cases(L, ctx, corpus):
    cs = [c for c in corpus if c["kind"] == "reject"]
    paths = [c["path"] for c in cs]
    _, state = ctx.png_raw_files(paths, 1)
    assert (state == 0).all(), dict(zip((c["name"] for c in cs), state))
    (hrows, hstatus), herr, _, _ = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.load_images_224(paths, threads=4))
    (grows, gstatus), gerr, st, ing = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224(paths, threads=4))
    assert (hstatus != 0).all() and np.array_equal(gstatus, hstatus) and np.array_equal(grows, hrows) and not grows.any()
    assert gerr == herr and cs[0]["message"] in gerr
    assert st["redone_on_host"] == len(cs) and st["gpu_pngs"] == 0 and st["host_pngs"] == 0 and ing["host_files"] == 0, (st, ing)
    for c in cs:  # every file's own message
        (_, hs), herr, _, _ = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.load_images_224([c["path"]]))
        (_, gs), gerr, st, _ = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224([c["path"]]))
        assert gs[0] == hs[0] != 0 and gerr == herr and ("PNG: " + c["message"]) in gerr and st["redone_on_host"] == 1, c["name"]


@pytest.mark.parametrize("entropy", ["ENTROPY_HOST", "ENTROPY_GPU"])
def test_mixed_list(L, ctx, corpus, tmp_path, entropy):
    by = {c["name"]: c["path"] for c in corpus}
    ppm = tmp_path / "p.ppm"
    ppm.write_bytes(b"P6\n9 7\n255\n" + picture(9, 7, 3).tobytes())
    paths = [save_jpeg(tmp_path / "base.jpg", 67, 45, 1, quality=80, subsampling=2),
             save_jpeg(tmp_path / "prog.jpg", 67, 45, 2, quality=80, subsampling=2, progressive=True),
             by["blocks_dynamic"], by["unqualified_adam7"], str(ppm), str(tmp_path / "missing.png"), by["reject_adler"], by["filters_random_301x203"],
             by["blocks_dynamic"]]
    (hrows, hstatus), herr, _, _ = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.load_images_224(paths, threads=4))
    (grows, gstatus), gerr, st, ing = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224(paths, threads=4), getattr(L, entropy))
    assert np.array_equal(gstatus, hstatus) and np.array_equal(grows, hrows) and gerr == herr
    assert [int(s != 0) for s in gstatus] == [0, 0, 0, 0, 0, 1, 1, 0, 0]
    for i, p in enumerate(paths):  # row i belongs to path i
        if gstatus[i] == 0:
            assert np.array_equal(grows[i], L.load_image_224(p)), p
    assert np.array_equal(grows[2], grows[8]) and not np.array_equal(grows[2], grows[7])
    assert st["gpu_pngs"] == 3 and st["host_pngs"] == 1 and st["redone_on_host"] == 1, st
    assert ing["gpu_jpegs"] == 2 and ing["host_files"] == 2, ing
    assert ing["gpu_jpegs"] + ing["host_files"] + st["gpu_pngs"] + int((gstatus != 0).sum()) == len(paths)


def test_more_than_one_slab_memory_sources_embeddings_and_requests(L, ctx, clean):
    cs, paths, rows = clean
    small = [i for i, c in enumerate(cs) if len(c["data"]) < 20000]
    pick = [small[k % len(small)] for k in range(300)]  # more than one slab of 256 rows
    many = [paths[i] for i in pick]
    (got, status), _, st, _ = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224(many, threads=8))
    assert (status == 0).all() and st["gpu_pngs"] == 300 and st["redone_on_host"] == 0, st
    for k, i in enumerate(pick):
        assert np.array_equal(got[k], rows[i]), (k, cs[i]["name"])
    bufs = [cs[i]["data"] for i in pick[:40]]
    (got, status), _, st, _ = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224_mem(bufs, threads=4))
    assert (status == 0).all() and st["gpu_pngs"] == 40 and np.array_equal(got, rows[pick[:40]]), st
    (Eh, sh), _, _, _ = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.embed_files(many, L.HEAD_POOLED, L.PREC_BF16, 8))
    (Eg, sg), _, st, _ = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.embed_files(many, L.HEAD_POOLED, L.PREC_BF16, 8))
    assert (sh == 0).all() and (sg == 0).all() and st["gpu_pngs"] == 300 and np.array_equal(Eg, Eh)
    reqs = [(many[:12], [[] for _ in range(12)], 0, 2, 6)]
    host, _, _, _ = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.cluster_requests(reqs, L.HEAD_DENSE0, L.PREC_BF16, threads=4, want_E=True))
    gpu, _, st, _ = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.cluster_requests(reqs, L.HEAD_DENSE0, L.PREC_BF16, threads=4, want_E=True))
    assert st["gpu_pngs"] == 12 and len(host) == len(gpu) == 1
    for a, b in zip(host[0], gpu[0]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_jpeg_only_list_is_untouched(L, ctx, tmp_path):
    paths = [save_jpeg(tmp_path / ("j%d.jpg" % k), 64 + 9 * k, 48 + 5 * k, k, quality=80, subsampling=k % 3) for k in range(6)]
    (hrows, hstatus), _, hst, hing = in_mode(ctx, L, L.PNG_HOST, lambda: ctx.load_images_224(paths, threads=4))
    (grows, gstatus), _, gst, ging = in_mode(ctx, L, L.PNG_GPU, lambda: ctx.load_images_224(paths, threads=4))
    assert np.array_equal(grows, hrows) and np.array_equal(gstatus, hstatus) and (gstatus == 0).all()
    assert {k: v for k, v in ging.items() if k != "host_decode_s"} == {k: v for k, v in hing.items() if k != "host_decode_s"}
    assert gst == {"gpu_pngs": 0, "host_pngs": 0, "redone_on_host": 0, "stream_bytes": 0} == hst
