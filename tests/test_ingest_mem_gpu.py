"""Images from memory through the batched ingest, the coalescing queue and the request driver (icl_*_mem): for the same bytes every
memory call gives what its path twin gives for the bytes written to files -- rows, statuses, statistics, messages up to the image's
name -- BIT-EXACT (np.array_equal), in ICL_ENTROPY_HOST and ICL_ENTROPY_GPU.  No kernel is new: the tests compare two routes into the
same driver, and the statistics show that the route taken was the same (GPU rebuild, GPU entropy decoder, repair pass).
Images are 64x48 to 320x240 plus one 1920x1080 (a stream of more than one 256-subsequence workgroup); the model is the seeded synthetic one."""
import re
import threading

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_sampling_cases
from tests.jpeg_entropy_cases import damaged, picture, save_jpeg

pytestmark = pytest.mark.gpu

MODES = ["ENTROPY_HOST", "ENTROPY_GPU"]


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


@pytest.fixture
def mode(L, ctx, request):
    """The context in the entropy mode the test is parametrised with; back to the default afterwards."""
    ctx.set_ingest_options(getattr(L, request.param))
    yield request.param
    ctx.set_ingest_options(L.ENTROPY_HOST)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory, L):
    """About 40 images as (paths, buffers): the seven samplings (grey, 1x1, 2x1, 2x2, 1x2, 4x1, 1x4), progressive, PNG, PPM, an EXIF-rotated
    file, one 1080p file, streams the GPU entropy check rejects but host stage A reads, a garbage buffer and an empty one."""
    d = tmp_path_factory.mktemp("mem_gpu")
    paths = []
    for k, (w, h) in enumerate(((64, 48), (97, 61), (320, 240))):
        for sub in (0, 1, 2):
            paths.append(save_jpeg(d / ("b%d_s%d.jpg" % (k, sub)), w, h, 10 * k + sub, quality=80, subsampling=sub))
        paths.append(save_jpeg(d / ("g%d.jpg" % k), w, h, 10 * k + 3, quality=85, grey=True))
        paths.append(save_jpeg(d / ("p%d.jpg" % k), w, h, 10 * k + 4, quality=75, subsampling=2, progressive=True))
    for name, luma, src, size in (("v2.jpg", (1, 2), (64, 48), (41, 50)), ("h4.jpg", (4, 1), (64, 64), (45, 59)), ("v4.jpg", (1, 4), (64, 64), (59, 45))):
        paths.append(jpeg_sampling_cases.make(d, name, luma, src, size, seed=60 + len(paths))["path"])
    paths.append(jpeg_sampling_cases.make(d, "h4_o6.jpg", (4, 1), (64, 64), (45, 59), seed=70, orient=6)["path"])
    exif = Image.Exif()
    exif[0x0112] = 8
    paths.append(save_jpeg(d / "o8.jpg", 97, 61, 71, quality=85, subsampling=1, exif=exif.tobytes()))
    paths.append(save_jpeg(d / "rst.jpg", 160, 120, 72, quality=75, subsampling=2, restart_marker_blocks=3))
    paths.append(save_jpeg(d / "rst_rows.jpg", 97, 61, 77, quality=75, subsampling=1, restart_marker_rows=1))
    paths.append(save_jpeg(d / "opt_grey.jpg", 160, 120, 78, quality=80, grey=True, optimize=True))
    for o in (3, 5):
        exif[0x0112] = o
        paths.append(save_jpeg(d / ("o%d.jpg" % o), 97, 61, 78 + o, quality=85, subsampling=2, exif=exif.tobytes()))
    paths.append(save_jpeg(d / "prog_444.jpg", 160, 120, 90, quality=80, subsampling=0, progressive=True))
    paths.append(save_jpeg(d / "q95.jpg", 320, 240, 91, quality=95, subsampling=0))
    paths.append(save_jpeg(d / "opt.jpg", 160, 120, 73, quality=90, subsampling=0, optimize=True))
    paths.append(save_jpeg(d / "hd_1920x1080.jpg", 1920, 1080, 74, quality=75, subsampling=2))
    pic = picture(97, 61, 75)
    for m in ("RGB", "P", "LA"):
        Image.fromarray(pic).convert(m).save(str(d / ("c_%s.png" % m)))
        paths.append(str(d / ("c_%s.png" % m)))
    (d / "c.ppm").write_bytes(b"P6\n97 61\n255\n" + pic.tobytes())
    paths.append(str(d / "c.ppm"))
    dm = {p.split("/")[-1]: p for p in damaged(d)}  # 300x200 streams: truncated or with a flipped byte
    paths += [dm["trunc_plain_1.jpg"], dm["flip_rst_1.jpg"], dm["trunc_opt_2.jpg"], dm["flip_plain_1.jpg"]]
    (d / "garbage.bin").write_bytes(np.random.default_rng(76).integers(0, 256, 5000, dtype=np.uint8).tobytes())
    paths.append(str(d / "garbage.bin"))
    (d / "empty.jpg").write_bytes(b"")
    paths.append(str(d / "empty.jpg"))
    paths.append(paths[0])
    bufs = [open(p, "rb").read() for p in paths]
    forms = [bytes, bytearray, memoryview, lambda b: np.frombuffer(b, np.uint8)]  # every accepted form of a buffer
    return paths, [forms[i % 4](b) for i, b in enumerate(bufs)]


@pytest.fixture(scope="module")
def repairable(L, mixed):
    """Indices of the images the GPU entropy check rejects although host stage A reads them (decided by the host loop over the same
    subsequences, jpeg_coefs_file_host, and the host decoder)."""
    out = []
    for i, p in enumerate(mixed[0]):
        if p.endswith(".jpg") and "empty" not in p and L.jpeg_coefs_file_host(p, 1024)[1]["state"] == 0:
            try:
                L.load_image_224(p)
                out.append(i)
            except L.ICLError:
                pass
    assert len(out) >= 2, "the corpus must hold streams for the repair pass"
    return out


def stats(ctx):
    a, b = ctx.last_ingest_stats(), ctx.last_entropy_stats()
    return ({k: a[k] for k in ("gpu_jpegs", "host_files", "upload_bytes")},
            {k: b[k] for k in ("gpu_entropy_jpegs", "host_entropy_jpegs", "redone_on_host", "stream_bytes")})


def mem_message(msg, paths, bufs, path_call, mem_call):
    """A path call's message as its memory twin words it: the call's own name, and the path replaced by the name of the memory image
    at that index."""
    i = int(re.search(r"file (\d+) of", msg).group(1))
    assert msg.startswith(path_call + ": ") and paths[i] in msg, msg
    return mem_call + msg[len(path_call):].replace(paths[i], "image %d (in memory, %d bytes)" % (i, len(bufs[i])))


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_u8_rows(L, ctx, mixed, repairable, mode):
    paths, bufs = mixed
    want, wst = ctx.load_images_224(paths, threads=4)
    werr, wstats = ctx.last_error(), stats(ctx)
    got, st = ctx.load_images_224_mem(bufs, threads=4)
    err, gstats = ctx.last_error(), stats(ctx)
    assert list(st) == list(wst) and np.array_equal(got, want)
    assert gstats == wstats, (gstats, wstats)
    failed = np.flatnonzero(st)
    assert len(failed) >= 3 and (st[-3:-1] == L.ICL_ERR_IO).all() and not got[failed].any()  # garbage and empty among them; zero rows
    assert err == mem_message(werr, paths, bufs, "icl_load_images_224_dev", "icl_load_images_224_mem_dev") and "image %d (in memory" % failed[0] in err
    ok = np.flatnonzero(st == 0)
    assert np.array_equal(got[ok], np.stack([L.load_image_224(paths[i]) for i in ok]))  # and both equal the host path
    if mode == "ENTROPY_GPU":
        assert gstats[1]["redone_on_host"] >= len(repairable) and gstats[1]["gpu_entropy_jpegs"] >= 15, gstats
    else:
        assert gstats[1]["redone_on_host"] == 0 and gstats[1]["gpu_entropy_jpegs"] == 0 and gstats[1]["stream_bytes"] == 0, gstats
    assert gstats[0]["host_files"] == 4 and gstats[0]["gpu_jpegs"] >= 25, gstats  # three PNGs and the PPM on the host


def test_lowest_failed_index_and_empty_sources(L, ctx, mixed):
    paths, bufs = mixed
    lst = [bufs[0], None, b"", bufs[1], bytearray()]
    got, st = ctx.load_images_224_mem(lst, threads=2)
    assert list(st) == [0, L.ICL_ERR_IO, L.ICL_ERR_IO, 0, L.ICL_ERR_IO]
    assert ctx.last_error() == "icl_load_images_224_mem_dev: file 1 of 5: failed to read image: image 1 (in memory, 0 bytes). empty image buffer"
    assert np.array_equal(got[0], L.load_image_224(paths[0])) and np.array_equal(got[3], L.load_image_224(paths[1])) and not got[[1, 2, 4]].any()


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("head,prec", [(1000, "PREC_BF16"), (2048, "PREC_BF16"), (1000, "PREC_FP32"), (2048, "PREC_FP32")])
def test_embedding_rows_host_and_dev(L, ctx, mixed, mode, head, prec):
    paths, bufs = mixed
    prec = getattr(L, prec)
    want, wst = ctx.embed_files(paths, head, prec, 4)
    werr, wstats = ctx.last_error(), stats(ctx)
    got, st = ctx.embed_images_mem(bufs, head, prec, 4)
    assert list(st) == list(wst) and ctx.last_error() == mem_message(werr, paths, bufs, "icl_embed_files", "icl_embed_images_mem") and stats(ctx) == wstats
    assert np.array_equal(got, want, equal_nan=True)
    failed = st != 0
    assert np.isnan(got[failed]).all() and np.isfinite(got[~failed]).all() and failed.sum() >= 3
    d = ctx.malloc(len(bufs) * head * 4)
    try:
        std = ctx.embed_images_mem_dev(bufs, d, head, prec, 4)
        dev = np.empty_like(got)
        ctx.d2h(dev, d)
    finally:
        ctx.free(d)
    assert list(std) == list(wst) and np.array_equal(dev, want, equal_nan=True) and stats(ctx) == wstats


def test_repair_pass_reads_the_callers_buffer_again(L, ctx, mixed, repairable):
    """A stream the GPU check rejects is decoded a second time, by host stage A, from the same memory: its row equals the host mode's."""
    paths, bufs = mixed
    sub = [bufs[i] for i in repairable] + [bufs[0]]
    ctx.set_ingest_options(L.ENTROPY_HOST)
    want, wst = ctx.embed_images_mem(sub, L.HEAD_DENSE0, L.PREC_FP32, 2)
    assert (wst == 0).all() and ctx.last_entropy_stats()["redone_on_host"] == 0
    ctx.set_ingest_options(L.ENTROPY_GPU)
    try:
        got, st = ctx.embed_images_mem(sub, L.HEAD_DENSE0, L.PREC_FP32, 2)
        es = ctx.last_entropy_stats()
    finally:
        ctx.set_ingest_options(L.ENTROPY_HOST)
    assert (st == 0).all() and np.array_equal(got, want)
    assert es["redone_on_host"] == len(repairable) and es["gpu_entropy_jpegs"] == 1, es
    assert np.array_equal(want[:-1], ctx.embed_u8(np.stack([L.load_image_224(paths[i]) for i in repairable]), L.HEAD_DENSE0, L.PREC_FP32))


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_slab_seams(L, ctx, mixed, mode):
    """301 images -- the same 12 buffers over and over: the pointers repeat, which the interface allows -- cut at least two slabs of 256
    rows; the output does not depend on the number of host threads and every row is its buffer's."""
    paths, bufs = mixed
    pick = [i for i, p in enumerate(paths) if "1920" not in p and "src_" not in p][:10] + [len(paths) - 3, len(paths) - 2]  # ... garbage, empty
    want, wst = ctx.load_images_224([paths[i] for i in pick], threads=2)
    lst = [bufs[pick[k % 12]] for k in range(301)]
    ref = None
    for threads in (1, 3, 16):
        got, st = ctx.load_images_224_mem(lst, threads=threads)
        for k in range(301):
            assert st[k] == wst[k % 12] and np.array_equal(got[k], want[k % 12]), (threads, k)
        cur = stats(ctx)
        cur[0].pop("upload_bytes")
        assert ref is None or cur == ref, (threads, cur, ref)
        ref = cur
    assert ref[0]["gpu_jpegs"] + ref[0]["host_files"] == 301 - 2 * 25  # (k % 12 == 10 and 11: the garbage and the empty buffer, 25 times each)


def test_coalescing_queue_mixes_path_and_memory_callers(L, ctx, mixed):
    paths, bufs = mixed
    ok = [i for i, p in enumerate(paths) if "1920" not in p and "garbage" not in p and "empty" not in p][:16]
    want = ctx.embed_u8(np.stack([L.load_image_224(paths[i]) for i in ok]), L.HEAD_DENSE0, L.PREC_FP32)
    assert np.array_equal(ctx.embed_image_mem(bufs[ok[0]], L.HEAD_DENSE0), want[0])  # one at a time
    ctx.set_file_options(L.PREC_FP32, 20000, 64)
    before = ctx.file_batch_stats()
    out, res = [None] * 16, [None] * 16
    gate = threading.Barrier(16)

    def worker(k):
        gate.wait()
        try:
            out[k] = ctx.embed_image_mem(bufs[ok[k]], L.HEAD_DENSE0) if k % 2 else ctx.embed_file(paths[ok[k]], L.HEAD_DENSE0)
            res[k] = "ok"
        except L.ICLError as e:
            res[k] = e.code

    def run():
        th = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(16)]
        for t in th:
            t.start()
        for t in th:
            t.join(60)
        assert not any(t.is_alive() for t in th), "a caller is still blocked"

    try:
        run()
        assert res == ["ok"] * 16
        for k in range(16):
            assert np.array_equal(out[k], want[k]), k
        st = ctx.file_batch_stats()
        assert st["images"] - before["images"] == 16 and st["batches"] - before["batches"] < 16, (st, before)
        ctx.set_file_options(L.PREC_FP32 | L.FILE_FAIL_NEXT_LEADER, 20000, 64)  # one leader gives up with its whole batch
        run()
        failed = [k for k in range(16) if res[k] != "ok"]
        assert failed and all(res[k] == L.ICL_ERR_NOMEM for k in failed), res  # every caller of that batch, path or memory
        assert any(k % 2 for k in failed) or len(failed) == 1
        ctx.set_file_options(L.PREC_FP32, 0, 256)
        assert np.array_equal(ctx.embed_image_mem(bufs[ok[1]], L.HEAD_DENSE0), want[1])  # the following call succeeds
        with pytest.raises(L.ICLError) as ei:
            ctx.embed_image_mem(b"", L.HEAD_DENSE0)
        assert ei.value.code == L.ICL_ERR_IO and "image 0 (in memory, 0 bytes). empty image buffer" in str(ei.value)
    finally:
        ctx.set_file_options(L.PREC_FP32, 2000, 256)


def make_requests(items, rng):
    """6 requests over consecutive runs of items: n in [8, 24], L in [0, 20], min 3 / max 6; request 2 holds an undecodable image,
    request 4 has constraints that cannot be met (min 5 / max 5 over a count no multiple fits)."""
    ns, Ls = [8, 13, 24, 9, 11, 17], [0, 20, 4, 7, 1, 12]
    reqs, at = [], 0
    for r, (n, nl) in enumerate(zip(ns, Ls)):
        labels = [sorted(int(j) for j in rng.integers(0, nl, int(rng.integers(1, 3)))) if nl else [] for _ in range(n)]
        mn, mx = (5, 5) if r == 4 else (3, 6)
        reqs.append((items[at:at + n], labels, nl, mn, mx))
        at += n
    return reqs


@pytest.fixture(scope="module")
def request_images(tmp_path_factory):
    d = tmp_path_factory.mktemp("mem_req")
    paths = [save_jpeg(d / ("r%02d.jpg" % i), 64 + 8 * (i % 5), 48 + 4 * (i % 3), 500 + i, quality=75 + i % 20, subsampling=i % 3) for i in range(82)]
    (d / "bad.jpg").write_bytes(b"\xff\xd8" + bytes(300))
    paths[8 + 13 + 5] = str(d / "bad.jpg")  # inside request 2
    return paths, [open(p, "rb").read() for p in paths]


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_requests(L, ctx, request_images, mode):
    paths, bufs = request_images
    want = ctx.cluster_requests(make_requests(paths, np.random.default_rng(9)), L.HEAD_DENSE0, L.PREC_FP32, 4, want_merges=True, want_E=True)
    wfst, wrc, werr, wstats = ctx.last_file_status, ctx.last_requests_rc, ctx.last_error(), stats(ctx)
    got = ctx.cluster_requests_mem(make_requests(bufs, np.random.default_rng(9)), L.HEAD_DENSE0, L.PREC_FP32, 4, want_merges=True, want_E=True)
    assert [w[3] for w in want] == [0, 0, L.ICL_ERR_IO, 0, L.ICL_ERR_CONSTRAINT, 0]
    assert ctx.last_requests_rc == wrc == L.ICL_ERR_IO and list(ctx.last_file_status) == list(wfst) and stats(ctx) == wstats
    i = 8 + 13 + 5
    assert ctx.last_error() == werr.replace("icl_cluster_requests:", "icl_cluster_requests_mem:").replace(paths[i], "image %d (in memory, %d bytes)" % (i, len(bufs[i])))
    for r, (g, w) in enumerate(zip(got, want)):
        cid, rank, nc, st, mg, E = g
        assert np.array_equal(cid, w[0]) and np.array_equal(rank, w[1]) and nc == w[2] and st == w[3] and np.array_equal(mg, w[4]), r
        assert np.array_equal(E, w[5], equal_nan=True), r
    assert got[0][2] > 0 and (got[2][0] == -1).all() and (got[4][0] == -1).all()


def test_run_uploaded(L, ctx, request_images):
    from imageclust_amd import embeddings, workflow

    paths, bufs = request_images
    app = embeddings.AppContext(Net=embeddings.Net(ctx))
    labelSet = {"cat": 0, "dog": 1, "tree": 2}
    names = ["cat", "dog", "tree", "bird"]
    reqs, ups = [], []
    for r, (a, n) in enumerate([(0, 9), (9, 2), (30, 14)]):
        labels = [[names[(i + r) % 4]] for i in range(n)]
        ls = labelSet if r != 1 else {}
        reqs.append((paths[a:a + n], ["img_%d" % i for i in range(n)], labels, ls, 3, 6))
        ups.append(([("upload_%d.jpg" % i, bufs[a + i]) for i in range(n)], labels, ls, 3, 6))
    wcodes, codes = [], []
    want = workflow.RunRequests(app, reqs, prec=L.PREC_FP32, threads=4, statuses=wcodes)
    got = workflow.RunUploaded(app, ups, prec=L.PREC_FP32, threads=4, statuses=codes)
    assert codes == wcodes == [0, L.ICL_ERR_CONSTRAINT, 0] and got == want
    assert sorted(m for ms in got[0][0].values() for m in ms) == sorted("img_%d" % i for i in range(9))
    emb, err = embeddings.GetImageEmbeddingBytes(app, bufs[0])
    assert err is None and np.array_equal(emb, embeddings.GetImageEmbedding(app, paths[0])[0])
    emb, err = embeddings.GetImageEmbeddingBytes(app, b"\xff\xd8")
    assert emb is None and "image 0 (in memory, 2 bytes)" in err


def test_call_level_errors_leave_status_untouched(L, request_images):
    paths, bufs = request_images
    c = L.Context(0)  # no model loaded
    try:
        with pytest.raises(L.ICLError) as ei:
            c.cluster_requests_mem(make_requests(bufs, np.random.default_rng(9)))
        assert ei.value.code == L.ICL_ERR_NOMODEL
        import ctypes as C

        lib = L.load()
        one = (C.c_int32 * 1)(1)
        zero = (C.c_int32 * 1)(0)
        off = (C.c_int64 * 2)(0, 0)
        mn, mx = (C.c_int32 * 1)(1), (C.c_int32 * 1)(1)
        cid, rank, nc, nm, st = ((C.c_int32 * 1)(-7) for _ in range(5))
        data, size, _, keep = L._byte_arrays([bufs[0]])
        args = lambda d, s, n: (c.h, 1, d, s, n, zero, off, None, mn, mx, L.HEAD_DENSE0, L.PREC_FP32, 0, cid, rank, nc, nm, None, st, None, None)
        assert lib.icl_cluster_requests_mem(*args(data, size, one)) == L.ICL_ERR_NOMODEL and st[0] == -7
        assert lib.icl_cluster_requests_mem(*args(None, size, one)) == L.ICL_ERR_ARG and st[0] == -7  # a null data array
        assert lib.icl_cluster_requests_mem(*args(data, None, one)) == L.ICL_ERR_ARG and st[0] == -7  # a null bytes array
        assert [cid[0], rank[0], nc[0], nm[0]] == [-7] * 4
        out = np.zeros(1000, np.float32)
        stat = np.full(1, -7, np.int32)
        assert lib.icl_embed_images_mem(c.h, None, size, 1, 1000, 0, 0, out.ctypes.data, stat.ctypes.data) == L.ICL_ERR_ARG
        assert lib.icl_embed_images_mem(c.h, data, None, 1, 1000, 0, 0, out.ctypes.data, stat.ctypes.data) == L.ICL_ERR_ARG
        assert lib.icl_embed_images_mem(c.h, data, size, -1, 1000, 0, 0, out.ctypes.data, stat.ctypes.data) == L.ICL_ERR_ARG
        assert lib.icl_embed_images_mem(c.h, data, size, 1, 1000, 0, 0, out.ctypes.data, stat.ctypes.data) == L.ICL_ERR_NOMODEL
        assert lib.icl_load_images_224_mem_dev(c.h, None, size, 1, 0, None, stat.ctypes.data) == L.ICL_ERR_ARG
        assert stat[0] == -7 and not out.any()
        del keep
    finally:
        c.close()


@pytest.mark.parametrize("entropy", MODES)
def test_coefficients(L, ctx, mixed, entropy):
    """jpeg_coefs_mem against jpeg_coefs_files on the JPEGs host stage A reads (a file it cannot read fails either call)."""
    paths, bufs = mixed
    idx = [i for i, p in enumerate(paths) if p.endswith(".jpg") and "empty" not in p]
    good = []
    for i in idx:
        try:
            L.load_image_224(paths[i])
            good.append(i)
        except L.ICLError:
            pass
    assert len(good) >= 25
    e = getattr(L, entropy)
    want, wstate = ctx.jpeg_coefs_files([paths[i] for i in good], e)
    got, state = ctx.jpeg_coefs_mem([bufs[i] for i in good], e)
    assert list(state) == list(wstate) and len(got) == len(want)
    for g, w, i in zip(got, want, good):
        assert g.shape == w.shape and np.array_equal(g, w), paths[i]
    if entropy == "ENTROPY_GPU":
        assert set(state) == {1, 0, -1}  # accepted, rejected by the check, not qualifying (progressive)
    else:
        assert (state == 1).all()
        with pytest.raises(L.ICLError) as ei:
            ctx.jpeg_coefs_mem([bufs[good[0]], b"P6 garbage"], e)
        assert ei.value.code == L.ICL_ERR_IO and "image 1 (in memory, 10 bytes) is not a readable JPEG" in str(ei.value)
