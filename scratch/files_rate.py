"""Files/s of the image-file ingest routes on one device, for two corpora written by Pillow on local disk:
4096 1920x1080 q75 baseline JPEGs and 512 4000x3000 q75 JPEGs (smooth photo-like content plus noise; the page cache is warmed by
reading every file once before timing).  Three configurations, all bf16, head 2048:
  (a) 16 host threads each calling icl_embed_file (one file per call: the route of workflow.go:156-175 today)
  (b) icl_embed_files with 16 host threads (stage A on the host, pixel rebuild + resize on the GPU)
  (c) icl_embed_u8 on the same images already decoded and resized (the ceiling)
plus icl_last_ingest_stats of (b) per image: host decode seconds, upload bytes.  Prints and writes one JSON object.

    python scratch/files_rate.py --out OUT.json
    python scratch/files_rate.py --trace-only --n1080 512     # (b) alone, e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import threading
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402

HEAD, PREC, THREADS = 2048, _lib.PREC_BF16, 16


def _write(job):
    path, w, h, seed = job
    from PIL import Image

    rng = np.random.default_rng(seed)
    y = np.linspace(0, 6.0 + (seed % 7), h, dtype=np.float32)[:, None]
    x = np.linspace(0, 9.0 + (seed % 5), w, dtype=np.float32)[None, :]
    base = np.stack([128 + 90 * np.sin(x * (1 + 0.3 * c) + y * (1 + 0.2 * c) + seed) for c in range(3)], -1)
    img = np.clip(base + rng.integers(-12, 13, (h, w, 3), dtype=np.int16), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(path, "JPEG", quality=75)
    return os.path.getsize(path)


def make_corpus(d, n, w, h, seed0):
    jobs = [(os.path.join(d, "img%05d.jpg" % i), w, h, seed0 + i) for i in range(n)]
    with ProcessPoolExecutor(THREADS) as ex:
        sizes = list(ex.map(_write, jobs, chunksize=8))
    return [j[0] for j in jobs], float(np.mean(sizes))


def warm(paths):
    for p in paths:
        with open(p, "rb") as f:
            f.read()


def rate_embed_file(ctx, paths):
    """(a): THREADS threads, each taking the next file and calling icl_embed_file (coalesced into batched forward passes)."""
    ctx.set_file_options(PREC, 2000, 256)
    nxt = [0]
    lock = threading.Lock()
    errs = []

    def run():
        while True:
            with lock:
                i = nxt[0]
                nxt[0] += 1
            if i >= len(paths):
                return
            try:
                ctx.embed_file(paths[i], HEAD)
            except _lib.ICLError as e:
                errs.append(str(e))

    t0 = time.perf_counter()
    ts = [threading.Thread(target=run) for _ in range(THREADS)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    assert not errs, errs[:3]
    return len(paths) / dt


def rate_embed_files(ctx, paths):
    t0 = time.perf_counter()
    E, status = ctx.embed_files(paths, HEAD, PREC, THREADS)
    dt = time.perf_counter() - t0
    assert (status == 0).all()
    st = ctx.last_ingest_stats()
    assert st["gpu_jpegs"] == len(paths), st
    if ENTROPY["mode"] != "host":  # the GPU decoder must have taken (and accepted) every file when it is on
        es = ctx.last_entropy_stats()
        assert es["gpu_entropy_jpegs"] in (0, len(paths)) and es["redone_on_host"] == 0, es
    return len(paths) / dt, st


def rate_embed_u8(ctx, imgs):
    ctx.embed_u8(imgs[:256], HEAD, PREC)
    t0 = time.perf_counter()
    ctx.embed_u8(imgs, HEAD, PREC)
    return imgs.shape[0] / (time.perf_counter() - t0)


ENTROPY = {"mode": "host", "reps": 3}


def images_per_slab(w, h, payload_bytes_per_file):
    """The slab builder's limits (jpeg_gpu.hip) for 4:2:0 files of one size: 256 rows, 128 MiB of payload, 768 MiB of u8 planes."""
    mx, my = -(-w // 16), -(-h // 16)
    planes = mx * 16 * my * 16 + 2 * (mx * 8 * my * 8)
    return int(min(256, (128 << 20) // max(1, payload_bytes_per_file), (768 << 20) // planes))


def entropy_ab(ctx, paths, w, h):
    """host and gpu entropy modes alternating on the same files: files/s per mode and repetition, host ms per file (stage A / A0),
    bytes uploaded and stream bytes per file.  The yardstick is the host mode of the same run."""
    out = {"host": [], "gpu": []}
    for mode, flag in (("host", _lib.ENTROPY_HOST), ("gpu", _lib.ENTROPY_GPU)):  # warm-up of both modes
        ctx.set_ingest_options(flag)
        ctx.embed_files(paths[:64], HEAD, PREC, THREADS)
    for _ in range(ENTROPY["reps"]):
        for mode, flag in (("host", _lib.ENTROPY_HOST), ("gpu", _lib.ENTROPY_GPU)):
            ctx.set_ingest_options(flag)
            r, st = rate_embed_files(ctx, paths)
            es = ctx.last_entropy_stats()
            out[mode].append({"files_per_s": round(r, 1), "host_ms_per_file": round(st["host_decode_s"] / len(paths) * 1e3, 3),
                              "upload_bytes_per_file": round(st["upload_bytes"] / len(paths)), "stream_bytes_per_file": round(es["stream_bytes"] / len(paths)),
                              "gpu_entropy_jpegs": es["gpu_entropy_jpegs"], "redone_on_host": es["redone_on_host"],
                              "images_per_slab": images_per_slab(w, h, round(st["upload_bytes"] / len(paths)))})
    ctx.set_ingest_options(_lib.ENTROPY_HOST)
    return out


def corpus_rates(ctx, name, paths, mean_bytes, trace_only, w=0, h=0):
    warm(paths)
    out = {"files": len(paths), "mean_jpeg_bytes": round(mean_bytes)}
    if ENTROPY["mode"] == "both":
        out["entropy_ab"] = entropy_ab(ctx, paths, w, h)
        return out
    ctx.embed_files(paths[:64], HEAD, PREC, THREADS)  # warm-up: code objects, pinned slabs, workspace
    if trace_only:
        r, st = rate_embed_files(ctx, paths)
        out["b_embed_files_per_s"] = round(r, 1)
        return out
    out["a_embed_file_16thr_per_s"] = round(rate_embed_file(ctx, paths), 1)
    r, st = rate_embed_files(ctx, paths)
    out["b_embed_files_16thr_per_s"] = round(r, 1)
    out["b_over_a"] = round(out["b_embed_files_16thr_per_s"] / out["a_embed_file_16thr_per_s"], 2)
    out["b_host_decode_ms_per_image"] = round(st["host_decode_s"] / len(paths) * 1e3, 3)
    out["b_upload_bytes_per_image"] = round(st["upload_bytes"] / len(paths))
    imgs, status = ctx.load_images_224(paths, THREADS)
    assert (status == 0).all()
    out["c_embed_u8_per_s"] = round(rate_embed_u8(ctx, imgs), 1)
    # the host route's decode cost per image on one thread, for comparison with stage A alone
    t0 = time.perf_counter()
    for p in paths[:32]:
        _lib.load_image_224(p)
    out["host_load_image_224_ms_per_image_1thr"] = round((time.perf_counter() - t0) / 32 * 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1080", type=int, default=4096)
    ap.add_argument("--n12mp", type=int, default=512)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--entropy", choices=["host", "gpu", "both"], default="host",
                    help="where the JPEG Huffman decoder runs; both: the two modes alternate on the same files (--reps times each)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    ctx = _lib.Context(0)
    ctx.load_synthetic(1)
    ENTROPY["mode"], ENTROPY["reps"] = args.entropy, args.reps
    if args.entropy == "gpu":
        ctx.set_ingest_options(_lib.ENTROPY_GPU)
    res = {"head": HEAD, "prec": "bf16", "threads": THREADS}
    tmp = tempfile.mkdtemp(prefix="icl_files_rate_")
    try:
        for name, n, w, h, seed in (("1080p_q75_baseline", args.n1080, 1920, 1080, 1), ("4000x3000_q75", args.n12mp, 4000, 3000, 100000)):
            if n <= 0:
                continue
            d = os.path.join(tmp, name)
            os.makedirs(d)
            paths, mean_bytes = make_corpus(d, n, w, h, seed)
            res[name] = corpus_rates(ctx, name, paths, mean_bytes, args.trace_only, w, h)
            shutil.rmtree(d, ignore_errors=True)
            print(name, json.dumps(res[name]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        ctx.close()
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
