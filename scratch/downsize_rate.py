"""Files/s of icl_downsize_images_mem against 16 host threads calling icl_downsize_image_mem, alternating in one process on one device.

Workload (seeded): 128 JPEGs of 4000x3000 at quality 95 written by Pillow into a temporary directory, each above 5 MiB (a smooth field
plus sigma 12 noise), held in memory; the reference's real limits (5 MiB, 2048).
  (gpu-host)  Context.downsize_images_mem with ICL_ENTROPY_HOST, 16 host threads
  (gpu-gpu)   ... with ICL_ENTROPY_GPU
  (host)      16 threads calling _lib.downsize_image_mem (ctypes releases the GIL)
The files are written by worker processes before the Context exists (no forked child ever holds the GPU open).  One warm-up of each,
then --rounds rounds of (gpu-host, gpu-gpu, host).  At 128 files a GPU-entropy round is a window of about 0.3 s: raise --files for a longer one.  Reports the median and min-max of files/s of each, the batched
call's stage split (icl_last_downsize_stats), and checks once that all three give the same bytes.  The batched call is the recommended
route only if its median is not below the host figure's maximum of the same run.

    python scratch/downsize_rate.py --out OUT.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402

THREADS = 16
MAX_BYTES, MAX_DIM = _lib.MAX_IMAGE_SIZE, _lib.MAX_IMAGE_DIM


def _write(job):
    path, w, h, seed = job
    from PIL import Image

    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (70 + 130 * c) + y / (110 + 50 * c) + c + seed % 97) for c in range(3)], -1)
    Image.fromarray(np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)).save(path, "JPEG", quality=95)
    return os.path.getsize(path)


def spread(dts, n):
    r = sorted(n / dt for dt in dts)
    return {"median": round(statistics.median(r), 2), "min": round(r[0], 2), "max": round(r[-1], 2), "all": [round(x, 2) for x in r]}


def run_batched(ctx, bufs, entropy):
    ctx.set_ingest_options(entropy)
    t0 = time.perf_counter()
    out, status = ctx.downsize_images_mem(bufs, MAX_BYTES, MAX_DIM, THREADS)
    dt = time.perf_counter() - t0
    assert (status == 0).all()
    return dt, out, ctx.last_downsize_stats()


def run_host(pool, bufs):
    t0 = time.perf_counter()
    out = list(pool.map(lambda b: _lib.downsize_image_mem(b, MAX_BYTES, MAX_DIM), bufs))
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="icl_downsize_rate_")
    ctx = None
    try:
        # the files first: the worker processes are forked, and must be gone, before anything in this process opens the GPU
        jobs = [(os.path.join(tmp, "img%04d.jpg" % i), 4000, 3000, 20261019 + i) for i in range(args.files)]
        with ProcessPoolExecutor(THREADS) as ex:
            sizes = list(ex.map(_write, jobs, chunksize=2))
        assert min(sizes) > MAX_BYTES, "a file is not above the limit: %d" % min(sizes)
        bufs = [open(j[0], "rb").read() for j in jobs]
        ctx = _lib.Context(0)
        pool = ThreadPoolExecutor(THREADS)
        modes = [("batched_entropy_host", _lib.ENTROPY_HOST), ("batched_entropy_gpu", _lib.ENTROPY_GPU)]
        ref = run_host(pool, bufs)[1]
        for name, e in modes:  # warm-up, and once: the same bytes
            assert run_batched(ctx, bufs, e)[1] == ref, name
        dts = {name: [] for name, _ in modes}
        stats = {name: [] for name, _ in modes}
        host = []
        for _ in range(args.rounds):
            for name, e in modes:
                dt, _, st = run_batched(ctx, bufs, e)
                dts[name].append(dt)
                stats[name].append(st)
            host.append(run_host(pool, bufs)[0])
        res = {"files": len(bufs), "image_size": "4000x3000 q95", "mean_jpeg_bytes": round(float(np.mean(sizes))), "mean_out_bytes": round(float(np.mean([len(r) for r in ref]))),
               "max_bytes": MAX_BYTES, "max_dim": MAX_DIM, "threads": THREADS, "rounds": args.rounds, "host_threads_files_per_s": spread(host, len(bufs)),
               "host_threads_window_s": round(statistics.median(host), 3)}
        for name, _ in modes:
            res[name + "_files_per_s"] = spread(dts[name], len(bufs))
            res[name + "_window_s"] = round(statistics.median(dts[name]), 3)
            last = stats[name][-1]
            res[name + "_stats"] = {k: last[k] for k in ("passthrough", "gpu_rebuilt", "host_decoded", "second_attempts")}
            res[name + "_stage_ms"] = {k: round(statistics.median(s["stage_ms"][k] for s in stats[name]), 1) for k in last["stage_ms"]}
            res[name + "_median_over_host_max"] = round(res[name + "_files_per_s"]["median"] / res["host_threads_files_per_s"]["max"], 3)
        res["recommended"] = "batched" if max(res[n + "_median_over_host_max"] for n, _ in modes) >= 1.0 else "host threads"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if ctx is not None:
            ctx.set_ingest_options(_lib.ENTROPY_HOST)
            ctx.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
