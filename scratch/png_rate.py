"""Files/s of the batched file ingest on PNG files, with the PNGs decoded by the host workers (PNG_HOST) and on the GPU (PNG_GPU), on one
device: 1024 1920x1080 and 256 4000x3000 RGB PNGs of photo-like content written by Pillow at its default level on local disk (the page
cache is warmed by reading every file once).  icl_embed_files, bf16, head 2048, 16 host threads; the two modes alternate in one process,
3 rounds each; files/s as min / median / max per mode.  The baseline is the host mode of the same run.  Per round also: host worker
milliseconds per file (icl_last_ingest_stats), bytes uploaded per file, and the wall time of icl_load_images_224_dev alone (the route
without the forward pass).  A JPEG-only corpus runs the same alternation, to show that the JPEG route does not move when PNG_GPU is set.
Prints and writes one JSON object; a line per round as it goes.

    python scratch/png_rate.py --out profiles/r23_png_rate.json
    python scratch/png_rate.py --trace-only --n1080 256 --n12mp 0     # PNG_GPU alone, e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402

HEAD, PREC, THREADS = 2048, _lib.PREC_BF16, 16


def _write(job):
    path, w, h, seed, fmt = job
    from PIL import Image

    rng = np.random.default_rng(seed)
    y = np.linspace(0, 6.0 + (seed % 7), h, dtype=np.float32)[:, None]
    x = np.linspace(0, 9.0 + (seed % 5), w, dtype=np.float32)[None, :]
    base = np.stack([128 + 90 * np.sin(x * (1 + 0.3 * c) + y * (1 + 0.2 * c) + seed) for c in range(3)], -1)
    img = np.clip(base + rng.integers(-12, 13, (h, w, 3), dtype=np.int16), 0, 255).astype(np.uint8)
    if fmt == "png":
        Image.fromarray(img).save(path, "PNG")  # Pillow's default level
    else:
        Image.fromarray(img).save(path, "JPEG", quality=75)
    return os.path.getsize(path)


def make_corpus(d, n, w, h, seed0, fmt):
    jobs = [(os.path.join(d, "img%05d.%s" % (i, fmt)), w, h, seed0 + i, fmt) for i in range(n)]
    with ProcessPoolExecutor(THREADS) as ex:
        sizes = list(ex.map(_write, jobs, chunksize=4))
    return [j[0] for j in jobs], float(np.mean(sizes))


def one_round(ctx, paths, mode, png):
    ctx.set_png_options(_lib.PNG_GPU if mode == "gpu" else _lib.PNG_HOST)
    t0 = time.perf_counter()
    E, status = ctx.embed_files(paths, HEAD, PREC, THREADS)
    dt = time.perf_counter() - t0
    assert (status == 0).all()
    st, ps = ctx.last_ingest_stats(), ctx.last_png_stats()
    if png:
        assert ps["redone_on_host"] == 0 and (ps["gpu_pngs"] if mode == "gpu" else ps["host_pngs"]) == len(paths), ps
    else:
        assert st["gpu_jpegs"] == len(paths) and not any(ps.values()), (st, ps)
    d = ctx.malloc(len(paths) * _lib.IMG_BYTES)
    try:
        t0 = time.perf_counter()
        ctx.load_images_224_dev(paths, d, THREADS)
        dl = time.perf_counter() - t0
    finally:
        ctx.free(d)
    return {"files_per_s": round(len(paths) / dt, 1), "decode_only_files_per_s": round(len(paths) / dl, 1),
            "host_ms_per_file": round(st["host_decode_s"] / len(paths) * 1e3, 3), "upload_bytes_per_file": round(st["upload_bytes"] / len(paths))}


def alternate(ctx, paths, reps, png, name):
    for p in paths:
        with open(p, "rb") as f:
            f.read()
    rounds = {"host": [], "gpu": []}
    for mode in ("host", "gpu"):  # warm-up of both modes: code objects, pinned slabs, workspace
        ctx.set_png_options(_lib.PNG_GPU if mode == "gpu" else _lib.PNG_HOST)
        ctx.embed_files(paths[:32], HEAD, PREC, THREADS)
    for r in range(reps):
        for mode in ("host", "gpu"):
            rounds[mode].append(one_round(ctx, paths, mode, png))
            print(name, mode, r, json.dumps(rounds[mode][-1]), flush=True)
    ctx.set_png_options(_lib.PNG_HOST)
    out = {"rounds": rounds}
    for mode in ("host", "gpu"):
        v = sorted(x["files_per_s"] for x in rounds[mode])
        out[mode + "_files_per_s_min_median_max"] = [v[0], v[len(v) // 2], v[-1]]
    out["gpu_min_over_host_max"] = round(out["gpu_files_per_s_min_median_max"][0] / out["host_files_per_s_min_median_max"][2], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n1080", type=int, default=1024)
    ap.add_argument("--n12mp", type=int, default=256)
    ap.add_argument("--njpeg", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.Context(0)
    ctx.load_synthetic(1)
    res = {"head": HEAD, "prec": "bf16", "threads": THREADS, "reps": args.reps}
    tmp = tempfile.mkdtemp(prefix="icl_png_rate_")
    try:
        for name, n, w, h, seed, fmt in (("png_1080p", args.n1080, 1920, 1080, 1, "png"), ("png_4000x3000", args.n12mp, 4000, 3000, 100000, "png"),
                                         ("jpeg_only_1080p_q75", 0 if args.trace_only else args.njpeg, 1920, 1080, 200000, "jpg")):
            if n <= 0:
                continue
            d = os.path.join(tmp, name)
            os.makedirs(d)
            paths, mean_bytes = make_corpus(d, n, w, h, seed, fmt)
            if args.trace_only:
                ctx.set_png_options(_lib.PNG_GPU)
                ctx.embed_files(paths[:32], HEAD, PREC, THREADS)
                res[name] = one_round(ctx, paths, "gpu", True)
            else:
                res[name] = alternate(ctx, paths, args.reps, fmt == "png", name)
            res[name].update({"files": n, "mean_file_bytes": round(mean_bytes)})
            shutil.rmtree(d, ignore_errors=True)
            print(name, json.dumps(res[name]), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(res, f, indent=1)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
