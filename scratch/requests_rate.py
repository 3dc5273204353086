"""Requests/s of icl_cluster_requests against the composition it replaces, alternating in one process on one device.

Workload (seeded): 256 requests, n uniform in [8, 64] images each, 640x480 q75 baseline JPEGs written by Pillow on local disk (smooth
photo-like content plus noise; the page cache is warmed by reading every file once), label sets of L in [0, 200] columns with one or
two labels per image, min 3 / max 6, bf16, head 1000, 16 host threads.
  (new)  Context.cluster_requests: files -> dense rows -> combined rows assembled on the GPU -> Ward, one call
  (comp) Context.embed_files -> [dense | one-hot] rows built with numpy on the host -> Context.cluster_many
One warm-up of each, then --rounds rounds of (new, comp).  Reports the median and min-max of requests/s of both, the three stage times
of the new call (icl_last_requests_ms, medians) and the composition's own split, and checks once that both give the same ids.
--entropy both repeats the whole measurement with ICL_ENTROPY_GPU.

    python scratch/requests_rate.py --out OUT.json
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402

HEAD, PREC, THREADS = _lib.HEAD_DENSE0, _lib.PREC_BF16, 16


def _write(job):
    path, w, h, seed = job
    from PIL import Image

    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (7 + 13 * c) + y / (11 + 5 * c) + c + seed % 97) for c in range(3)], -1)  # picture() of the tests
    Image.fromarray(np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)).save(path, "JPEG", quality=75)
    return os.path.getsize(path)


def make_requests(d, nreq, seed):
    rng = np.random.default_rng(seed)
    ns = rng.integers(8, 65, nreq)
    jobs = [(os.path.join(d, "img%05d.jpg" % i), 640, 480, seed * 100000 + i) for i in range(int(ns.sum()))]
    with ProcessPoolExecutor(THREADS) as ex:
        sizes = list(ex.map(_write, jobs, chunksize=16))
    reqs, at = [], 0
    for n in ns:
        nl = int(rng.integers(0, 201))
        labels = [sorted(int(j) for j in rng.integers(0, nl, int(rng.integers(1, 3)))) if nl else [] for _ in range(int(n))]
        reqs.append(([j[0] for j in jobs[at:at + int(n)]], labels, nl, 3, 6))
        at += int(n)
    return reqs, float(np.mean(sizes))


def run_new(ctx, reqs):
    t0 = time.perf_counter()
    res = ctx.cluster_requests(reqs, HEAD, PREC, THREADS)
    dt = time.perf_counter() - t0
    assert (ctx.last_file_status == 0).all()
    return dt, res, ctx.last_requests_ms()


def run_comp(ctx, reqs, pk):
    t0 = time.perf_counter()
    dense, status = ctx.embed_files(pk["paths"], HEAD, PREC, THREADS)
    t1 = time.perf_counter()
    probs = []
    for r, (ps, labels, nl, mn, mx) in enumerate(reqs):
        a = int(pk["img_off"][r])
        E = np.zeros((len(ps), HEAD + nl), np.float32)
        E[:, :HEAD] = dense[a:a + len(ps)]
        for i, li in enumerate(labels):
            for j in li:
                E[i, HEAD + j] = 1.0
        probs.append((E, mn, mx))
    t2 = time.perf_counter()
    res = ctx.cluster_many(probs)
    t3 = time.perf_counter()
    assert (status == 0).all()
    return t3 - t0, res, {"embed_files_ms": (t1 - t0) * 1e3, "host_combine_ms": (t2 - t1) * 1e3, "cluster_many_ms": (t3 - t2) * 1e3}


def spread(dts, nreq):
    r = sorted(nreq / dt for dt in dts)
    return {"median": round(statistics.median(r), 1), "min": round(r[0], 1), "max": round(r[-1], 1), "all": [round(x, 1) for x in r]}


def med(dicts):
    return {k: round(statistics.median(d[k] for d in dicts), 3) for k in dicts[0]}


def measure(ctx, reqs, rounds):
    pk = _lib.pack_requests(reqs, HEAD)
    _, a, _ = run_new(ctx, reqs)
    _, b, _ = run_comp(ctx, reqs, pk)
    for r, (x, y) in enumerate(zip(a, b)):  # (once, outside the timed rounds)
        assert all(np.array_equal(p, q) for p, q in zip(x, y)), "request %d differs from the composition" % r
    new, comp, new_ms, comp_ms = [], [], [], []
    for _ in range(rounds):
        dt, _, ms = run_new(ctx, reqs)
        new.append(dt)
        new_ms.append(ms)
        dt, _, ms = run_comp(ctx, reqs, pk)
        comp.append(dt)
        comp_ms.append(ms)
    out = {"cluster_requests_per_s": spread(new, len(reqs)), "composition_requests_per_s": spread(comp, len(reqs)),
           "cluster_requests_stage_ms": med(new_ms), "composition_stage_ms": med(comp_ms)}
    out["new_median_over_composition_min"] = round(out["cluster_requests_per_s"]["median"] / out["composition_requests_per_s"]["min"], 3)
    out["new_median_over_composition_median"] = round(out["cluster_requests_per_s"]["median"] / out["composition_requests_per_s"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--entropy", choices=["host", "both"], default="host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.Context(0)
    ctx.load_synthetic(1)
    ctx.set_ingest_options(_lib.ENTROPY_HOST)
    tmp = tempfile.mkdtemp(prefix="icl_requests_rate_")
    try:
        reqs, mean_bytes = make_requests(tmp, args.requests, 20261018)
        images = sum(len(r[0]) for r in reqs)
        for r in reqs:
            for p in r[0]:
                with open(p, "rb") as f:
                    f.read()
        res = {"requests": len(reqs), "images": images, "mean_jpeg_bytes": round(mean_bytes), "image_size": "640x480 q75", "head": HEAD, "prec": "bf16",
               "threads": THREADS, "rounds": args.rounds, "min_size": 3, "max_size": 6}
        res["entropy_host"] = measure(ctx, reqs, args.rounds)
        print("entropy_host", json.dumps(res["entropy_host"]), flush=True)
        if args.entropy == "both":
            ctx.set_ingest_options(_lib.ENTROPY_GPU)
            res["entropy_gpu"] = measure(ctx, reqs, args.rounds)
            ctx.set_ingest_options(_lib.ENTROPY_HOST)
            print("entropy_gpu", json.dumps(res["entropy_gpu"]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        ctx.close()
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
