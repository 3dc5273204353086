"""Files/s of three ways to embed images a caller holds as encoded bytes, on one device: 4096 1920x1080 q75 baseline JPEGs (the corpus
of files_rate.py), bf16, head 2048, 16 host threads, one process, in ICL_ENTROPY_HOST and ICL_ENTROPY_GPU:
  (a) icl_embed_files on the files as they lie on disk (page cache warm)
  (b) icl_embed_images_mem on the same bytes held in memory
  (c) the service's pattern without (b): write the bytes to a fresh temporary directory, then icl_embed_files (workflow.go:120-127)
The three alternate, three repetitions each per mode.  The comparison that matters is (b) against (c); (b) against (a) shows the read
cost on a warm page cache.  Condition: (b)'s median is not below (a)'s minimum in the same run.  Prints and writes one JSON object.

    python scratch/mem_rate.py --out profiles/r17_mem_rate.json [--n 4096]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402
from scratch.files_rate import make_corpus, warm  # noqa: E402

HEAD, PREC, THREADS, REPS = 2048, _lib.PREC_BF16, 16, 3


def timed(call, n):
    t0 = time.perf_counter()
    E, status = call()
    dt = time.perf_counter() - t0
    assert (status == 0).all() and E.shape == (n, HEAD)
    return n / dt, E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--n", type=int, default=4096)
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="icl_mem_rate_")
    try:
        paths, mean_bytes = make_corpus(d, a.n, 1920, 1080, 7000)
        warm(paths)
        bufs = [open(p, "rb").read() for p in paths]
        ctx = _lib.Context(0)
        ctx.load_synthetic(1)
        res = {"n": a.n, "mean_file_bytes": mean_bytes, "head": HEAD, "prec": "bf16", "threads": THREADS, "reps": REPS, "modes": {}}
        for mode, name in ((_lib.ENTROPY_HOST, "host"), (_lib.ENTROPY_GPU, "gpu")):
            ctx.set_ingest_options(mode)
            ref = ctx.embed_files(paths[:256], HEAD, PREC, THREADS)[0]  # warm-up: workspaces, first-launch costs
            rates = {"a_files_on_disk": [], "b_bytes_in_memory": [], "c_write_then_files": []}
            for _ in range(REPS):
                r, E = timed(lambda: ctx.embed_files(paths, HEAD, PREC, THREADS), a.n)
                rates["a_files_on_disk"].append(r)
                assert np.array_equal(E[:256], ref)
                r, E = timed(lambda: ctx.embed_images_mem(bufs, HEAD, PREC, THREADS), a.n)
                rates["b_bytes_in_memory"].append(r)
                assert np.array_equal(E[:256], ref)
                es = ctx.last_entropy_stats()
                assert es["redone_on_host"] == 0 and es["gpu_entropy_jpegs"] == (a.n if name == "gpu" else 0), es
                tmp = tempfile.mkdtemp(prefix="icl_upload_", dir=d)

                def write_then_embed():
                    out = []
                    for i, b in enumerate(bufs):
                        p = os.path.join(tmp, "img_%d.jpg" % i)
                        with open(p, "wb") as f:
                            f.write(b)
                        out.append(p)
                    return ctx.embed_files(out, HEAD, PREC, THREADS)

                r, E = timed(write_then_embed, a.n)
                rates["c_write_then_files"].append(r)
                shutil.rmtree(tmp)
            m = {k: {"files_per_s": v, "median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in rates.items()}
            m["b_median_not_below_a_min"] = m["b_bytes_in_memory"]["median"] >= m["a_files_on_disk"]["min"]
            m["b_over_c_median"] = m["b_bytes_in_memory"]["median"] / m["c_write_then_files"]["median"]
            res["modes"][name] = m
        ctx.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
