"""Where the GPU PNG route spends its time on one image: wall-clock milliseconds, each behind a stream synchronisation, of the test hook
icl_png_raw_files at stage 0 (parse + upload + inflate + Adler-32) and stage 1 (the same + unfilter), and of icl_load_images_224_dev on
the one file (the same + gather / resize) in PNG_GPU and in PNG_HOST mode, for 1920x1080 RGB PNGs of scratch/png_rate.py's content.
One image occupies one workgroup of the inflate and unfilter kernels, so these are latencies of the serial stages, not rates.

    python scratch/png_stage_time.py --out profiles/r23_png_stage_ms.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402
from scratch.png_rate import _write  # noqa: E402


def ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = _lib.Context(0)
    with tempfile.TemporaryDirectory(prefix="icl_png_stage_") as d:
        paths = [os.path.join(d, "img%d.png" % i) for i in range(args.files)]
        for i, p in enumerate(paths):
            _write((p, 1920, 1080, 1 + i, "png"))
        rows = {"stage0_inflate_adler_ms": [], "stage1_plus_unfilter_ms": [], "load_224_png_gpu_ms": [], "load_224_png_host_ms": []}
        for rep in range(2):  # (the first repetition warms code objects and buffers up and is dropped)
            for p in paths:
                t = {}
                for stage, key in ((0, "stage0_inflate_adler_ms"), (1, "stage1_plus_unfilter_ms")):
                    t[key] = ms(lambda: ctx.png_raw_files([p], stage))
                ctx.set_png_options(_lib.PNG_GPU)
                t["load_224_png_gpu_ms"] = ms(lambda: ctx.load_images_224([p]))
                assert ctx.last_png_stats()["gpu_pngs"] == 1
                ctx.set_png_options(_lib.PNG_HOST)
                t["load_224_png_host_ms"] = ms(lambda: ctx.load_images_224([p]))
                if rep:
                    for k, v in t.items():
                        rows[k].append(round(v, 2))
    ctx.close()
    res = {"size": "1920x1080 RGB", "files": args.files, "per_file_ms": rows, "median_ms": {k: round(statistics.median(v), 2) for k, v in rows.items()}}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
