#!/usr/bin/env python3
"""merge_ms (icl_last_stage_ms, as bench.py reports it) of the merge loop under two builds of the library:
  finish_ab_merge_ms.py PARENT.so BRANCH.so OUTDIR [PROCESSES_PER_BUILD [RUNS]]

Alternating child processes (ICL_SO_PATH; parent, branch, parent, ...).  Each embeds bench.py's 100 000 synthetic images once (bf16, batch
256, as the benchmark's default workload), then clusters the embeddings with min / max size 5 / 50: N = 100 000 in auto mode (bound rows,
ward_finish_lb_kernel) and the first 24 000 rows with ICL_DIST_BOUND (exact rows, ward_finish_batch_kernel) -- one warm-up call and RUNS timed
calls each, profiler and timers off.  A child writes OUTDIR/merge_ms_<build><k>.json in the form scratch/ab_rate_summary.py reads.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(out, runs):
    import torch

    from imageclust_amd import _lib

    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    ctx.load_synthetic(1)
    ctx.set_batch(256)
    n = 100000
    imgs = torch.empty(n * _lib.IMG_BYTES, dtype=torch.uint8, device=dev)
    ctx.synth_images_dev(20250217, 0, n, _lib.SYNTH_STRUCTURED, imgs.data_ptr())
    ctx.sync()
    E = torch.empty((n, _lib.HEAD_POOLED), dtype=torch.float32, device=dev)
    ctx.embed_u8_dev(imgs.data_ptr(), n, E.data_ptr(), _lib.HEAD_POOLED, _lib.PREC_BF16)
    del imgs
    res = {}
    for name, rows, mode in [("n100000_auto_bound_rows", n, 0), ("n24000_dist_bound_exact_rows", 24000, 2)]:
        ctx.set_ward_options(mode)
        ms, info = [], None
        for r in range(runs + 1):
            cid, rank, nc = ctx.cluster_dev(E.data_ptr(), rows, _lib.HEAD_POOLED, 5, 50)
            if r:
                ms.append(ctx.last_stage_ms()["merge_ms"])
            st = ctx.last_ward_stats()
            info = dict(clusters=int(nc), merges=st["merges"], steps=st["steps"], single_pick_steps=st["single_pick_steps"], rows=ctx.last_ward_mode()[0])
        res[name] = dict(merge_ms=dict(median=float(np.median(ms)), min=min(ms), max=max(ms), runs=ms), loop=info)
    ctx.close()
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]))
    libs = dict(parent=os.path.abspath(sys.argv[1]), branch=os.path.abspath(sys.argv[2]))
    outdir = sys.argv[3]
    procs = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    runs = int(sys.argv[5]) if len(sys.argv) > 5 else 5
    os.makedirs(outdir, exist_ok=True)
    for k in range(1, procs + 1):
        for tag in ("parent", "branch"):
            out = os.path.join(outdir, "merge_ms_%s%d.json" % (tag, k))
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, str(runs)], env=dict(os.environ, ICL_SO_PATH=libs[tag]),
                                timeout=240).returncode
            if rc != 0:
                print("child %s %d ended with status %d: nothing more is started" % (tag, k, rc))
                return 1
            j = json.load(open(out))
            print(tag, k, {name: [round(x, 2) for x in v["merge_ms"]["runs"]] for name, v in j.items()}, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
