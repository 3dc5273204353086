"""Problems/s of icl_cluster_many against icl_cluster on one device, for seeded problems of the reference's request shape
(workflow.Run -> PerformClusteringWithConstraints on one upload): n uniform in [8, 256], d = 1000 + L with L uniform in [0, 200]
appended 0/1 label columns (one-hot), min 3 / max 6, exact mode.
  (a)  icl_cluster_many on all problems, E from host memory (upload included); (a') icl_cluster_many_dev, E already on the device
  (b)  a loop of icl_cluster on one context
  (c)  16 host threads calling icl_cluster on one context
  (d)  wall time of a one-problem icl_cluster_many against one icl_cluster on the same problem
  (e)  the same for single problems of n = 256 ... 1024 rows (the cap of the one-workgroup route)
Every call returns after the stream is idle (the library synchronises before it hands back results).  Warm-up calls first; spreads
are over repeats.  Prints and writes one JSON object.

    python scratch/cluster_many_rate.py --out OUT.json
    python scratch/cluster_many_rate.py --trace-only        # (a) once, e.g. under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402

THREADS = 16


def problems(count, seed, n_lo=8, n_hi=256):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(n_lo, n_hi + 1))
        L = int(rng.integers(0, 201))
        E = np.zeros((n, 1000 + L), np.float32)
        E[:, :1000] = np.abs(rng.standard_normal(1000, dtype=np.float32)) + 0.3 * rng.standard_normal((n, 1000), dtype=np.float32)
        if L:
            E[np.arange(n), 1000 + rng.integers(0, L, n)] = 1.0
        out.append((E, 3, 6))
    return out


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()), reps=int(xs.size))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def loop_cluster(ctx, probs):
    for E, mn, mx in probs:
        ctx.cluster(E, mn, mx)


def threads_cluster(ctx, probs):
    nxt = [0]
    lock = threading.Lock()

    def work():
        while True:
            with lock:
                i = nxt[0]
                nxt[0] += 1
            if i >= len(probs):
                return
            E, mn, mx = probs[i]
            ctx.cluster(E, mn, mx)

    ts = [threading.Thread(target=work) for _ in range(THREADS)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--baseline-problems", type=int, default=1024, help="problems timed for (b) and (c): the first ones of the same set")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    probs = problems(a.problems, 20261016)
    ctx = _lib.Context(0)
    if a.trace_only:
        ctx.cluster_many(probs[:64])
        ctx.cluster_many(probs)
        ctx.close()
        return
    res = ctx.cluster_many(probs)  # warm-up (workspace, code objects)
    assert all(r[3] == 0 for r in res)
    ta = timed(lambda: ctx.cluster_many(probs), a.reps)
    pk = _lib.pack_many(probs)
    dE = ctx.malloc(pk["E"].nbytes)
    ctx.h2d(dE, pk["E"])
    dev = lambda: ctx.cluster_many_dev(dE, pk["E"].size, pk["e_off"], pk["n"], pk["d"], pk["min_size"], pk["max_size"])
    dev()
    tad = timed(dev, a.reps)
    ctx.free(dE)
    base = probs[: a.baseline_problems]
    loop_cluster(ctx, base[:32])  # warm-up
    tb = timed(lambda: loop_cluster(ctx, base), max(2, a.reps // 2))
    tc = timed(lambda: threads_cluster(ctx, base), max(2, a.reps // 2))
    # (d): one problem of the set's median size, many single calls
    one = sorted(probs[:256], key=lambda p: p[0].shape[0])[128]
    for _ in range(5):
        ctx.cluster_many([one])
        ctx.cluster(*one)
    d_many = timed(lambda: ctx.cluster_many([one]), 50)
    d_one = timed(lambda: ctx.cluster(*one), 50)
    # (e): single problems up to the cap
    e = {}
    rng = np.random.default_rng(5)
    for n in (256, 512, 768, 1024):
        E = problems(1, 100 + n, n, n)[0][0]
        ctx.cluster_many([(E, 3, 6)])
        ctx.cluster(E, 3, 6)
        e[str(n)] = dict(d=int(E.shape[1]), cluster_many_ms=stats([1e3 * t for t in timed(lambda: ctx.cluster_many([(E, 3, 6)]), 5)]),
                         cluster_ms=stats([1e3 * t for t in timed(lambda: ctx.cluster(E, 3, 6), 5)]))
    ctx.close()
    nb = len(base)
    out = dict(
        device="MI355X (1 GCD)", problems=a.problems, baseline_problems=nb, n_range=[8, 256], d="1000 + L, L in [0, 200] one-hot label columns",
        min_size=3, max_size=6, mean_n=float(np.mean([p[0].shape[0] for p in probs])), mean_d=float(np.mean([p[0].shape[1] for p in probs])),
        a_cluster_many_problems_per_s=stats([a.problems / t for t in ta]),
        a_dev_cluster_many_problems_per_s=stats([a.problems / t for t in tad]),
        b_cluster_loop_problems_per_s=stats([nb / t for t in tb]),
        c_cluster_16_threads_problems_per_s=stats([nb / t for t in tc]),
        d_one_problem=dict(n=int(one[0].shape[0]), d=int(one[0].shape[1]), cluster_many_ms=stats([1e3 * t for t in d_many]),
                           cluster_ms=stats([1e3 * t for t in d_one])),
        e_single_problem_by_n=e,
    )
    out["speedup_a_over_b"] = out["a_cluster_many_problems_per_s"]["median"] / out["b_cluster_loop_problems_per_s"]["median"]
    out["speedup_a_over_c"] = out["a_cluster_many_problems_per_s"]["median"] / out["c_cluster_16_threads_problems_per_s"]["median"]
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
