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

--n-lo / --n-hi change the range of n and --mid the context's mid-size route (icl_set_many_options); the defaults are the run above.
--mid-table measures the mid-size route (problems of 257 to 2048 rows, one workgroup each) against the large-N engine instead: per
band of n and batch size, ICL_MANY_MID_OFF and ICL_MANY_MID_ON alternate in one process on the same problems (one untimed call of
each first), E from host memory and E on the device; the rates, their spreads and what ICL_MANY_MID_AUTO chose go to the JSON.

    python scratch/cluster_many_rate.py --out OUT.json
    python scratch/cluster_many_rate.py --trace-only        # (a) once, e.g. under rocprofv3 --kernel-trace --stats
    python scratch/cluster_many_rate.py --mid-table --out OUT.json
    python scratch/cluster_many_rate.py --trace-only --mid on --problems 256 --n-lo 513 --n-hi 1024
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


MID_MODES = {"auto": _lib.MANY_MID_AUTO, "off": _lib.MANY_MID_OFF, "on": _lib.MANY_MID_ON}
BANDS = [(257, 512, (1, 2, 4, 8, 16, 64, 256, 1024)), (513, 1024, (1, 2, 4, 8, 16, 64, 256)), (1025, 2048, (1, 2, 4, 8, 16, 64, 256))]


def mid_table(ctx, reps, bands, out_path):
    """OFF against ON per (band, batch size): alternating in one process on the same problems, the context warmed by one untimed call of
    each mode.  A rate's spread is (max - min) / 2 over its repetitions."""
    cells = []

    def rate(xs, count):
        r = np.asarray([count / t for t in xs])
        return dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), spread=float((r.max() - r.min()) / 2), reps=int(r.size))

    for lo, hi, sizes in bands:
        probs_all = problems(max(sizes), 20261016 + lo, lo, hi)
        for bs in sizes:
            probs = probs_all[:bs]
            pk = _lib.pack_many(probs)
            dE = ctx.malloc(pk["E"].nbytes)
            ctx.h2d(dE, pk["E"])
            host = lambda: ctx.cluster_many(probs)
            dev = lambda: ctx.cluster_many_dev(dE, pk["E"].size, pk["e_off"], pk["n"], pk["d"], pk["min_size"], pk["max_size"])
            t = {("off", "host"): [], ("on", "host"): [], ("off", "dev"): [], ("on", "dev"): []}
            for mode in ("off", "on"):  # untimed: workspace, code objects
                ctx.set_many_options(MID_MODES[mode])
                host()
                dev()
            for _ in range(reps):
                for mode in ("off", "on"):
                    ctx.set_many_options(MID_MODES[mode])
                    t[(mode, "host")] += timed(host, 1)
                    t[(mode, "dev")] += timed(dev, 1)
            ctx.set_many_options(MID_MODES["auto"])
            host()
            auto = ctx.last_many_stats()
            ctx.free(dE)
            cell = dict(band=[lo, hi], batch=bs, mean_n=float(np.mean([p[0].shape[0] for p in probs])),
                        auto_took_mid=auto["mid"] > 0, auto_stats=auto)
            for (mode, where), xs in t.items():
                cell["%s_%s_problems_per_s" % (mode, where)] = rate(xs, bs)
            for where in ("host", "dev"):
                a, b = cell["off_%s_problems_per_s" % where], cell["on_%s_problems_per_s" % where]
                margin = a["spread"] + b["spread"]
                cell["%s_winner" % where] = "on" if b["median"] - a["median"] > margin else "off" if a["median"] - b["median"] > margin else "within spreads"
            cells.append(cell)
            print(json.dumps(cell), flush=True)
            if out_path:  # (kept up to date: a long run that is cut short leaves its finished cells)
                with open(out_path, "w") as f:
                    f.write(json.dumps(dict(device="MI355X (1 GCD)", d="1000 + L, L in [0, 200] one-hot label columns", min_size=3, max_size=6,
                                            reps=reps, cells=cells), indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--baseline-problems", type=int, default=1024, help="problems timed for (b) and (c): the first ones of the same set")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--n-lo", type=int, default=8)
    ap.add_argument("--n-hi", type=int, default=256)
    ap.add_argument("--mid", choices=sorted(MID_MODES), default="auto", help="the mid-size route of the context (icl_set_many_options)")
    ap.add_argument("--mid-table", action="store_true")
    ap.add_argument("--bands", default="0,1,2", help="--mid-table: which of the bands [257, 512], [513, 1024], [1025, 2048]")
    ap.add_argument("--batches", help="--mid-table: these batch sizes (comma-separated) instead of the standard ones")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    if a.mid_table:
        bands = [BANDS[int(b)] for b in a.bands.split(",")]
        if a.batches:
            bands = [(lo, hi, tuple(int(x) for x in a.batches.split(","))) for lo, hi, _ in bands]
        mid_table(ctx, max(a.reps, 3), bands, a.out)
        ctx.close()
        return
    probs = problems(a.problems, 20261016, a.n_lo, a.n_hi)
    ctx.set_many_options(MID_MODES[a.mid])
    if a.trace_only:
        ctx.cluster_many(probs[:64])
        ctx.cluster_many(probs)
        print(json.dumps(ctx.last_many_stats()))
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
        device="MI355X (1 GCD)", problems=a.problems, baseline_problems=nb, n_range=[a.n_lo, a.n_hi], mid=a.mid, d="1000 + L, L in [0, 200] one-hot label columns",
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
