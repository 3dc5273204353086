"""Problems/s of icl_cluster_many_seeded on one device, on the request-shape problems of scratch/cluster_many_rate.py (n uniform in
[8, 256], d = 1000 + L, min 3 / max 6), every call with E in host memory (upload included), modes alternating round by round in
one process after one untimed call of each:
  (a) all-ones seeds: icl_cluster_many against icl_cluster_many_seeded without and with C_out, on the same problems;
  (b) "add 8 images to a finished request": the request's first n - 8 images are clustered once (untimed; the state is the final
      clusters with their sizes and C_out centroids); timed are the seeded call on [state clusters + 8 singletons] against
      icl_cluster_many on all n images from scratch.  (The two end with different partitions: the seeded run keeps what was formed.)
Prints and writes one JSON object.

    python scratch/seeded_rate.py --out profiles/r24_seeded_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))

from cluster_many_rate import problems  # noqa: E402
from imageclust_amd import _lib  # noqa: E402

ADD = 8


def rate(ts, count):
    r = np.asarray([count / t for t in ts])
    return dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), rounds=int(r.size))


def finished_state(E, res):
    """(centroids, sizes) of every final cluster -- dropped ones included -- of a seeded all-ones run: res = (.., merge log, C_out)"""
    m, mg, co = len(E), res[4], res[5]
    first, size = {i: i for i in range(m)}, {i: 1 for i in range(m)}
    for t, (a, b) in enumerate(mg):
        first[m + t], size[m + t] = first.pop(int(a)), size.pop(int(a)) + size.pop(int(b))
        first.pop(int(b))
    ids = sorted(first)
    return co[[first[c] for c in ids]], np.array([size[c] for c in ids], np.int32)


def alternate(modes, rounds):
    """modes: name -> callable; one untimed call of each, then `rounds` rounds of one timed call each, in turn"""
    for fn in modes.values():
        fn()
    ts = {k: [] for k in modes}
    for _ in range(rounds):
        for k, fn in modes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--add-problems", type=int, default=1024, help="requests of (b): the first ones of the set with more than 16 images")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    probs = problems(a.problems, 20261016)
    ones = [(E, np.ones(len(E), np.int32), mn, mx) for E, mn, mx in probs]
    ref, got = ctx.cluster_many(probs, want_merges=True), ctx.cluster_many_seeded(ones, want_merges=True)
    assert all(x[3] == 0 and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(ref, got))
    ta = alternate({"cluster_many": lambda: ctx.cluster_many(probs), "seeded": lambda: ctx.cluster_many_seeded(ones),
                    "seeded_with_C_out": lambda: ctx.cluster_many_seeded(ones, want_centroids=True)}, a.rounds)
    out = dict(device="MI355X (1 GCD)", problems=a.problems, n_range=[8, 256], d="1000 + L, L in [0, 200] one-hot label columns", min_size=3,
               max_size=6, rounds=a.rounds, mean_n=float(np.mean([len(p[0]) for p in probs])),
               all_ones_problems_per_s={k: rate(v, a.problems) for k, v in ta.items()})
    out["all_ones_seeded_over_cluster_many"] = out["all_ones_problems_per_s"]["seeded"]["median"] / out["all_ones_problems_per_s"]["cluster_many"]["median"]
    # (b)
    full = [p for p in probs if len(p[0]) > 2 * ADD][: a.add_problems]
    del probs, ones, ref, got
    first = ctx.cluster_many_seeded([(E[:-ADD], np.ones(len(E) - ADD, np.int32), mn, mx) for E, mn, mx in full], want_merges=True, want_centroids=True)
    more = []
    for (E, mn, mx), r in zip(full, first):
        assert r[3] == 0
        C, ss = finished_state(E[:-ADD], r)
        more.append((np.concatenate([C, E[-ADD:]]), np.concatenate([ss, np.ones(ADD, np.int32)]), mn, mx))
    tb = alternate({"recluster_from_scratch": lambda: ctx.cluster_many(full), "seeded_add_8": lambda: ctx.cluster_many_seeded(more, want_centroids=True)},
                   a.rounds)
    out["add_8_images"] = dict(requests=len(full), mean_n=float(np.mean([len(p[0]) for p in full])), mean_seeds=float(np.mean([len(p[0]) for p in more])),
                               requests_per_s={k: rate(v, len(full)) for k, v in tb.items()})
    out["add_8_images"]["seeded_over_scratch"] = (out["add_8_images"]["requests_per_s"]["seeded_add_8"]["median"]
                                                   / out["add_8_images"]["requests_per_s"]["recluster_from_scratch"]["median"])
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
