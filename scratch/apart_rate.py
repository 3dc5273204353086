"""Problems/s of icl_cluster_many_apart on one device, on the request-shape problems of scratch/seeded_rate.py (n uniform in [8, 256],
d = 1000 + L, min 3 / max 6), every call with E in host memory (upload included), modes alternating round by round in one process
after one untimed call of each:
  (a) all-ones seeds, no constraint: icl_cluster_many_apart against icl_cluster_many_seeded on the same problems (equal results:
      asserted) -- what the bit rows cost when they are empty;
  (b) "absorb the leftovers of a finished request": the request is clustered once (untimed; the state is the final clusters, dropped
      ones included, with their sizes and C_out centroids); timed is the constrained call on that state with every cluster of at least
      min_size items in class 1 and k_target = their number.  No comparator: no other route does it.
Prints and writes one JSON object.

    python scratch/apart_rate.py --out profiles/r34_apart_rate.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))

from cluster_many_rate import problems  # noqa: E402
from imageclust_amd import _lib  # noqa: E402
from seeded_rate import alternate, finished_state  # noqa: E402


def rate(ts, count):
    r = np.asarray([count / t for t in ts])
    return dict(median=float(np.median(r)), min=float(r.min()), max=float(r.max()), rounds=int(r.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=4096)
    ap.add_argument("--absorb-problems", type=int, default=1024, help="requests of (b): the first ones of the set with more than 16 images")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    probs = problems(a.problems, 20261016)
    ones = [(E, np.ones(len(E), np.int32), mn, mx) for E, mn, mx in probs]
    bare = [j + (0, None, None) for j in ones]
    ref, got = ctx.cluster_many_seeded(ones, want_merges=True, want_centroids=True), ctx.cluster_many_apart(bare, want_merges=True, want_centroids=True)
    assert all(x[3] == 0 and all(np.array_equal(u, v) for u, v in zip(x, y)) for x, y in zip(ref, got))
    ta = alternate({"seeded": lambda: ctx.cluster_many_seeded(ones), "apart_no_constraint": lambda: ctx.cluster_many_apart(bare)}, a.rounds)
    out = dict(device="MI355X (1 GCD)", problems=a.problems, n_range=[8, 256], d="1000 + L, L in [0, 200] one-hot label columns", min_size=3,
               max_size=6, rounds=a.rounds, mean_n=float(np.mean([len(p[0]) for p in probs])),
               all_ones_problems_per_s={k: rate(v, a.problems) for k, v in ta.items()})
    r = out["all_ones_problems_per_s"]
    out["apart_over_seeded"] = r["apart_no_constraint"]["median"] / r["seeded"]["median"]
    out["apart_median_below_seeded_min"] = bool(r["apart_no_constraint"]["median"] < r["seeded"]["min"])
    # (b)
    first = [(p, q) for p, q in zip(probs, ref) if len(p[0]) > 16][: a.absorb_problems]
    del ones, bare, got
    jobs, left = [], 0
    for (E, mn, mx), res in first:
        C, ss = finished_state(E, res)
        anchors = (ss >= mn).astype(np.int32)
        left += int(ss[ss < mn].sum())
        jobs.append((C, ss, mn, mx, max(1, int(anchors.sum())), anchors, None))
    res = ctx.cluster_many_apart(jobs, want_merges=True)
    assert all(x[3] == 0 for x in res)
    placed = sum(int(j[1][x[0] >= 0].sum()) for j, x in zip(jobs, res)) - sum(int(j[1][j[1] >= j[2]].sum()) for j in jobs)
    tb = alternate({"absorb_leftovers": lambda: ctx.cluster_many_apart(jobs, want_centroids=True)}, a.rounds)
    out["absorb_leftovers"] = dict(requests=len(jobs), mean_seeds=float(np.mean([len(j[1]) for j in jobs])), mean_merges=float(np.mean([len(x[4]) for x in res])),
                                   leftover_images=left, images_placed=placed, requests_per_s=rate(tb["absorb_leftovers"], len(jobs)))
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
