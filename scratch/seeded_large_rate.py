"""Adding images to a large finished clustering: icl_cluster_seeded_dev on [final clusters + new singletons] against icl_cluster_dev on all
rows again, on one device.

20 000 mixture-of-Gaussians rows of d = 2048 are clustered at min 5 / max 50 (untimed); the state is the 2 200 final clusters, dropped ones
included, with their sizes and the centroids the engine holds (C_out of an all-ones seeded run, whose log must equal icl_cluster_dev's).
512 more rows join as singleton seeds: 2 712 seeds, 456 merges.  Timed, wall clock around the call (results on the host when it returns),
inputs resident on the device: the seeded call on the 2 712 seeds against icl_cluster_dev on all 20 512 rows.  Each mode has a context of its
own (so each keeps its workspace, as a long-running service would); one untimed call of each, then the modes alternate round by round.
(The two end with different partitions: the seeded run keeps what was formed.)  Prints and writes one JSON object.

    python scratch/seeded_large_rate.py --out profiles/r25_seeded_large_rate.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402


def make_rows(n, d, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cen = torch.randn((n // 20, d), generator=g, device="cuda")
    lab = torch.randint(0, n // 20, (n,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).contiguous()
    torch.cuda.synchronize()
    return E


def ms(ts):
    t = 1e3 * np.asarray(ts)
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()), rounds=int(t.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--add", type=int, default=512)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, d, mn, mx = a.n, a.d, 5, 50
    full_ctx, seed_ctx = _lib.Context(0), _lib.Context(0)
    E = make_rows(n + a.add, d, 20261019)
    # the finished clustering and its state
    cid, rank, nc = full_ctx.cluster_dev(E.data_ptr(), n, d, mn, mx)
    log = full_ctx.last_merges()
    co = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    r = seed_ctx.cluster_seeded_dev(E.data_ptr(), n, d, np.ones(n, np.int32), mn, mx, 0, co.data_ptr())
    ones_equal = bool(r[3] == 0 and np.array_equal(seed_ctx.last_merges(), log) and np.array_equal(r[0], cid) and np.array_equal(r[1], rank))
    first, size = {i: i for i in range(n)}, {i: 1 for i in range(n)}
    for t, (x, y) in enumerate(log):
        first[n + t], size[n + t] = first.pop(int(x)), size.pop(int(x)) + size.pop(int(y))
        first.pop(int(y))
    ids = sorted(first)
    rows = torch.as_tensor(np.array([first[c] for c in ids], np.int64), device="cuda")
    seeds = torch.cat([co[rows], E[n:]]).contiguous()
    ss = np.concatenate([np.array([size[c] for c in ids], np.int32), np.ones(a.add, np.int32)])
    m = len(ss)
    del co
    torch.cuda.synchronize()
    stats = {}

    def resumed():
        out = seed_ctx.cluster_seeded_dev(seeds.data_ptr(), m, d, ss, mn, mx)
        assert out[3] == 0
        stats["seeded"] = dict(seed_ctx.last_ward_stats(), mode=list(seed_ctx.last_ward_mode()), **seed_ctx.last_stage_ms())

    def again():
        full_ctx.cluster_dev(E.data_ptr(), n + a.add, d, mn, mx)
        stats["full"] = dict(full_ctx.last_ward_stats(), mode=list(full_ctx.last_ward_mode()), **full_ctx.last_stage_ms())

    modes = {"icl_cluster_seeded_dev": resumed, "icl_cluster_dev_all_rows": again}
    for fn in modes.values():
        fn()
    ts = {k: [] for k in modes}
    for _ in range(a.rounds):
        for k, fn in modes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    out = dict(device="MI355X (1 GCD)", rows_clustered=n, rows_added=a.add, d=d, min_size=mn, max_size=mx, clusters_held=len(ids), seeds=m,
               seeded_merges=stats["seeded"]["merges"], all_ones_seeded_equals_icl_cluster_dev=ones_equal,
               wall_ms={k: ms(v) for k, v in ts.items()}, last_ward_stats=stats)
    w = out["wall_ms"]
    out["seeded_median_over_full_min"] = w["icl_cluster_seeded_dev"]["median"] / w["icl_cluster_dev_all_rows"]["min"]
    out["recommend_seeded_route"] = bool(w["icl_cluster_seeded_dev"]["median"] <= w["icl_cluster_dev_all_rows"]["min"])
    full_ctx.close()
    seed_ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
