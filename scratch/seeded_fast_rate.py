"""Seeded clustering in FAST mode against the exact seeded call, on one device: icl_cluster_seeded_fast_dev against icl_cluster_seeded_dev on
the same seeds, at two shapes.

  adding    README's adding shape: 20 000 mixture-of-Gaussians rows of d = 2048 clustered at min 5 / max 50 (untimed), the final clusters --
            dropped ones included -- with the centroids the exact engine holds, plus 512 more rows as singleton seeds: 2 712 seeds.
  library   a library-sized state: 11 000 clusters of 5 .. 40 items around their own blob centres plus 20 000 singletons drawn around the same
            centres, d = 2048, min 5 / max 50, k_target = 11 000 (the library takes the new images in: 20 000 merges asked for).

Inputs are resident on the device; wall clock around a call that ends in a synchronise (the results are on the host when it returns).  Each mode
has a context of its own, one untimed call of each, then the modes alternate round by round.  Beside min / median / max: the stage split of
icl_last_stage_ms, the loop's counters, and the Rand index between the two partitions of the seeds (sampled pairs).  The FAST route is called
recommended for a shape only where its median is below the exact call's minimum in this run.  Prints and writes one JSON object.

    python scratch/seeded_fast_rate.py --out profiles/r42_seeded_fast_rate.json
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


def gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def ms(ts):
    t = 1e3 * np.asarray(ts)
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()), rounds=int(t.size))


def rand_index(a, b, pairs=200000, seed=0):
    """Over sampled pairs of seeds: the share on which the two partitions agree (a dropped seed, id -1, shares a cluster with nobody)."""
    rng = np.random.default_rng(seed)
    i, j = rng.integers(0, len(a), pairs), rng.integers(0, len(a), pairs)
    keep = i != j
    i, j = i[keep], j[keep]
    sa = (a[i] == a[j]) & (a[i] >= 0)
    sb = (b[i] == b[j]) & (b[i] >= 0)
    return float((sa == sb).mean())


def adding_shape(ctx, n, add, d, mn, mx):
    """-> (seeds on the device, seed_size, k_target)"""
    g = gen(20261019)
    cen = torch.randn((n // 20, d), generator=g, device="cuda")
    lab = torch.randint(0, n // 20, (n + add,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n + add, d), generator=g, device="cuda")).contiguous()
    co = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r = ctx.cluster_seeded_dev(E.data_ptr(), n, d, np.ones(n, np.int32), mn, mx, 0, co.data_ptr())
    assert r[3] == 0
    log = ctx.last_merges()
    first, size = {i: i for i in range(n)}, {i: 1 for i in range(n)}
    for t, (x, y) in enumerate(log):
        first[n + t], size[n + t] = first.pop(int(x)), size.pop(int(x)) + size.pop(int(y))
        first.pop(int(y))
    ids = sorted(first)
    rows = torch.as_tensor(np.array([first[c] for c in ids], np.int64), device="cuda")
    seeds = torch.cat([co[rows], E[n:]]).contiguous()
    ss = np.concatenate([np.array([size[c] for c in ids], np.int32), np.ones(add, np.int32)])
    torch.cuda.synchronize()
    return seeds, ss, 0


def library_shape(clusters, singles, d):
    g = gen(20261021)
    cen = torch.randn((clusters, d), generator=g, device="cuda")
    sizes = torch.randint(5, 41, (clusters,), generator=g, device="cuda")
    held = cen + 0.1 * torch.randn((clusters, d), generator=g, device="cuda") / sizes.sqrt()[:, None]  # a mean of `size` draws around the centre
    lab = torch.randint(0, clusters, (singles,), generator=g, device="cuda")
    new = cen[lab] + 0.1 * torch.randn((singles, d), generator=g, device="cuda")
    seeds = torch.cat([held, new]).contiguous()
    ss = np.concatenate([sizes.cpu().numpy().astype(np.int32), np.ones(singles, np.int32)])
    torch.cuda.synchronize()
    return seeds, ss, clusters


def measure(name, seeds, ss, mn, mx, kt, rounds, ctxs):
    m, d = seeds.shape
    stats, ids = {}, {}

    def call(mode):
        c = ctxs[mode]
        out = c.cluster_seeded_dev(seeds.data_ptr(), m, d, ss, mn, mx, kt, update=_lib.UPDATE_LW if mode == "fast" else _lib.UPDATE_EXACT)
        assert out[3] == 0, (name, mode, out[3])
        ids[mode] = (out[0].copy(), int(out[2]))
        stats[mode] = dict(c.last_ward_stats(), mode=list(c.last_ward_mode()), **c.last_stage_ms())

    for mode in ("fast", "exact"):
        call(mode)
    ts = {"fast": [], "exact": []}
    for _ in range(rounds):
        for mode in ("fast", "exact"):
            t0 = time.perf_counter()
            call(mode)
            ts[mode].append(time.perf_counter() - t0)
    w = {"icl_cluster_seeded_fast_dev": ms(ts["fast"]), "icl_cluster_seeded_dev": ms(ts["exact"])}
    return dict(seeds=int(m), items=int(np.abs(ss).sum()), d=int(d), min_size=mn, max_size=mx, k_target=int(kt), wall_ms=w,
                last_ward_stats={"icl_cluster_seeded_fast_dev": stats["fast"], "icl_cluster_seeded_dev": stats["exact"]},
                n_clusters={"fast": ids["fast"][1], "exact": ids["exact"][1]}, rand_index_fast_vs_exact=rand_index(ids["fast"][0], ids["exact"][0]),
                identical_ids=float((ids["fast"][0] == ids["exact"][0]).mean()),
                fast_median_over_exact_min=w["icl_cluster_seeded_fast_dev"]["median"] / w["icl_cluster_seeded_dev"]["min"],
                recommend_fast_route=bool(w["icl_cluster_seeded_fast_dev"]["median"] < w["icl_cluster_seeded_dev"]["min"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--add", type=int, default=512)
    ap.add_argument("--clusters", type=int, default=11000)
    ap.add_argument("--singles", type=int, default=20000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    mn, mx = 5, 50
    ctxs = {"fast": _lib.Context(0), "exact": _lib.Context(0)}
    out = dict(device="MI355X (1 GCD)")
    seeds, ss, kt = adding_shape(ctxs["exact"], a.n, a.add, a.d, mn, mx)
    out["adding"] = measure("adding", seeds, ss, mn, mx, kt, a.rounds, ctxs)
    del seeds
    seeds, ss, kt = library_shape(a.clusters, a.singles, a.d)
    out["library"] = measure("library", seeds, ss, mn, mx, kt, a.rounds, ctxs)
    for c in ctxs.values():
        c.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
