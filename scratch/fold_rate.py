"""icl_fold_centroids_dev against the numpy fold on the host, and deleting from a finished clustering against clustering again, on one
device; wall clock around a call that ends in a synchronise.

  library  100 000 rows x 2 048 on the device, 11 000 groups of 5 .. 50 members from a fixed seed, every row in one group.
           icl_fold_centroids_dev against the same fold in numpy on a host copy of the rows (the arithmetic of Clustering.keep_together,
           vectorised over the groups: step t of every group that has one in a single gather).  Both must return equal bits: asserted.
  delete   20 000 mixture-of-Gaussians rows, d = 2048, min 5 / max 50, clustered by Clustering.start; then remove() of 512 random ids +
           recluster() against Clustering.start on the 19 488 rows that remain (host rows, the host entry points: what a caller of the
           Python layer pays).  The two end in different partitions: the resumed run keeps what was formed.

One untimed call of each mode, then the modes alternate round by round.  Prints and writes one JSON object.

    python scratch/fold_rate.py --out profiles/r45_fold_rate.json
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib, clustering as CL  # noqa: E402


def ms(ts):
    t = 1e3 * np.asarray(ts)
    return dict(min=float(t.min()), median=float(np.median(t)), max=float(t.max()), rounds=int(t.size))


def alternate(modes, rounds):
    for fn in modes.values():
        fn()
    ts = {k: [] for k in modes}
    for _ in range(rounds):
        for k, fn in modes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    return {k: ms(v) for k, v in ts.items()}


def group_lengths(K, n, lo, hi, seed):
    """K lengths in [lo, hi] that add up to n, skewed: most groups short, some long"""
    rng = np.random.default_rng(seed)
    w = rng.exponential(size=K)
    lens = lo + np.minimum(np.floor(w / w.sum() * (n - lo * K)).astype(np.int64), hi - lo)
    while lens.sum() < n:
        room = np.flatnonzero(lens < hi)
        pick = rng.choice(room, min(len(room), int(n - lens.sum())), replace=False)
        lens[pick] += 1
    assert lens.sum() == n and lens.min() >= lo and lens.max() <= hi
    return lens


def host_fold(E, row_ptr, member):
    """The fold in numpy, singletons: step t of every group that has one, each operation rounded to fp32"""
    lens = np.diff(row_ptr)
    C = np.zeros((len(lens), E.shape[1]), np.float32)
    act = np.flatnonzero(lens > 0)
    C[act] = E[member[row_ptr[act]]]
    for t in range(1, int(lens.max())):
        act = np.flatnonzero(lens > t)
        C[act] = (np.float32(t) * C[act] + np.float32(1) * E[member[row_ptr[act] + t]]) / np.float32(t + 1)
    return C


def library(ctx, n, K, d, rounds):
    g = torch.Generator(device="cuda")
    g.manual_seed(20261021)
    E = torch.randn((n, d), generator=g, device="cuda").contiguous()
    C = torch.empty((K, d), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    Eh = E.cpu().numpy()
    lens = group_lengths(K, n, 5, 50, 1)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    member = np.random.default_rng(2).permutation(n).astype(np.int32)
    held = {}

    def device():
        ctx.fold_centroids_dev(E.data_ptr(), n, d, row_ptr, member, C.data_ptr())
        ctx.sync()

    def host():
        held["C"] = host_fold(Eh, row_ptr, member)

    wall = alternate({"icl_fold_centroids_dev": device, "numpy_fold_on_the_host": host}, rounds)
    device()
    equal = bool(np.array_equal(C.cpu().numpy().view(np.uint32), held["C"].view(np.uint32)))
    assert equal, "the device fold and the host fold differ"
    a, b = wall["icl_fold_centroids_dev"], wall["numpy_fold_on_the_host"]
    moved = (n + K) * d * 4
    return dict(rows=n, groups=K, d=d, group_lengths=dict(min=int(lens.min()), median=float(np.median(lens)), max=int(lens.max())), wall_ms=wall,
                both_routes_equal_as_bits=equal, fold_stats=ctx.last_fold_stats(), bytes_moved=moved,
                device_bytes_per_second_at_median=moved / (a["median"] * 1e-3), streaming_1x1_kernel_bytes_per_second=5.5e12,
                device_median_over_host_min=a["median"] / b["min"], recommend_device_fold=bool(a["median"] < b["min"]))


def delete(ctx, n, gone, d, mn, mx, rounds):
    g = torch.Generator(device="cuda")
    g.manual_seed(20261019)
    cen = torch.randn((n // 20, d), generator=g, device="cuda")
    lab = torch.randint(0, n // 20, (n,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).cpu().numpy()
    ids = ["i%d" % i for i in range(n)]
    out = np.random.default_rng(3).permutation(n)[:gone]
    keep = np.setdiff1d(np.arange(n), out)
    base = CL.Clustering.start(E, ids, mn, mx, ctx=ctx)
    assert base.ok
    held = {}

    def edited():
        st = held.pop("copy")
        st.remove([ids[i] for i in out])
        assert st.recluster()
        held["edited"] = st

    def again():
        held["again"] = CL.Clustering.start(E[keep], [ids[i] for i in keep], mn, mx, ctx=ctx)

    def timed_edit():  # (the copy of the state is made outside the clock)
        held["copy"] = copy.copy(base)
        held["copy"].clusters, held["copy"].embeddings = [copy.copy(c) for c in base.clusters], dict(base.embeddings)
        t0 = time.perf_counter()
        edited()
        return time.perf_counter() - t0

    timed_edit()
    again()
    ts = {"remove_plus_recluster": [], "start_on_the_remaining_rows": []}
    for _ in range(rounds):
        ts["remove_plus_recluster"].append(timed_edit())
        t0 = time.perf_counter()
        again()
        ts["start_on_the_remaining_rows"].append(time.perf_counter() - t0)
    wall = {k: ms(v) for k, v in ts.items()}
    a, b = wall["remove_plus_recluster"], wall["start_on_the_remaining_rows"]
    e, s = held["edited"], held["again"]
    return dict(rows=n, removed=gone, d=d, min_size=mn, max_size=mx, clusters_before=len(base.clusters), fold_stats=ctx.last_fold_stats(),
                merges_after_the_edit=int(len(e.last_merges)), wall_ms=wall, kept_clusters=dict(edited=len(e.as_map()), again=len(s.as_map())),
                same_partition=bool(sorted(map(sorted, e.as_map().values())) == sorted(map(sorted, s.as_map().values()))),
                edit_median_over_start_min=a["median"] / b["min"], recommend_edit_route=bool(a["median"] < b["min"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--skip-delete", action="store_true")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    res = dict(device="MI355X (1 GCD)", rounds=a.rounds, library=library(ctx, 100000, 11000, a.d, a.rounds))
    if not a.skip_delete:
        res["delete"] = delete(ctx, 20000, 512, a.d, 5, 50, a.rounds)
    res["not_measured"] = ["d = 1000 + labels", "one group of 100 000 members", "several devices"]
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
