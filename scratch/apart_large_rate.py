"""icl_cluster_apart_dev on one device: what the keep-apart relation costs on the one-merge-per-step loop, what leaving the batched loop costs,
and the call on a library-sized state that no other route takes.

(a) The shape of scratch/seeded_large_rate.py: 20 000 mixture-of-Gaussians rows of d = 2048 clustered at min 5 / max 50 (untimed), the
    final clusters with the centroids the engine holds plus 512 new singletons as seeds.  icl_cluster_apart_dev with an EMPTY relation
    against icl_cluster_seeded_dev in the same process (the seeded call runs the batched loop there), and both again in a child process
    under ICL_WARD_BATCH=0 (read once per process), where the seeded call runs the one-merge-per-step loop too: the second pair is the
    price of the bit reads and the commit launch, the first pair adds the price of leaving the batched loop.
(b) 100 000 such rows clustered at min 5 / max 50 (untimed); every final cluster, kept or dropped, is a seed (centroid: the fp32 mean of its
    rows), every kept cluster is in class 1 and k_target is their number: "put the leftovers somewhere".  No comparator: no other call
    takes this problem.  Recorded: wall time, merges, the bit table's bytes, the images of dropped clusters that end in a kept cluster.

Timed: wall clock around a call that returns with its results on the host, inputs resident on the device; one untimed call of each
mode, then the modes alternate over the rounds.  Prints and writes one JSON object.

    python scratch/apart_large_rate.py --out profiles/r40_apart_large_rate.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(n, d, seed):
    import torch

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


def final_list(n, log):
    """creation id -> member rows of every final cluster of a run from n singletons, ascending creation id"""
    mem = {i: [i] for i in range(n)}
    for t, (x, y) in enumerate(log):
        mem[n + t] = mem.pop(int(x)) + mem.pop(int(y))
    return [mem[c] for c in sorted(mem)]


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


def part_a(a):
    import torch

    from imageclust_amd import _lib

    n, add, d, mn, mx = 20000, 512, a.d, 5, 50
    full, c_seed, c_apart = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    E = make_rows(n + add, d, 20261019)
    full.cluster_dev(E.data_ptr(), n, d, mn, mx)
    log = full.last_merges()
    full.close()
    co = torch.zeros((n, d), dtype=torch.float32, device="cuda")
    r = c_seed.cluster_seeded_dev(E.data_ptr(), n, d, np.ones(n, np.int32), mn, mx, 0, co.data_ptr())
    assert r[3] == 0 and np.array_equal(c_seed.last_merges(), log)
    lists = final_list(n, log)
    rows = torch.as_tensor(np.array([m[0] for m in lists], np.int64), device="cuda")
    seeds = torch.cat([co[rows], E[n:]]).contiguous()
    ss = np.concatenate([np.array([len(m) for m in lists], np.int32), np.ones(add, np.int32)])
    m = len(ss)
    del co
    torch.cuda.synchronize()
    stats, logs = {}, {}

    def seeded():
        out = c_seed.cluster_seeded_dev(seeds.data_ptr(), m, d, ss, mn, mx)
        assert out[3] == 0
        stats["seeded"], logs["seeded"] = dict(c_seed.last_ward_stats(), mode=list(c_seed.last_ward_mode()), **c_seed.last_stage_ms()), c_seed.last_merges()

    def apart():
        out = c_apart.cluster_apart_dev(seeds.data_ptr(), m, d, ss, mn, mx, 0, np.zeros(m, np.int32), None)
        assert out[3] == 0
        stats["apart"], logs["apart"] = dict(c_apart.last_ward_stats(), mode=list(c_apart.last_ward_mode()), **c_apart.last_stage_ms()), c_apart.last_merges()

    wall = alternate({"icl_cluster_apart_dev_empty_relation": apart, "icl_cluster_seeded_dev": seeded}, a.rounds)
    out = dict(seeds=m, clusters_held=len(lists), rows_added=add, d=d, min_size=mn, max_size=mx, ICL_WARD_BATCH=os.environ.get("ICL_WARD_BATCH", "unset"),
               same_log=bool(np.array_equal(logs["seeded"], logs["apart"])), wall_ms=wall, last_ward_stats=stats,
               apart_median_over_seeded_median=wall["icl_cluster_apart_dev_empty_relation"]["median"] / wall["icl_cluster_seeded_dev"]["median"])
    c_seed.close()
    c_apart.close()
    return out


def part_b(a):
    import torch

    from imageclust_amd import _lib

    n, d, mn, mx = a.n, a.d, 5, 50
    full = _lib.Context(0)
    E = make_rows(n, d, 20261020)
    full.cluster_dev(E.data_ptr(), n, d, mn, mx)
    log = full.last_merges()
    full.close()   # (its workspace goes back before the constrained call takes its own)
    lists = final_list(n, log)
    m = len(lists)
    ss = np.array([len(x) for x in lists], np.int32)
    owner = np.empty(n, np.int64)
    for q, x in enumerate(lists):
        owner[x] = q
    cen = torch.zeros((m, d), dtype=torch.float32, device="cuda").index_add_(0, torch.as_tensor(owner, device="cuda"), E)
    cen /= torch.as_tensor(ss, device="cuda").to(torch.float32)[:, None]
    cen = cen.contiguous()
    del E
    torch.cuda.synchronize()
    kept = ss >= mn
    cls = kept.astype(np.int32)
    ctx = _lib.Context(0)
    res = {}

    def absorb():
        res["r"] = ctx.cluster_apart_dev(cen.data_ptr(), m, d, ss, mn, mx, int(kept.sum()), cls, None)
        assert res["r"][3] == 0

    wall = alternate({"icl_cluster_apart_dev": absorb}, a.rounds)
    cid = res["r"][0]
    anchors = set(int(c) for c in cid[kept])
    placed = np.array([(not kept[i]) and int(cid[i]) in anchors for i in range(m)])
    out = dict(rows=n, d=d, min_size=mn, max_size=mx, seeds=m, kept_clusters=int(kept.sum()), leftover_clusters=int((~kept).sum()),
               leftover_images=int(ss[~kept].sum()), leftover_images_in_a_kept_cluster=int(ss[placed].sum()), k_target=int(kept.sum()),
               table_bytes=int(m * ((m + 31) // 32) * 4), wall_ms=wall["icl_cluster_apart_dev"],
               last_ward_stats=dict(ctx.last_ward_stats(), mode=list(ctx.last_ward_mode()), **ctx.last_stage_ms()),
               clusters_after=int(res["r"][2]))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--part", default="all")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.part == "a":   # (the child: one JSON line)
        print(json.dumps(part_a(a)))
        return
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "a", "--d", str(a.d), "--rounds", str(a.rounds)],
                       env=dict(os.environ, ICL_WARD_BATCH="0"), capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("the ICL_WARD_BATCH=0 child failed (%d):\n%s" % (p.returncode, p.stderr[-3000:]))
    one_step = json.loads(p.stdout.strip().split("\n")[-1])
    out = dict(device="MI355X (1 GCD)", a_r25_shape=dict(batched_default=part_a(a), one_merge_per_step_child=one_step), b_library_shape=part_b(a),
               not_measured=["100 000 seeds (the bit table would take 1.25 GB)", "a relation of explicit pairs at library size", "several devices"])
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
