"""icl_cluster_fit_dev against the composition that does without its fused epilogue -- icl_nearest_dev with exclude = cluster_of for the
alternatives, plus icl_ward_values_at_dev on the pairs (i, cluster_of[i]) for the own costs -- on one device, inputs resident, wall
clock around a call that ends in a synchronise.

  library  100 000 singleton rows against 11 000 clusters with sizes in [5, 50], d = 2048, k_alt = 1, max_size = 50, no frozen cluster
           (the composition cannot leave frozen columns out).  Both routes must return equal bits: asserted.
  own_only the same shape with k_alt = 0: only the listed-pair kernel runs.
  small    20 000 rows against 2 200 clusters, otherwise as library.

One untimed call of each mode, then the modes alternate round by round.  Prints and writes one JSON object.

    python scratch/cluster_fit_rate.py --out profiles/r32_cluster_fit_rate.json
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


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def point(ctx, nq, K, d, k_alt, max_size, rounds, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    C = torch.randn((K, d), generator=g, device="cuda").contiguous()
    cof_dev = torch.randint(0, K, (nq,), generator=g, device="cuda")
    Q = (C[cof_dev] + 0.1 * torch.randn((nq, d), generator=g, device="cuda")).contiguous()
    torch.cuda.synchronize()
    cof = cof_dev.cpu().numpy().astype(np.int32)
    c_size = np.random.default_rng(seed).integers(5, 51, K).astype(np.int32)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device="cuda")
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    own, ai, av, listed, rep, worst = f32(nq), i32(nq, max(k_alt, 1)), f32(nq, max(k_alt, 1)), i32(K), i32(K), i32(K)
    own_b, ai_b, av_b = f32(nq), i32(nq, max(k_alt, 1)), f32(nq, max(k_alt, 1))
    rows = np.arange(nq, dtype=np.int32)
    stats = {}

    def fused(k=k_alt):
        ctx.cluster_fit_dev(Q.data_ptr(), cof, nq, C.data_ptr(), K, d, k, own.data_ptr(), ai.data_ptr(), av.data_ptr(), listed.data_ptr(),
                            rep.data_ptr(), worst.data_ptr(), c_size=c_size, max_size=max_size)
        ctx.sync()

    def composed():
        ctx.nearest_dev(Q.data_ptr(), nq, C.data_ptr(), K, d, k_alt, ai_b.data_ptr(), av_b.data_ptr(), None, c_size, max_size, cof.astype(np.int64))
        stats["nearest"] = ctx.last_nearest_stats()
        ctx.ward_values_at_dev(Q.data_ptr(), nq, C.data_ptr(), K, d, rows, cof, own_b.data_ptr(), e_size=c_size)
        ctx.sync()

    def nearest_alone():
        ctx.nearest_dev(Q.data_ptr(), nq, C.data_ptr(), K, d, k_alt, ai_b.data_ptr(), av_b.data_ptr(), None, c_size, max_size, cof.astype(np.int64))
        ctx.sync()

    def values_alone():
        ctx.ward_values_at_dev(Q.data_ptr(), nq, C.data_ptr(), K, d, rows, cof, own_b.data_ptr(), e_size=c_size)
        ctx.sync()

    wall = alternate({"icl_cluster_fit_dev": fused, "nearest_dev_plus_values_at_dev": composed, "nearest_dev_alone": nearest_alone,
                      "values_at_dev_alone": values_alone}, rounds)
    fused()
    stats["fit"] = ctx.last_fit_stats()
    composed()
    equal = same_bits(own, own_b) and bool(torch.equal(ai, ai_b)) and same_bits(av, av_b)
    assert equal, "the fused call and the composition differ"
    a, b = wall["icl_cluster_fit_dev"], wall["nearest_dev_plus_values_at_dev"]
    out = dict(rows=nq, clusters=K, d=d, k_alt=k_alt, max_size=max_size, sizes="[5, 50]", wall_ms=wall, both_routes_equal_as_bits=equal,
               fit_stats=stats["fit"], nearest_stats_of_the_composition=stats["nearest"], fused_median_over_composition_min=a["median"] / b["min"],
               recommend_fused=bool(a["median"] <= b["min"]),
               slower_stage_of_the_composition=max(("nearest_dev_alone", "values_at_dev_alone"), key=lambda m: wall[m]["median"]))
    own_wall = alternate({"icl_cluster_fit_dev_k_alt_0": lambda: fused(0)}, rounds)
    fused(0)
    out["own_only"] = dict(k_alt=0, wall_ms=own_wall, fit_stats=ctx.last_fit_stats(), own_equal_as_bits=same_bits(own, own_b))
    assert out["own_only"]["own_equal_as_bits"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--small", action="store_true", help="also the 20 000 x 2 200 point")
    a = ap.parse_args()
    ctx = _lib.Context(0)
    res = dict(device="MI355X (1 GCD)", rounds=a.rounds, library=point(ctx, 100000, 11000, a.d, 1, 50, a.rounds, 1))
    if a.small:
        res["small"] = point(ctx, 20000, 2200, a.d, 1, 50, a.rounds, 2)
    ctx.close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
