"""icl_nearest_dev against the route it replaces -- icl_ward_distance_matrix_dev over queries and library together, then a device sort
(torch.topk) -- on one device, inputs resident, wall clock around a call that ends in a synchronise.

  library    256 singleton queries against 11 000 clusters with sizes in [5, 50], d = 2048, k = 10, max_size = 50.  The composition
             builds the matrix of the 11 256 stacked rows and sorts the query block.
  self_join  n = 20 000, d = 2048, k = 10, exclude[i] = i, against the n x n matrix plus topk (k + 1: the diagonal's zero comes first).
             icl_nearest_dev evaluates (i, j) and (j, i) both; the matrix kernel evaluates each pair once.
  no_matrix  one self-join at n = 100 000, k = 10 (the matrix would be 40 GB beside its sort buffers): time and workspace bytes.

One untimed call of each mode, then the modes alternate round by round.  The values of the two routes are compared as bit patterns
(without the ban, which the composition does not apply).  Prints and writes one JSON object.

    python scratch/nearest_rate.py --out profiles/r27_nearest_rate.json
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
    cen = torch.randn((max(n // 20, 1), d), generator=g, device="cuda")
    lab = torch.randint(0, max(n // 20, 1), (n,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).contiguous()
    torch.cuda.synchronize()
    return E


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


def verdict(w):
    new, old = w["icl_nearest_dev"], w["distance_matrix_plus_topk"]
    return dict(nearest_median_over_composition_min=new["median"] / old["min"], recommend_nearest=bool(new["median"] <= old["min"]))


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def compare(ctx, X, rows, nq, d, k, sizes_dev, q_size, e_size, exclude, col0, drop):
    """nearest_dev on (X[:nq], X[col0:]) against the matrix of X's rows + topk; `drop` leading entries of the sort are the diagonal"""
    n = rows - col0
    idx = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    val = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    D = torch.empty((rows, rows), dtype=torch.float32, device="cuda")
    out = {}

    def new(max_size=0):
        ctx.nearest_dev(X.data_ptr(), nq, X.data_ptr() + col0 * d * 4, n, d, k, idx.data_ptr(), val.data_ptr(), q_size, e_size, max_size, exclude)
        ctx.sync()

    def old():
        _lib.check(ctx.h, ctx.L.icl_ward_distance_matrix_dev(ctx.h, X.data_ptr(), sizes_dev.data_ptr() if sizes_dev is not None else None, rows, d,
                                                             D.data_ptr(), rows))
        ctx.sync()
        out["topk"] = torch.topk(D[:nq, col0:], k + drop, dim=1, largest=False, sorted=True)
        torch.cuda.synchronize()

    new()
    old()
    out["values_equal_as_bits"] = same_bits(val, out["topk"].values[:, drop:].contiguous())
    return new, old, out, D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--self-n", type=int, default=20000)
    ap.add_argument("--big-n", type=int, default=100000)
    ap.add_argument("--out")
    a = ap.parse_args()
    d, k = a.d, 10
    ctx = _lib.Context(0)
    res = dict(device="MI355X (1 GCD)", d=d, k=k, rounds=a.rounds)

    # -- library shape
    nq, n, mx = 256, 11000, 50
    X = make_rows(nq + n, d, 20261019)
    es = np.random.default_rng(1).integers(5, 51, n).astype(np.int32)
    stacked = np.concatenate([np.ones(nq, np.int32), es])
    s_dev = torch.as_tensor(stacked, device="cuda")
    new, old, out, D = compare(ctx, X, nq + n, nq, d, k, s_dev, None, es, None, nq, 0)
    w = alternate({"icl_nearest_dev": lambda: new(mx), "distance_matrix_plus_topk": old}, a.rounds)
    new(mx)
    res["library"] = dict(queries=nq, clusters=n, sizes="[5, 50]", max_size=mx, wall_ms=w, values_equal_as_bits=out["values_equal_as_bits"],
                          nearest_stats=ctx.last_nearest_stats(), composition_matrix_bytes=int(D.numel() * 4), **verdict(w))
    del X, D, out, new, old
    torch.cuda.empty_cache()

    # -- self-join
    n = a.self_n
    X = make_rows(n, d, 20261020)
    ex = np.arange(n, dtype=np.int64)
    new, old, out, D = compare(ctx, X, n, n, d, k, None, None, None, ex, 0, 1)
    w = alternate({"icl_nearest_dev": new, "distance_matrix_plus_topk": old}, a.rounds)
    res["self_join"] = dict(n=n, wall_ms=w, values_equal_as_bits=out["values_equal_as_bits"], nearest_stats=ctx.last_nearest_stats(),
                            composition_matrix_bytes=int(D.numel() * 4),
                            note="icl_nearest_dev evaluates (i, j) and (j, i); the matrix kernel evaluates each pair once", **verdict(w))
    del X, D, out, new, old
    torch.cuda.empty_cache()

    # -- no matrix
    n = a.big_n
    if n > 0:
        X = make_rows(n, d, 20261021)
        ex = np.arange(n, dtype=np.int64)
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        val = torch.empty((n, k), dtype=torch.float32, device="cuda")
        t0 = time.perf_counter()
        ctx.nearest_dev(X.data_ptr(), n, X.data_ptr(), n, d, k, idx.data_ptr(), val.data_ptr(), None, None, 0, ex)
        ctx.sync()
        t = time.perf_counter() - t0
        st = ctx.last_nearest_stats()
        ok = bool((idx >= 0).all().item() and (val[:, 1:] >= val[:, :-1]).all().item() and (idx != torch.arange(n, device="cuda", dtype=torch.int32)[:, None]).all().item())
        res["no_matrix"] = dict(n=n, wall_ms_one_call=1e3 * t, nearest_stats=st, rows_ascending_and_no_self=ok, matrix_bytes_avoided=4 * n * n,
                                exact_tflops=3.0 * st["pairs"] * d / t / 1e12)
    else:
        res["no_matrix"] = "not measured"
    ctx.close()
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
