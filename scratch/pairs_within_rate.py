"""icl_pairs_within_dev against the two routes that answer "which rows are duplicates of each other" today, on one device, inputs
resident, wall clock around a call that ends in a synchronise.

  rows       mixture-of-Gaussians rows (nearest_rate.py's recipe), d = 2048, with 2 % of the rows planted as near-copies of other rows
             (the source plus 1e-3 * noise).  The threshold lies between the planted pairs' largest value and the smallest other
             value, both taken from the oracle's matrix of a small set drawn by the same recipe (geometric mean of the two).
  no_matrix  n = 100 000: icl_pairs_within_dev against the icl_nearest_dev self-join at k = 10 (exclude[i] = i), the only route at
             this size today (its filter on the threshold is not timed).
  matrix     n = 20 000: against icl_ward_distance_matrix_dev + torch.nonzero on the thresholded lower triangle.

One untimed call of each mode, then the modes alternate round by round; min, median and max are reported.  The pairs of the two routes
and their values are compared as bit patterns.  Prints and writes one JSON object.

    python scratch/pairs_within_rate.py --out profiles/r29_pairs_within_rate.json
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from imageclust_amd import _lib  # noqa: E402


def make_rows(n, d, seed, planted=0.02):
    """-> (rows on the device, family[n] on the host: the row a planted row copies, itself for every other row)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cen = torch.randn((max(n // 20, 1), d), generator=g, device="cuda")
    lab = torch.randint(0, max(n // 20, 1), (n,), generator=g, device="cuda")
    E = (cen[lab] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).contiguous()
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    m = int(round(planted * n))
    copies, others = perm[:m], perm[m:]
    src = others[rng.integers(0, len(others), m)]
    E[torch.as_tensor(copies, device="cuda")] = E[torch.as_tensor(src, device="cuda")] + 1e-3 * torch.randn((m, d), generator=g, device="cuda")
    fam = np.arange(n)
    fam[copies] = src
    torch.cuda.synchronize()
    return E, fam


def planted_pairs(fam):
    c = np.bincount(fam)
    return int((c * (c - 1) // 2).sum())


def threshold_from_oracle(d, seed, n=1500):
    from oracle import oracle as O

    E, fam = make_rows(n, d, seed)
    V = np.asarray(O.initial_distance_matrix(E.cpu().numpy(), None), np.float32)
    i, j = np.tril_indices(n, -1)
    same = fam[i] == fam[j]
    pmax, omin = float(V[i, j][same].max()), float(V[i, j][~same].min())
    assert pmax < omin, (pmax, omin)
    return float(np.float32(np.sqrt(pmax * omin))), dict(n=n, planted_pairs=int(same.sum()), planted_max=pmax, other_min=omin)


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


class PairsCall:
    """icl_pairs_within_dev into preallocated device buffers: one call, no size query"""

    def __init__(self, ctx, X, n, d, thr, cap):
        self.ctx, self.X, self.n, self.d, self.thr, self.cap = ctx, X, n, d, thr, cap
        self.row_ptr = np.zeros(n + 1, np.int64)
        self.col = torch.empty(cap, dtype=torch.int32, device="cuda")
        self.val = torch.empty(cap, dtype=torch.float32, device="cuda")
        self.total = ctypes.c_int64(-1)

    def __call__(self):
        c = self.ctx
        _lib.check(c.h, c.L.icl_pairs_within_dev(c.h, self.X.data_ptr(), None, self.n, self.d, self.thr, self.row_ptr.ctypes.data,
                                                 self.col.data_ptr(), self.val.data_ptr(), self.cap, ctypes.byref(self.total)))
        c.sync()

    def keyed(self):
        """(i * n + j ascending, value bits) of the listed pairs"""
        t = self.total.value
        rows = torch.repeat_interleave(torch.arange(self.n, device="cuda"), torch.as_tensor(np.diff(self.row_ptr), device="cuda"))
        return rows * self.n + self.col[:t].long(), self.val[:t].view(torch.int32)


def sorted_keyed(i, j, v, n):
    key = i.long() * n + j.long()
    o = torch.argsort(key)
    return key[o], v[o].contiguous().view(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--matrix-n", type=int, default=20000)
    ap.add_argument("--big-n", type=int, default=100000)
    ap.add_argument("--out")
    a = ap.parse_args()
    d, k = a.d, 10
    ctx = _lib.Context(0)
    thr, how = threshold_from_oracle(d, 20261101)
    res = dict(device="MI355X (1 GCD)", d=d, rounds=a.rounds, planted_share=0.02, threshold=thr, threshold_from=how)

    # -- n = 20 000: against the distance matrix + nonzero
    n = a.matrix_n
    X, fam = make_rows(n, d, 20261102)
    new = PairsCall(ctx, X, n, d, thr, 4 * planted_pairs(fam) + 1024)
    D = torch.empty((n, n), dtype=torch.float32, device="cuda")
    out = {}

    def old():
        _lib.check(ctx.h, ctx.L.icl_ward_distance_matrix_dev(ctx.h, X.data_ptr(), None, n, d, D.data_ptr(), n))
        ctx.sync()
        out["ij"] = torch.nonzero(torch.tril(D <= thr, -1))
        torch.cuda.synchronize()

    w = alternate({"icl_pairs_within_dev": new, "distance_matrix_plus_nonzero": old}, a.rounds)
    ij = out["ij"]
    ok, ov = sorted_keyed(ij[:, 0], ij[:, 1], D[ij[:, 0], ij[:, 1]], n)
    nk, nv = new.keyed()
    res["matrix"] = dict(n=n, wall_ms=w, pairs=new.total.value, planted_pairs=planted_pairs(fam), pairs_stats=ctx.last_pairs_stats(),
                         same_pairs=bool(torch.equal(ok, nk)), values_equal_as_bits=bool(torch.equal(ok, nk) and torch.equal(ov, nv)),
                         composition_matrix_bytes=int(D.numel() * 4),
                         pairs_median_over_composition_min=w["icl_pairs_within_dev"]["median"] / w["distance_matrix_plus_nonzero"]["min"])
    del X, D, out, new, old, ij
    torch.cuda.empty_cache()

    # -- n = 100 000: against the nearest self-join
    n = a.big_n
    if n > 0:
        X, fam = make_rows(n, d, 20261103)
        new = PairsCall(ctx, X, n, d, thr, 4 * planted_pairs(fam) + 1024)
        ex = np.arange(n, dtype=np.int64)
        idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        val = torch.empty((n, k), dtype=torch.float32, device="cuda")

        def join():
            ctx.nearest_dev(X.data_ptr(), n, X.data_ptr(), n, d, k, idx.data_ptr(), val.data_ptr(), None, None, 0, ex)
            ctx.sync()

        w = alternate({"icl_pairs_within_dev": new, "icl_nearest_dev_self_join": join}, a.rounds)
        st = ctx.last_pairs_stats()  # (the last call of the alternation is the self-join: pairs' figures are the context's own)
        rows = torch.arange(n, device="cuda")[:, None].expand(n, k)
        keep = (val <= thr) & (idx >= 0) & (idx.long() < rows)  # each pair from its higher row
        jk, jv = sorted_keyed(rows[keep], idx[keep], val[keep], n)
        nk, nv = new.keyed()
        fam_max = int(np.bincount(fam).max())
        res["no_matrix"] = dict(n=n, k=k, wall_ms=w, pairs=new.total.value, planted_pairs=planted_pairs(fam), largest_family=fam_max,
                                pairs_stats=st, nearest_stats=ctx.last_nearest_stats(), matrix_bytes_avoided=4 * n * n,
                                same_pairs=bool(torch.equal(jk, nk)), values_equal_as_bits=bool(torch.equal(jk, nk) and torch.equal(jv, nv)),
                                pairs_median_over_self_join_min=w["icl_pairs_within_dev"]["median"] / w["icl_nearest_dev_self_join"]["min"],
                                recommend_pairs_within=bool(w["icl_pairs_within_dev"]["median"] <= w["icl_nearest_dev_self_join"]["min"]),
                                exact_tflops=3.0 * st["pairs"] * d / (w["icl_pairs_within_dev"]["median"] / 1e3) / 1e12)
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
