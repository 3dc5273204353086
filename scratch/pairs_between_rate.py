"""icl_pairs_between_dev against the routes that answer "which new rows duplicate which library rows" without it, on one device, inputs
resident, wall clock around a call that ends in a synchronise.

  rows     mixture-of-Gaussians rows (nearest_rate.py's recipe) on both sides, d = 2048, with 2 % of the queries planted as near-copies of
           library rows (the source plus 1e-3 * noise).  The threshold lies between the planted pairs' largest value and the smallest
           other value, both taken from the oracle's values of a small problem drawn by the same recipe (geometric mean of the two).
  library  256 x 11 000: icl_pairs_between_dev against icl_nearest_dev at k = 64 (its filter on the threshold is not timed) and against
           icl_ward_distance_matrix_dev on the stacked rows + torch.nonzero of the block.
  bulk     20 000 x 100 000: against icl_nearest_dev at k = 10.
  dense    256 x 11 000 with threshold = +Inf (every pair listed): the engine's split count against one split per band.

One untimed call of each mode, then the modes alternate round by round; min, median and max are reported.  The pairs of the routes and
their values are compared as bit patterns.  Prints and writes one JSON object.

    python scratch/pairs_between_rate.py --out profiles/r35_pairs_between_rate.json
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


def make_sets(nq, n, d, seed, planted=0.02):
    """-> (Q, L on the device, fam[nq] on the host: the library row a planted query copies, -1 for every other query)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    ncen = max(n // 20, 1)
    cen = torch.randn((ncen, d), generator=g, device="cuda")
    L = (cen[torch.randint(0, ncen, (n,), generator=g, device="cuda")] + 0.1 * torch.randn((n, d), generator=g, device="cuda")).contiguous()
    Q = (cen[torch.randint(0, ncen, (nq,), generator=g, device="cuda")] + 0.1 * torch.randn((nq, d), generator=g, device="cuda")).contiguous()
    rng = np.random.default_rng(seed)
    m = max(int(round(planted * nq)), 1)
    copies = rng.permutation(nq)[:m]
    src = rng.integers(0, n, m)
    Q[torch.as_tensor(copies, device="cuda")] = L[torch.as_tensor(src, device="cuda")] + 1e-3 * torch.randn((m, d), generator=g, device="cuda")
    fam = np.full(nq, -1, np.int64)
    fam[copies] = src
    torch.cuda.synchronize()
    return Q, L, fam


def threshold_from_oracle(d, seed, nq=300, n=1500):
    from oracle import oracle as O

    Q, L, fam = make_sets(nq, n, d, seed)
    V = np.asarray(O.initial_distance_matrix(torch.cat([Q, L]).cpu().numpy(), None), np.float32)[:nq, nq:]
    same = np.zeros(V.shape, bool)
    same[np.flatnonzero(fam >= 0), fam[fam >= 0]] = True
    pmax, omin = float(V[same].max()), float(V[~same].min())
    assert pmax < omin, (pmax, omin)
    return float(np.float32(np.sqrt(pmax * omin))), dict(nq=nq, n=n, planted_pairs=int(same.sum()), planted_max=pmax, other_min=omin)


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


class BetweenCall:
    """icl_pairs_between_dev into preallocated device buffers: one call, no size query"""

    def __init__(self, ctx, Q, L, d, thr, cap, splits=0):
        self.ctx, self.Q, self.L, self.nq, self.n, self.d, self.thr, self.cap, self.splits = ctx, Q, L, len(Q), len(L), d, thr, cap, splits
        self.row_ptr = np.zeros(self.nq + 1, np.int64)
        self.col = torch.empty(cap, dtype=torch.int32, device="cuda")
        self.val = torch.empty(cap, dtype=torch.float32, device="cuda")
        self.total = ctypes.c_int64(-1)

    def __call__(self):
        c = self.ctx
        c.set_nearest_options(self.splits)
        _lib.check(c.h, c.L.icl_pairs_between_dev(c.h, self.Q.data_ptr(), None, self.nq, self.L.data_ptr(), None, self.n, self.d, self.thr, None,
                                                  self.row_ptr.ctypes.data, self.col.data_ptr(), self.val.data_ptr(), self.cap, ctypes.byref(self.total)))
        c.sync()
        c.set_nearest_options(0)

    def keyed(self):
        """(i * n + j ascending, value bits) of the listed pairs"""
        t = self.total.value
        rows = torch.repeat_interleave(torch.arange(self.nq, device="cuda"), torch.as_tensor(np.diff(self.row_ptr), device="cuda"))
        return rows * self.n + self.col[:t].long(), self.val[:t].view(torch.int32)


def sorted_keyed(i, j, v, n):
    key = i.long() * n + j.long()
    o = torch.argsort(key)
    return key[o], v[o].contiguous().view(torch.int32)


def nearest_route(ctx, Q, L, d, k, thr):
    nq, n = len(Q), len(L)
    idx = torch.empty((nq, k), dtype=torch.int32, device="cuda")
    val = torch.empty((nq, k), dtype=torch.float32, device="cuda")

    def call():
        ctx.nearest_dev(Q.data_ptr(), nq, L.data_ptr(), n, d, k, idx.data_ptr(), val.data_ptr())
        ctx.sync()

    def keyed():
        rows = torch.arange(nq, device="cuda")[:, None].expand(nq, k)
        keep = (val <= thr) & (idx >= 0)
        return sorted_keyed(rows[keep], idx[keep], val[keep], n)

    return call, keyed


def against(new, keyed):
    (ak, av), (bk, bv) = new.keyed(), keyed()
    same = bool(torch.equal(ak, bk))
    return dict(same_pairs=same, values_equal_as_bits=bool(same and torch.equal(av, bv)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--lib", type=int, nargs=2, default=[256, 11000])
    ap.add_argument("--bulk", type=int, nargs=2, default=[20000, 100000], help="0 0: leave the bulk shape out")
    ap.add_argument("--out")
    a = ap.parse_args()
    d = a.d
    ctx = _lib.Context(0)
    thr, how = threshold_from_oracle(d, 20261201)
    res = dict(device="MI355X (1 GCD)", d=d, rounds=a.rounds, planted_share=0.02, threshold=thr, threshold_from=how)

    # -- library shape: against nearest at k = 64 and against the distance matrix of the stacked rows
    nq, n = a.lib
    Q, L, fam = make_sets(nq, n, d, 20261202)
    planted = int((fam >= 0).sum())
    new = BetweenCall(ctx, Q, L, d, thr, 4 * planted + 1024)
    near, near_keyed = nearest_route(ctx, Q, L, d, 64, thr)
    S = torch.cat([Q, L]).contiguous()
    D = torch.empty((nq + n, nq + n), dtype=torch.float32, device="cuda")
    out = {}

    def matrix():
        _lib.check(ctx.h, ctx.L.icl_ward_distance_matrix_dev(ctx.h, S.data_ptr(), None, nq + n, d, D.data_ptr(), nq + n))
        ctx.sync()
        out["ji"] = torch.nonzero(D[nq:, :nq] <= thr)  # the lower triangle's block: rows are library rows, columns queries
        torch.cuda.synchronize()

    w = alternate({"icl_pairs_between_dev": new, "icl_nearest_dev_k64": near, "distance_matrix_plus_nonzero": matrix}, a.rounds)
    new()
    st = ctx.last_pairs_between_stats()
    ji = out["ji"]
    m = w["icl_pairs_between_dev"]["median"]
    res["library"] = dict(nq=nq, n=n, wall_ms=w, pairs=new.total.value, planted_pairs=planted, between_stats=st,
                          nearest_stats=ctx.last_nearest_stats(), against_nearest_k64=against(new, near_keyed),
                          against_matrix=against(new, lambda: sorted_keyed(ji[:, 1], ji[:, 0], D[nq:, :nq][ji[:, 0], ji[:, 1]], n)),
                          composition_matrix_bytes=int(D.numel() * 4),
                          between_median_over_nearest_min=m / w["icl_nearest_dev_k64"]["min"],
                          between_median_over_matrix_min=m / w["distance_matrix_plus_nonzero"]["min"],
                          recommend_between=bool(m < min(w["icl_nearest_dev_k64"]["min"], w["distance_matrix_plus_nonzero"]["min"])),
                          exact_tflops=3.0 * st["pairs"] * d / (m / 1e3) / 1e12)
    del S, D, out, ji, near, near_keyed

    # -- dense: every pair listed, the engine's split count against one split per band
    auto, one = BetweenCall(ctx, Q, L, d, float("inf"), nq * n), BetweenCall(ctx, Q, L, d, float("inf"), nq * n, splits=1)
    w = alternate({"auto_splits": auto, "one_split": one}, a.rounds)
    auto()
    st_auto = ctx.last_pairs_between_stats()
    one()
    st_one = ctx.last_pairs_between_stats()
    res["dense"] = dict(nq=nq, n=n, threshold="+Inf", wall_ms=w, pairs=auto.total.value, stats_auto=st_auto, stats_one_split=st_one,
                        both_equal_as_bits=bool(np.array_equal(auto.row_ptr, one.row_ptr) and torch.equal(auto.col, one.col) and
                                                torch.equal(auto.val.view(torch.int32), one.val.view(torch.int32))),
                        auto_median_over_one_split_min=w["auto_splits"]["median"] / w["one_split"]["min"])
    del Q, L, new, auto, one
    torch.cuda.empty_cache()

    # -- bulk upload: against nearest at k = 10
    nq, n = a.bulk
    if nq > 0 and n > 0:
        Q, L, fam = make_sets(nq, n, d, 20261203)
        planted = int((fam >= 0).sum())
        new = BetweenCall(ctx, Q, L, d, thr, 4 * planted + 1024)
        near, near_keyed = nearest_route(ctx, Q, L, d, 10, thr)
        w = alternate({"icl_pairs_between_dev": new, "icl_nearest_dev_k10": near}, a.rounds)
        new()
        st = ctx.last_pairs_between_stats()
        m = w["icl_pairs_between_dev"]["median"]
        res["bulk"] = dict(nq=nq, n=n, wall_ms=w, pairs=new.total.value, planted_pairs=planted, between_stats=st, nearest_stats=ctx.last_nearest_stats(),
                           against_nearest_k10=against(new, near_keyed), matrix_bytes_avoided=4 * nq * n,
                           between_median_over_nearest_min=m / w["icl_nearest_dev_k10"]["min"],
                           recommend_between=bool(m < w["icl_nearest_dev_k10"]["min"]), exact_tflops=3.0 * st["pairs"] * d / (m / 1e3) / 1e12)
    else:
        res["bulk"] = "not measured"
    ctx.close()
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
