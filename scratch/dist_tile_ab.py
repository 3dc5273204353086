"""Two builds of libimageclust_hip.so on the distance stage: are the results the same bytes, and do the kernels take the same time?

    python scratch/dist_tile_ab.py --parent /path/to/parent/libimageclust_hip.so --branch imageclust_amd/libimageclust_hip.so \
        --out profiles/r28_dist_tile_ab.json

Every library runs in a fresh child process (ICL_SO_PATH), and the order alternates parent, branch, parent, branch, parent, branch.

  outputs  one child per library on seeded inputs; SHA-256 of the bytes of icl_distance_mfma_dev's matrix, of the span of
           icl_ward_distance_rows_dev for tile rows 8 .. 33 of n = 4224 (flagged bounds: n >= 4096, tr_lo != 0) and for the same rows as exact
           values, of icl_ward_distance_matrix with and without sizes on the scalar and the 16-byte load path, of icl_nearest's indices and
           values, and icl_distance_bounds_check_dev's counts for both bound kernels (dist_bound_i8_kernel's listing is the same in both builds,
           so it is compared here and not timed).  The two libraries' digests must be equal.
  times    three children per library under `rocprofv3 --kernel-trace --stats` (nothing else traced, the program behind `--`), at n = 32 768,
           d = 2048 and, for icl_nearest_dev, 4 096 queries against 100 000 rows.  A run's figure for a kernel is the median duration of its
           launches after the first; a library's figure is the median of its three runs.  s = (max - min) / min of the PARENT's three runs;
           the branch passes for a kernel when its median <= the parent's median * (1 + s).

A child that fails ends the job: nothing further is started on the device.
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> how a trace may spell it (demangled, mangled)
KERNELS = {"ward_dist_exact_kernel<0>": ["ward_dist_exact_kernel<0>", "ward_dist_exact_kernelILi0E"],
           "ward_dist_exact_kernel<1>": ["ward_dist_exact_kernel<1>", "ward_dist_exact_kernelILi1E"],
           "nearest_tile_select_kernel": ["nearest_tile_select_kernel", "band_select_kernel<nr_policy>", "band_select_kernelI9nr_policy"],
           "dist_mfma_kernel<0>": ["dist_mfma_kernel<0>", "dist_mfma_kernelILi0E"],
           "dist_mfma_kernel<1>": ["dist_mfma_kernel<1>", "dist_mfma_kernelILi1E"],
           "dist_bound_kernel": ["dist_bound_kernel"]}


# ---- children ------------------------------------------------------------------------------------------------------------------
def _ctx():
    sys.path.insert(0, ROOT)
    from imageclust_amd import _lib
    return _lib, _lib.Context(0)


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def _rows_span(_lib, ctx, E, row_lo, row_hi):
    import ctypes as C
    import numpy as np
    n, d = E.shape
    off, cnt = C.c_int64(), C.c_int64()
    assert ctx.L.icl_ward_span(row_lo, row_hi, C.byref(off), C.byref(cnt)) == 0
    dE, dS = ctx.malloc(E.nbytes), ctx.malloc(cnt.value * 4)
    try:
        ctx.h2d(dE, E)
        ctx.h2d(dS, np.zeros(cnt.value, np.float32))  # (the rows' padding is never written)
        ctx.ward_distance_rows_dev(dE, n, d, row_lo, row_hi, dS)
        out = np.empty(cnt.value, np.float32)
        ctx.d2h(out, dS)
    finally:
        ctx.free(dE)
        ctx.free(dS)
    return out


def child_outputs():
    import numpy as np
    _lib, ctx = _ctx()
    rng = np.random.default_rng(20261019)
    res = {}
    E = rng.standard_normal((1153, 100), dtype=np.float32)
    res["distance_mfma n=1153 d=100"] = _sha(ctx.distance_mfma(E))
    E = rng.standard_normal((4224, 200), dtype=np.float32)
    res["rows_hold_bounds n=4224"] = int(ctx.L.icl_ward_rows_hold_bounds(ctx.h, 4224, 200))
    res["ward_distance_rows_dev n=4224 d=200 rows 1024..4224 (flagged bounds)"] = _sha(_rows_span(_lib, ctx, E, 1024, 4224))
    ctx.set_ward_options(1)
    res["ward_distance_rows_dev n=4224 d=200 rows 1024..4224 (exact)"] = _sha(_rows_span(_lib, ctx, E, 1024, 4224))
    ctx.set_ward_options(0)
    for n, d in ((1153, 6), (1153, 8), (300, 2048)):
        E = rng.standard_normal((n, d), dtype=np.float32)
        sizes = rng.integers(1, 60, n).astype(np.int32)
        res["ward_distance_matrix n=%d d=%d" % (n, d)] = _sha(ctx.ward_distance_matrix(E))
        res["ward_distance_matrix n=%d d=%d sizes" % (n, d)] = _sha(ctx.ward_distance_matrix(E, sizes))
    for nq, n, d in ((300, 5000, 2048), (301, 1153, 6)):
        Q, E = rng.standard_normal((nq, d), dtype=np.float32), rng.standard_normal((n, d), dtype=np.float32)
        qs, es = rng.integers(1, 30, nq).astype(np.int32), rng.integers(1, 30, n).astype(np.int32)
        idx, val = ctx.nearest(Q, E, 10, qs, es, 40, rng.integers(-1, n, nq))
        res["nearest nq=%d n=%d d=%d idx" % (nq, n, d)], res["nearest nq=%d n=%d d=%d val" % (nq, n, d)] = _sha(idx), _sha(val)
    E = rng.standard_normal((4224, 256), dtype=np.float32)
    for kind in (1, 2):
        res["distance_bounds_check n=4224 d=256 kind=%d" % kind] = ctx.distance_bounds_check(E, kind)
    ctx.close()
    print("AB_RESULT " + json.dumps(res))


def child_times(n, d, nq, lib_n, reps, lw_reps):
    import ctypes as C
    import numpy as np
    _lib, ctx = _ctx()
    X = np.random.default_rng(20261020).standard_normal((lib_n, d), dtype=np.float32)
    dX, dD = ctx.malloc(X.nbytes), ctx.malloc(n * n * 4)
    dI, dV = ctx.malloc(nq * 10 * 4), ctx.malloc(nq * 10 * 4)
    ctx.h2d(dX, X)
    del X
    for _ in range(reps):
        _lib.check(ctx.h, ctx.L.icl_ward_distance_matrix_dev(ctx.h, C.c_void_p(dX), None, n, d, C.c_void_p(dD), n))  # ward_dist_exact_kernel<1>
        ctx.sync()
        _lib.check(ctx.h, ctx.L.icl_distance_mfma_dev(ctx.h, C.c_void_p(dX), n, d, C.c_void_p(dD), n))  # dist_mfma_kernel<1>
        ctx.sync()
        ctx.ward_distance_rows_dev(dX, n, d, 0, n, dD)  # dist_bound_kernel (n >= 4096)
        ctx.set_ward_options(1)
        ctx.ward_distance_rows_dev(dX, n, d, 0, n, dD)  # ward_dist_exact_kernel<0>
        ctx.set_ward_options(0)
        ctx.nearest_dev(dX, nq, dX, lib_n, d, 10, dI, dV)  # band_select_kernel<nr_policy> (a parent build: nearest_tile_select_kernel)
        ctx.sync()
    for _ in range(lw_reps):
        ctx.cluster_dev(dX, n, d, 3, 6, _lib.UPDATE_LW)  # dist_mfma_kernel<0> (the packed matrix of the fast mode)
    for p in (dX, dD, dI, dV):
        ctx.free(p)
    ctx.close()
    print("AB_RESULT {}")


# ---- driver --------------------------------------------------------------------------------------------------------------------
def run_child(so, args, limit, prof_dir=None):
    env = dict(os.environ, ICL_SO_PATH=os.path.abspath(so))
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    if prof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "-d", prof_dir, "--output-format", "csv", "--"] + cmd
    print("running %s: %s" % (os.path.basename(os.path.dirname(os.path.abspath(so))) + "/" + os.path.basename(so), " ".join(args)), flush=True)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-3000:] + "\n" + r.stderr[-6000:] + "\n")
        sys.exit("child failed with status %d (%s): nothing further is started" % (r.returncode, " ".join(cmd)))
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("AB_RESULT ")][-1]
    return json.loads(line[len("AB_RESULT "):])


def kernel_medians(prof_dir):
    """{kernel: median duration in us of its launches after the first} from the run's kernel trace"""
    files = glob.glob(os.path.join(prof_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + prof_dir
    dur = {}
    for f in files:
        rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
        for r in rows:
            for k, names in KERNELS.items():
                if any(nm in r["Kernel_Name"] for nm in names):
                    dur.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for k, v in dur.items():
        v = sorted(v[1:] if len(v) > 1 else v)
        out[k] = dict(median_us=v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), launches_counted=len(v))
    return out


def med3(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["outputs", "times"])
    ap.add_argument("--parent")
    ap.add_argument("--branch")
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--lib-n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--lw-reps", type=int, default=3, help="fast-mode clustering calls per run (each launches dist_mfma_kernel<0> once)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.child == "outputs":
        return child_outputs()
    if a.child == "times":
        return child_times(a.n, a.d, a.nq, a.lib_n, a.reps, a.lw_reps)

    libs = [("parent", a.parent), ("branch", a.branch)]
    res = dict(device="MI355X (1 GCD)", order="parent, branch alternating; a fresh child process per library and run")
    outs = {tag: run_child(so, ["--child", "outputs"], a.limit) for tag, so in libs}
    res["outputs"] = {k: dict(parent=outs["parent"][k], branch=outs["branch"][k], equal=outs["parent"][k] == outs["branch"][k]) for k in outs["parent"]}
    res["outputs_all_equal"] = all(v["equal"] for v in res["outputs"].values())

    shape = ["--n", str(a.n), "--d", str(a.d), "--nq", str(a.nq), "--lib-n", str(a.lib_n), "--reps", str(a.reps), "--lw-reps", str(a.lw_reps)]
    runs = {tag: [] for tag, _ in libs}
    for _ in range(a.runs):
        for tag, so in libs:
            with tempfile.TemporaryDirectory(prefix="dist_tile_ab_") as pd:
                run_child(so, ["--child", "times"] + shape, a.limit, pd)
                runs[tag].append(kernel_medians(pd))
    times = {}
    for k in KERNELS:
        p = [r[k]["median_us"] for r in runs["parent"] if k in r]
        b = [r[k]["median_us"] for r in runs["branch"] if k in r]
        if len(p) != a.runs or len(b) != a.runs:
            times[k] = "not launched by this workload"
            continue
        s = (max(p) - min(p)) / min(p)
        times[k] = dict(parent_runs_us=p, branch_runs_us=b, parent_median_us=med3(p), branch_median_us=med3(b), s=s,
                        bound_us=med3(p) * (1 + s), within_bound=bool(med3(b) <= med3(p) * (1 + s)),
                        launches_counted_per_run=runs["parent"][0][k]["launches_counted"])
    res["times"] = dict(n=a.n, d=a.d, nearest_queries=a.nq, nearest_rows=a.lib_n, runs_per_library=a.runs, kernels=times)
    s = json.dumps(res, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
