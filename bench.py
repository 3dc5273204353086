#!/usr/bin/env python3
"""bench.py -- images/sec (embed + Ward) of the MI355X engine, BASELINE.json's metric.

A "step" is one pass of the hot path over one batch of synthetic input that is already resident in HBM:
    u8 images (per rank) -> ResNet50-v1 bf16 embed (batch 256) -> [N>1: RCCL all-gather of E over xGMI]
    -> size-constrained Ward (min=5, max=50, exact update: cluster ids bit-identical to the reference)
    -> cluster_id[N] on the host.
The workload is the one BASELINE.json's metric is quoted on: "images/sec (embed+Ward) on 100k 224x224 imgs at 1/2/4/8
MI355X" -- 100 000 synthetic images (configs[2]'s N; it fits one 288 GB GPU: 15 GB of images, 40 GB distance matrix).
N=1 runs the whole job on one GPU; N>1 STRONG-scales the same 100 000-image job: the images are sharded over the ranks
for the embed, E is all-gathered, every rank computes its share of the initial distance matrix and sends it to rank 0
over xGMI, rank 0 runs the exact merge loop (configs[2]'s shape: "Ward on GPU0").  `--total-images 10000` is
configs[1] (its line is quoted in README.md), `--total-images 250000` configs[4] (250 GB distance matrix on one GPU),
`--embed-only --total-images 1000000` configs[3]; `--scaling weak` keeps --images-per-gpu images PER GPU instead;
`--prec fp32` runs the parity embedding (f32 MFMA, <= 1e-4 of the fp32 restatement) instead of the bf16 one.

Launch:  python bench.py --gpus 1 --steps K --warmup W [--full] [--dump-outputs DIR]
         python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
                bench.py --gpus N --steps K --warmup W
Rank 0 prints ONE JSON line.  PyTorch is used for device buffers, barriers and the all-gather only.
A plain run sets up, warms up, times K steps and prints the headline figure.  --full adds what the headline does not need: the
untimed profiling passes behind the `roofline*` objects, the CPU baseline and the `parity` checks against oracle/.
--dump-outputs DIR writes what the last timed step returned (see dump_outputs) so that two builds can be compared.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# roofline denominators (/opt/skills/guides/MI355X_MICROARCH.md "Chip-level parameters")
PEAK_BF16_TFLOPS = 2500.0
PEAK_F32_TFLOPS = 157.3
PEAK_I8_TOPS = 5000.0  # dense int8: twice the bf16 rate (MI355X_MICROARCH.md, Matrix cores)
PEAK_HBM_GBS = 8000.0
FLOP_PER_IMAGE = 2 * 3857973248  # 53 conv + 1 fc, MACs x 2


def cpu_baseline(n_embed=64, ward_sizes=(64, 1000, 2000, 4000), d=2048, budget_s=75.0, ctx=None, ward_mode=0, own_E=None):
    """The CPU restatement of the reference algorithm (oracle/, kind "port"), timed on this box's host cores as SURVEY.md
    8d prescribes: (i) embed = the fp32 ResNet50 restatement, batch 1, serial calls, all cores inside a call (OpenCV-DNN is
    internally multi-threaded, embeddings.go:133-141), 64 images; (ii) Ward = the literal O(N^3) restatement, ONE thread
    (the reference clusters on one goroutine, workflow.go:89), at N in {64, 1000, 2000, 4000}, D=2048, (min,max) = (3,6)
    for N=64 (handlers.go:111) and (5,50) otherwise, with the fitted a*N^3 + b*N^2*D model.  Nothing is extrapolated to
    100k: `value` is the measured rate of the largest measured job (embed N images + cluster them).
    With ctx (the engine's context) the same inputs also go through the GPU path and the second return value is the `parity`
    object of the JSON line: the oracle is the checker here, never the thing measured.  own_E: rows of the embedding matrix THIS run has just
    produced (workflow.go:84-94 clusters what it embedded): clustered by the engine (both bound modes) and by oracle/ward_fast.c, outside the timed baseline."""
    from oracle import oracle as O
    from imageclust_amd import _lib

    # the oracle's OpenMP team: the CPUs this process may run on, capped at 16 (a 1-GPU box's CPU share)
    cores = min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 16)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    t_start = time.perf_counter()
    blob = _lib.synthetic_blob(1)
    imgs = _lib.synth_images(20250217, 0, n_embed, _lib.SYNTH_STRUCTURED)
    O.resnet50_forward(blob, imgs[0])  # warm
    t0 = time.perf_counter()
    done = 0
    for im in imgs:
        O.resnet50_forward(blob, im)  # batch 1, serial calls, OpenMP inside: as embeddings.go:133-141
        done += 1
        if time.perf_counter() - t0 > 0.55 * budget_s:
            break
    t_embed = time.perf_counter() - t0
    embed_rate = done / t_embed
    parity = None
    if ctx is not None:  # the parity path (fp32) on 4 of the images the oracle has just embedded, against the oracle's embeddings
        ref4 = np.stack([O.resnet50_forward(blob, imgs[i])[0] for i in range(4)])
        got4 = ctx.embed_u8(imgs[:4], _lib.HEAD_POOLED, _lib.PREC_FP32)
        parity = {"embed_fp32_max_rel_err": float("%.3g" % (np.abs(got4 - ref4).max() / max(1.0, float(np.abs(ref4).max())))),
                  "embed_fp32_tolerance": 1e-4, "embed_images_compared": 4}
    rng = np.random.default_rng(20250217)
    ward = []
    for n_ward in ward_sizes:
        if ward and time.perf_counter() - t_start + ward[-1][1] * (n_ward / ward[-1][0]) ** 3 > budget_s:
            break  # the next size would not fit the budget on this host: report what was measured
        cen = rng.standard_normal((max(n_ward // 20, 1), d)).astype(np.float32)
        E = (cen[rng.integers(0, len(cen), n_ward)] + 0.1 * rng.standard_normal((n_ward, d))).astype(np.float32)
        mn, mx = (3, 6) if n_ward == 64 else (5, 50)
        t0 = time.perf_counter()
        ref = O.cluster(E, mn, mx, want_log=True, threads=1)
        ward.append((n_ward, time.perf_counter() - t0))
        if ctx is not None:  # the same E through the engine: ids, member order and the merge sequence, bit for bit
            # forced onto the kernels the timed 100 000-image step runs (auto would use exact rows below n = 4096): matrix-core bounds in the
            # initial matrix and Lance-Williams lower bounds in the new clusters' rows, evaluated exactly on demand
            ctx.set_ward_options(4)
            try:
                cid, mr, nc = ctx.cluster(E, mn, mx)
            finally:
                ctx.set_ward_options(ward_mode)
            same = bool(nc == ref["n_clusters"] and np.array_equal(cid, ref["cluster_id"]) and np.array_equal(mr, ref["member_rank"])
                        and np.array_equal(ctx.last_merges(), ref["log"][:, 2:4].astype(np.int32)))
            parity["ward_ids_and_log_equal_n%d" % n_ward] = same
    if ctx is not None and own_E is not None and len(own_E) >= 64:
        # the benchmark's own data: the first rows of the E the timed steps produced (bf16 ResNet embeddings: non-negative, a large common mean, near-ties),
        # through the timed step's kernels (ICL_DIST_LWBOUND) and the exact-rows batched pipeline (ICL_DIST_BOUND), against the sub-cubic restatement
        fe = O.cluster_fast(np.ascontiguousarray(own_E), 5, 50, lazy_ban=False)
        want = fe["log"][:, 2:4].astype(np.int32)
        for mode, name in ((4, "lwbound"), (2, "bound")):
            ctx.set_ward_options(mode)
            try:
                cid, mr, nc = ctx.cluster(own_E, 5, 50)
            finally:
                ctx.set_ward_options(ward_mode)
            parity["ward_own_embeddings_n%d_%s_ids_log_values_equal" % (len(own_E), name)] = bool(
                fe["ok"] and nc == fe["n_clusters"] and np.array_equal(cid, fe["cluster_id"]) and np.array_equal(mr, fe["member_rank"])
                and np.array_equal(ctx.last_merges(), want) and np.array_equal(ctx.last_merge_values().view(np.uint32), fe["vals"].view(np.uint32)))
    # least squares for t = a*N^3 + b*N^2*D (the scan and the distance/row-refresh terms of SURVEY.md 3.3)
    A = np.array([[float(n) ** 3, float(n) ** 2 * d] for n, _ in ward])
    coef, *_ = np.linalg.lstsq(A, np.array([t for _, t in ward]), rcond=None)
    n_big, t_big = ward[-1]
    value = n_big / (n_big / embed_rate + t_big)
    base = {"value": round(value, 3), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": "oracle/ CPU restatement: embed %d images (batch 1, serial calls, OpenMP %d threads: %.2f img/s) + Ward D=%d on 1 "
                      "thread at N=%s (%s s); value = the measured N=%d job: %d/(%d/embed_rate + %.2f s); no size beyond "
                      "N=%d is measured or extrapolated" % (done, cores, embed_rate, d, [n for n, _ in ward],
                                                           ", ".join("%.2f" % t for _, t in ward), n_big, n_big, n_big, t_big, n_big),
            "embed_images_per_sec": round(embed_rate, 3), "embed_images": done,
            "ward_seconds": {str(n): round(t, 3) for n, t in ward},
            "ward_fit": {"model": "t = a*N^3 + b*N^2*D seconds", "a": float("%.4g" % coef[0]), "b": float("%.4g" % coef[1])},
            "seconds_total": round(time.perf_counter() - t_start, 1)}
    return base, parity


def layerwise_roofline_seconds(batch):
    """Sum over the launches of the ResNet50-v1 forward pass of max(flops / bf16 MFMA peak, HBM bytes / HBM peak) for one batch:
    the time the pass would take if every launch sat on its own roofline (activations bf16 NHWC, each tensor read and written once
    per launch, residual read once, downsample branch fused; since round 4 the stem + maxpool and each stage-1 bottleneck are ONE
    launch: image in / pooled tensor out, block input in / block output out).  Context for the per-kernel roofline fraction."""
    B = batch
    lay = [(2 * B * 112 * 112 * 64 * 147, B * 224 * 224 * 3 + B * 56 * 56 * 64 * 2)]
    h, cin = 56, 64
    for s, nb in enumerate([3, 4, 6, 3]):
        cout = 256 << s
        mid = cout // 4
        for bl in range(nb):
            ho = h // (2 if (bl == 0 and s > 0) else 1)
            if s == 0:  # the whole bottleneck in one launch
                lay.append((2 * B * ho * ho * (mid * cin + mid * mid * 9 + cout * (mid + (cin if bl == 0 else 0))), (B * h * h * cin + B * ho * ho * cout) * 2))
            else:
                lay.append((2 * B * ho * ho * mid * cin, (B * h * h * cin + B * ho * ho * mid) * 2))
                lay.append((2 * B * ho * ho * mid * mid * 9, B * ho * ho * mid * 2 * 2))
                if bl == 0:
                    lay.append((2 * B * ho * ho * cout * (mid + cin), (B * ho * ho * mid + B * h * h * cin + B * ho * ho * cout) * 2))
                else:
                    lay.append((2 * B * ho * ho * cout * mid, (B * ho * ho * mid + 2 * B * ho * ho * cout) * 2))
            cin, h = cout, ho
    lay.append((0, B * 49 * 2048 * 2))
    return sum(max(f / (PEAK_BF16_TFLOPS * 1e12), b / (PEAK_HBM_GBS * 1e9)) for f, b in lay)


DUMP_ROWS = 4096  # embedding rows --dump-outputs writes: 32 MiB at D = 2048, the bulk of its 64 MB


def dump_outputs(out_dir, E, cid=None, mrank=None, nc=None):
    """--dump-outputs: what the last timed step handed its caller, one DIR/<name>.npy per array.  E (n x 2048 fp32 on the device,
    800 MB at 100 000 images) is written as a fixed sample: DUMP_ROWS rows drawn with a fixed seed, their indices beside them.  The
    clustering outputs are written whole, in float64 so that every index is exact (16 bytes per image: 4 MB at configs[4]'s 250 000)."""
    import torch

    os.makedirs(out_dir, exist_ok=True)
    n = E.shape[0]
    rows = np.sort(np.random.default_rng(20250217).choice(n, size=min(n, DUMP_ROWS), replace=False))
    arrays = {"embedding_rows": rows.astype(np.float64),
              "embeddings_sample": E[torch.from_numpy(rows).to(E.device)].float().cpu().numpy()}
    if cid is not None:
        arrays.update(cluster_id=np.asarray(cid, np.float64), member_rank=np.asarray(mrank, np.float64), n_clusters=np.array([nc], np.float64))
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--total-images", type=int, default=100000, help="strong scaling: images of the whole job (100000 = the metric's size, 10000 = configs[1])")
    ap.add_argument("--images-per-gpu", type=int, default=10000, help="weak scaling: images per rank")
    ap.add_argument("--scaling", choices=["strong", "weak"], default="strong")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl (= RCCL over xGMI, the product path); gloo stages the gather through host memory and lets several "
                         "ranks share one GPU -- only for rehearsing the N>1 control flow on a 1-GPU box")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--min-size", type=int, default=5)
    ap.add_argument("--max-size", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline and the parity checks")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the untimed profiling passes (roofline objects), the CPU baseline and the parity "
                         "checks against oracle/; off by default: a plain run does only what the headline figure needs")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step returned as DIR/<name>.npy (float32 / float64, < 64 MB)")
    ap.add_argument("--embed-only", action="store_true", help="configs[3]: embed throughput without clustering")
    ap.add_argument("--overlap", action="store_true",
                    help="N=1: run the distance rows of already-embedded images on a side stream beside the later forward passes "
                         "(icl_embed_cluster_dev's ICL_FUSE_OVERLAP).  Off by default: measured at 100 000 images the two do not "
                         "co-execute productively (embed + distances 1 881 ms overlapped, 1 859 ms one after the other; DESIGN.md 5)")
    ap.add_argument("--prec", choices=["bf16", "fp32"], default="bf16",
                    help="bf16: bf16 MFMA with fp32 accumulate (BASELINE.json configs[1], the default); fp32: f32 MFMA, the parity "
                         "path whose embeddings meet 1e-4 against the fp32 restatement (157.3 TFLOP/s matrix peak)")
    ap.add_argument("--tiles", choices=["auto", "distributed", "local"], default="auto",
                    help="N > 1, exact mode: who builds the initial distance matrix.  distributed: every rank computes an area-balanced run of "
                         "rows -- flagged matrix-core lower bounds, the same f32 GEMM as the single-GPU path (0.15 s / N at 100 000 images) -- and sends "
                         "its span to rank 0 (point-to-point, 20 GB x (N-1)/N); local: rank 0 fills the whole matrix itself (0.15 s, nothing to "
                         "transport: since round 5 from the integer GEMM, 63 ms at 100 000 images -- as long as receiving the rows takes); auto = local")
    ap.add_argument("--ward-dist", choices=["auto", "exact", "bound", "lwbound"], default="auto",
                    help="exact mode only (include/imageclust.h ICL_DIST_*): how distances are produced -- every value on the vector ALUs, "
                         "or proven lower bounds from the matrix cores in the initial matrix with exact evaluation on demand (same ids, bit for "
                         "bit; UpdateDistanceMatrix's new rows are always exact values); auto: bounds for n >= 4096")
    ap.add_argument("--update", choices=["exact", "lw"], default="exact",
                    help="exact: centroid recompute, cluster ids bit-identical to the reference (default); "
                         "lw: MFMA distance tile + Lance-Williams rows (fast, not bit-identical)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (ms_per_step is the time of one timed step)")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d; launch with torch.distributed.run" % (args.gpus, world), file=sys.stderr)
        if world == 1 and args.gpus > 1:
            sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py needs a GPU (no CPU fallback)", file=sys.stderr)
        sys.exit(2)
    if args.dist_backend == "gloo":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        from imageclust_amd import distributed as D0

        D0.init(args.dist_backend, rank, world, dev)  # nccl == RCCL on ROCm (xGMI inside the node)

    from imageclust_amd import _lib
    from imageclust_amd import distributed as D

    ctx = _lib.Context(local_rank)
    ctx.set_ward_options({"auto": 0, "exact": 1, "bound": 2, "lwbound": 4}[args.ward_dist])
    ctx.load_synthetic(1)
    ctx.set_batch(args.batch)
    if args.scaling == "weak":
        n_total = args.images_per_gpu * world
    else:
        n_total = args.total_images
    lo, hi = D.shard_range(n_total, rank, world)
    n_local = hi - lo
    DIM = _lib.HEAD_POOLED

    # synthetic inputs, generated on-device and resident in HBM before any timed region
    imgs = torch.empty(max(n_local, 1) * _lib.IMG_BYTES, dtype=torch.uint8, device=dev)
    ctx.synth_images_dev(20250217, lo, n_local, _lib.SYNTH_STRUCTURED, imgs.data_ptr())
    ctx.sync()
    E_local = torch.empty((max(n_local, 1), DIM), dtype=torch.float32, device=dev)[:n_local]
    update = _lib.UPDATE_LW if args.update == "lw" else _lib.UPDATE_EXACT
    PREC = _lib.PREC_FP32 if args.prec == "fp32" else _lib.PREC_BF16
    peak_mfma = PEAK_F32_TFLOPS if args.prec == "fp32" else PEAK_BF16_TFLOPS
    result = {}
    keep = {}

    def step():
        if world == 1 and not args.embed_only:
            # one GPU: workflow.go:84-94 as ONE call of the engine (embed -> distance rows -> merge loop, stages overlapped inside the context)
            keep["E_full"] = E_local
            cid, mrank, nc = ctx.embed_cluster_dev(imgs.data_ptr(), n_local, E_local.data_ptr(), args.min_size, args.max_size, PREC, update,
                                                   overlap=args.overlap)
            keep.update(cid=cid, mrank=mrank, nc=nc)
            st = ctx.last_stage_ms()
            result.update(embed_ms=st["embed_ms"], dist_ms=st["dist_ms"], merge_ms=st["merge_ms"], n_clusters=nc, merges=len(ctx.last_merges()),
                          dropped=int((cid < 0).sum()))
            return
        ctx.embed_u8_dev(imgs.data_ptr(), n_local, E_local.data_ptr(), DIM, PREC)  # returns with the stream idle
        st = ctx.last_stage_ms()
        result["embed_ms"] = st["embed_ms"]
        E_full = E_local
        if world > 1:
            t0 = time.perf_counter()
            if args.dist_backend == "nccl":
                E_full = D.gather_embeddings(E_local, n_total, rank, world)  # ONE RCCL all-gather, shard order
            else:
                E_full = D.gather_embeddings(E_local.cpu(), n_total, rank, world).to(dev)
            torch.cuda.synchronize()
            result["allgather_ms"] = (time.perf_counter() - t0) * 1e3
        if args.embed_only:
            keep["E_full"] = E_full
            return
        if world > 1 and args.update == "exact" and (args.tiles == "distributed"):
            # the initial distance matrix is built on ALL ranks (area-balanced runs of tile rows), every span goes to rank 0's
            # triangle over xGMI (point-to-point sends, no collective), rank 0 runs the exact merge loop
            t0 = time.perf_counter()
            res = D.cluster_with_distributed_tiles(ctx, E_full, args.min_size, args.max_size, rank, world, update,
                                                   staged=(args.dist_backend == "gloo"))
            if rank == 0:
                keep["E_full"] = E_full
                cid, mrank, nc = res
                keep.update(cid=cid, mrank=mrank, nc=nc)
                st = ctx.last_stage_ms()
                total_ms = (time.perf_counter() - t0) * 1e3
                result.update(dist_ms=total_ms - st["merge_ms"], merge_ms=st["merge_ms"], n_clusters=nc, merges=len(ctx.last_merges()),
                              dropped=int((cid < 0).sum()))
        elif rank == 0:
            keep["E_full"] = E_full  # rank 0 re-uses the gathered matrix for the untimed profiling pass (no second collective)
            cid, mrank, nc = ctx.cluster_dev(E_full.data_ptr(), n_total, DIM, args.min_size, args.max_size, update)
            keep.update(cid=cid, mrank=mrank, nc=nc)
            st = ctx.last_stage_ms()
            result.update(dist_ms=st["dist_ms"], merge_ms=st["merge_ms"], n_clusters=nc, merges=len(ctx.last_merges()),
                          dropped=int((cid < 0).sum()))

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    elapsed = D.max_over_ranks(elapsed, dev if args.dist_backend == "nccl" else None)
    if rank == 0 and args.dump_outputs:  # before anything below writes into E_local again
        dump_outputs(args.dump_outputs, keep["E_full"], keep.get("cid"), keep.get("mrank"), keep.get("nc"))
    # The timed steps keep two forward passes in flight on two streams, where single launches cannot be bracketed with
    # events.  One extra, UNTIMED embedding pass over the same images runs the identical kernels on one stream with a HIP
    # event pair around every conv launch (on the engine's own stream) for the roofline object.
    if rank == 0 and args.full:
        conv_mask = (1 << _lib.K_CONV) | (1 << _lib.K_CONV64)
        ctx.prof_reset()
        ctx.prof_enable(conv_mask)
        embed_ms_keep = result.get("embed_ms")
        # at most 102 400 images (400 batches, 21 200 bracketed launches): per-launch averages do not need more, and the event
        # pairs of a pass stay allocated until it ends (configs[3] embeds 1 000 000 images)
        n_prof = min(n_local, 102400)
        ctx.embed_u8_dev(imgs.data_ptr(), n_prof, E_local.data_ptr(), DIM, PREC)
        result["embed_ms_single_stream"] = ctx.last_stage_ms()["embed_ms"] * (n_local / max(n_prof, 1))
        if embed_ms_keep is not None:
            result["embed_ms"] = embed_ms_keep
        ctx.prof_enable(0)

    upd = dist_prof = rowmin_prof = None
    c128 = c64 = None
    if rank == 0 and args.full:
        c128, c64 = ctx.prof_query(_lib.K_CONV), ctx.prof_query(_lib.K_CONV64)
    if rank == 0 and args.full and not args.embed_only and args.update == "exact":
        # The timed steps replay the merge loop from a hipGraph, where single launches cannot be bracketed with events.
        # One extra, UNTIMED clustering pass over the same E runs the identical kernels eagerly with a HIP event pair around
        # every ward_update_exact_kernel launch (on the engine's stream) to get that kernel's average duration.
        # NOTE: only rank 0 runs this block, so it must not call a collective: it re-uses the matrix gathered in the last step
        E_prof = keep.get("E_full")
        if E_prof is not None:
            ctx.prof_reset()
            ctx.prof_enable((1 << _lib.K_UPDATE) | (1 << _lib.K_DIST_MFMA) | (1 << _lib.K_ROWMIN))
            ctx.cluster_dev(E_prof.data_ptr(), n_total, DIM, args.min_size, args.max_size, update)
            ctx.prof_enable(0)
            upd = ctx.prof_query(_lib.K_UPDATE)
            dist_prof, rowmin_prof = ctx.prof_query(_lib.K_DIST_MFMA), ctx.prof_query(_lib.K_ROWMIN)
    if rank == 0:
        ms_per_step = elapsed / max(args.steps, 1) * 1e3
        value = n_total * args.steps / elapsed
        name, ncu, hbm = ctx.device_info()
        out = {
            "metric": "images/sec (embed+Ward)" if not args.embed_only else "images/sec (embed only)",
            "value": round(value, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "bf16" if args.prec == "bf16" else "f32", "data": "synthetic",
            "config": {"workload": (("%s: %d synthetic 224x224x3 images (structured, seed 20250217; %d on this rank), ResNet50-v1 " + args.prec +
                                     " batch=%d -> 2048-d pooled E%s")
                                    % ("configs[3] (embed only)" if args.embed_only and n_total == 1000000
                                       else "embed only, custom size" if args.embed_only
                                       else "the metric's size (configs[2]'s N=100000) on %d GPU%s" % (world, "s" if world > 1 else "") if n_total == 100000
                                       else "configs[4] (250 GB distance matrix on GPU0)" if n_total == 250000
                                       else "configs[1]" if n_total == 10000 and world == 1 else "custom size",
                                       n_total, n_local, args.batch,
                                       "" if args.embed_only else ((" -> RCCL all-gather of E -> distance rows (matrix-core lower bounds) on all ranks, sent to rank 0 piecewise (point-to-point) and laid into its matrix"
                                                                     if args.update == "exact" and (args.tiles == "distributed")
                                                                     else " -> RCCL all-gather of E -> rank 0 builds the whole distance matrix itself (matrix-core bounds)") if world > 1 else "")))
                                   + ("" if args.embed_only else " -> Ward min=%d max=%d (merge loop on GPU0) -> cluster ids on host" % (args.min_size, args.max_size)),
                       "n_images_total": n_total, "embed_dim": DIM, "weights": "synthetic seed 1", "device": name,
                       "ward_update": "none (embed only)" if args.embed_only else "exact (ids bit-identical to the reference; new clusters' rows: Lance-Williams lower bounds, evaluated exactly on demand)" if (args.update == "exact" and (args.ward_dist == "lwbound" or (args.ward_dist == "auto" and n_total >= 4096))) else "exact (ids bit-identical to the reference)" if args.update == "exact"
                       else "lw (MFMA distance tile + Lance-Williams, not bit-identical)"},
            "stages_ms_last_step": {k: round(v, 3) for k, v in result.items() if k.endswith("_ms")},
            "stages_note": ("N=1: embed_ms includes the distance rows that ran beside the forward passes on a side stream; dist_ms is what was left "
                            "(tables, centroid transpose, initial row minima)" if world == 1 and not args.embed_only and args.overlap else ""),
            "ward": {k: v for k, v in result.items() if not k.endswith("_ms")},
        }
    if rank == 0 and args.full:
        # conv_igemm_kernel<BF16,128> (all Cout>=128 convolutions)
        avg_us = c128["ms"] * 1e3 / max(c128["launches"], 1)
        achieved = c128["flops"] / max(c128["ms"], 1e-9) / 1e9  # TFLOP/s
        # HBM traffic of the same kernels from the PMC counters (FETCH_SIZE doubled per MI355X_MICROARCH.md + WRITE_SIZE, two
        # separate `rocprofv3 --kernel-trace --pmc ... -- python3 bench.py --steps 1 --warmup 0 --no-cpu-baseline` passes:
        # scratch/collect_profiles.sh).  The counters cannot be read while this run is being timed, so the per-launch means are
        # committed under profiles/ and quoted here.
        traffic = traffic_upd = pmc_file = None
        traffic_note = ""
        # the PMC means were taken at the default workload (100 000 images, bf16): quoted for that workload only
        for cand in ("r05_pmc_traffic.json", "r04_pmc_traffic.json"):  # scratch/collect_profiles.sh (rocprofv3 --pmc passes of THIS script)
            if n_total != 100000 or args.prec != "bf16":
                break
            try:
                with open(os.path.join(ROOT, "profiles", cand)) as f:
                    pmc = json.load(f)
                convs = [v for k, v in pmc.items() if k.startswith("conv_igemm_kernel<BF16, 128") or k.startswith("conv3x3_halo_kernel<BF16, 128") or k.startswith("bneck56_kernel") or k.startswith("conv_p8_kernel") or k.startswith("conv_wr_kernel")]
                traffic = round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in convs) / max(sum(v["launches"] for v in convs), 1), 0)
                upd_pmc = [v for k, v in pmc.items() if k.startswith("ward_update_lb_kernel") or k.startswith("ward_update_batch2_kernel")]  # (whichever the profiled run used)
                traffic_upd = round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in upd_pmc) / max(sum(v["launches"] for v in upd_pmc), 1), 0)
                traffic_note = "(means over every launch of one bench.py run at N=100000; the ward figure includes the spare / preselection workgroups' row reads)"
                pmc_file = cand
                break
            except Exception:
                continue
        p8_l, other_l = ctx.conv_stats()
        mfma_busy = None  # MFMA utilisation of the same kernel group from SQ counters (a separate rocprofv3 --pmc run: scratch/r5_mfma_counters.sh), quoted like `traffic`
        try:
            with open(os.path.join(ROOT, "profiles", "r05_mfma_counters.json")) as f:
                mfma_busy = round(float(json.load(f)["conv_group_mfma_busy_frac"]), 4) if args.prec == "bf16" else None
        except Exception:
            pass
        conv_roof = {"bound": "mfma", "kernel": ("conv kernels with Cout >= 128 (conv_p8_kernel: the deep-pipelined 256x256x64 / 512x128x64 loop, conv_wr_kernel: the streaming c3 layers, "
                                                 "bneck56_kernel: the fused stage-1 bottlenecks, conv_igemm_kernel<BF16,128> for what is left)" if args.prec == "bf16" else
                                                 "conv kernels with Cout >= 128 (conv_igemm_kernel<F32,128>, conv3x3_halo_kernel<F32,128>)"),
                     "launches_on_p8_or_wr_since_start": p8_l, "launches_on_other_conv_kernels_since_start": other_l,
                     "mfma_busy_frac": mfma_busy,  # SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x kernel cycles), profiles/r05_mfma_counters.json (null: not collected for this precision)
                     "achieved": round(achieved, 2),
                     "peak": peak_mfma, "unit": "TFLOP/s", "frac": round(achieved / peak_mfma, 4), "traffic": traffic,
                     "launches": c128["launches"], "avg_launch_us": round(avg_us, 2),
                     "algorithmic_flops_per_launch": round(c128["flops"] / max(c128["launches"], 1), 0),
                     "all_conv_achieved": round((c128["flops"] + c64["flops"]) / max(c128["ms"] + c64["ms"], 1e-9) / 1e9, 2),
                     "embed_frac_of_mfma_peak": round(n_local * FLOP_PER_IMAGE / max(result.get("embed_ms", 0), 1e-9) / 1e9 / peak_mfma, 4),
                     "embed_frac_of_layerwise_roofline": (round(layerwise_roofline_seconds(args.batch) * 1e3 * n_local / args.batch
                                                                / max(result.get("embed_ms", 0), 1e-9), 4) if args.prec == "bf16" else None),
                     "measured": "HIP events around every launch in one extra untimed single-stream pass over the same images (the timed steps keep two forward passes in flight on two streams)"}
        ward_roof = None
        if upd and upd["launches"]:
            ws = ctx.last_ward_stats()
            gbs = upd["bytes"] / max(upd["ms"], 1e-9) / 1e6  # GB/s
            # rows of new clusters: Lance-Williams lower bounds evaluated on demand (auto from n = 4096, D % 4 == 0) or 3 D exact operations per entry
            row_mode, init_bounds = ctx.last_ward_mode()  # what the profiled loop actually ran (the options are requests: ADVICE r04)
            lb_rows = row_mode == _lib.ROWS_LW_BOUND
            exact = row_mode in (_lib.ROWS_EXACT_BATCH, _lib.ROWS_SINGLE)
            tfl = upd["flops"] / max(upd["ms"], 1e-9) / 1e9  # 3 flop per (pair, k): sub, mul, add -- unfused by construction
            # What binds the exact update is the vector ALU (16 rows x 3 unfused fp32 ops per byte-quad: 12 flop/B), not HBM:
            # `bound` says so, achieved / peak / frac are the vector-fp32 figures, the HBM view sits beside them in `hbm`.
            # (The Lance-Williams update of --update lw reads 12 bytes per pair: that one IS an HBM kernel.)
            ward_roof = {"bound": "valu" if exact else "hbm", "kernel": {_lib.ROWS_SINGLE: "ward_update_exact_kernel", _lib.ROWS_EXACT_BATCH: "ward_update_batch2_kernel", _lib.ROWS_LW_BOUND: "ward_update_lb_kernel", _lib.ROWS_LW_FAST: "ward_update_batch_lw_kernel"}[row_mode],
                         "row_mode": row_mode, "initial_matrix_bounds": init_bounds,
                         "achieved": round(tfl, 2) if exact else round(gbs, 1), "peak": PEAK_F32_TFLOPS if exact else PEAK_HBM_GBS,
                         "unit": "TFLOP/s" if exact else "GB/s",
                         "frac": round(tfl / PEAK_F32_TFLOPS, 4) if exact else round(gbs / PEAK_HBM_GBS, 4), "traffic": traffic_upd if (exact or lb_rows) else None,
                         "hbm": {"achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4)},
                         "traffic_note": ("PMC FETCH_SIZE x2 + WRITE_SIZE per launch, profiles/%s %s" % (pmc_file, traffic_note)) if pmc_file else
                                         "PMC passes were taken at the default workload (100 000 images, bf16) only",
                         "launches": upd["launches"],
                         "avg_launch_us": round(upd["ms"] * 1e3 / upd["launches"], 2),
                         "algorithmic_bytes_per_launch": round(upd["bytes"] / upd["launches"], 0),
                         "merges_per_working_launch": round(ws["merges"] / max(ws["steps"], 1), 2),
                         "algorithmic_unit": "4*n_live*D bytes (one pass over the live centroids) + 4*n_live per new row, per LAUNCH; a launch "
                                             "computes the rows of up to 16 independent merges from that one pass (SURVEY.md 8d quotes "
                                             "4*n_live*D per merge: 16x these bytes)",
                         "valu": {"nominal_unfused_ceiling": 78.6, "measured_unfused_ceiling": 61.0, "frac_of_measured_ceiling": round(tfl / 61.0, 4),
                                  "note": "the exact update is 3 UNFUSED fp32 ops per (new row, live cluster, k) -- the reference's rounding "
                                          "forbids FMA -- so half of the FMA-counted vector peak (78.6 TFLOP/s) is its nominal ceiling; measured "
                                          "(scratch/pk_rate_bench.hip) v_pk_add_f32 / v_pk_mul_f32 issue every 5.2-5.7 cycles against 3.2 for "
                                          "the scalar ops, i.e. unfused packed fp32 tops out at ~61 TFLOP/s on this part (ward_dist_exact_kernel "
                                          "runs at that rate); with 16 rows per pass the kernel is bound by vector-ALU issue, not by HBM"},
                         "note": "one workgroup per 64 live clusters streams their centroids once (LDS-DMA ring) and runs 16 in-order sums; "
                                 "SURVEY.md 8d classifies the merge loop as HBM-bound, but with 16 rows per pass over the centroids the kernel "
                                 "is bound by vector-ALU issue: `frac` is the vector-fp32 fraction (FMA-counted peak), `hbm` the HBM view; "
                                 "launches after the last merge of a 64-step chunk are empty",
                         "total_ms_in_profile_pass": round(upd["ms"], 1),
                         "measured": "HIP events around every launch in one extra untimed eager pass over the same E "
                                     "(the timed steps replay a hipGraph)"}
            if lb_rows:  # the exact-update fields do not describe this kernel
                ward_roof.pop("valu", None)
                complete_rows, row_pitch, _i8 = ctx.last_ward_layout()
                ward_roof["matrix_layout"] = {"complete_rows": complete_rows, "row_pitch_floats": row_pitch,
                                              "bytes": 4 * row_pitch * (n_total + 32)}
                ward_roof["algorithmic_unit"] = ("12 bytes per (new row, live cluster): two stored entries read, one lower bound written -- the Lance-Williams "
                                                 "recurrence on the distance matrix instead of 3*D operations on the centroids (SURVEY.md 8d's 4*n*D per merge no longer "
                                                 "moves); the bytes of the row re-scans that ride in the same launch (8 bytes x N columns each, ~50 per launch) are not counted; `traffic` "
                                                 "(PMC) is ~17x the algorithmic bytes: one of the two read directions walks a COLUMN of the 40 GB matrix, 4 useful bytes per 64-byte line")
                if complete_rows:
                    ward_roof["algorithmic_unit"] = ("16 bytes per (new row, live cluster): two stored entries read -- both from CONTIGUOUS rows: the matrix keeps one column per "
                                                     "creation id and every row complete (8 n^2 bytes; icl_last_ward_layout) -- and the lower bound written twice, to the new row and, "
                                                     "transposed through LDS, to the live cluster's row; the row re-scans that ride in the same launch (8 bytes x row length each, ~70 per "
                                                     "launch) are not counted and are what `traffic` (PMC) mostly is")
                ward_roof["note"] = ("the launch is bound by LATENCY, not by HBM or the vector ALUs: its length is the chain phase A (row-cache slices) -> flag barrier "
                                     "-> one or two row re-scans + one exact evaluation (a chain of D dependent fp32 additions) per spare workgroup -> preselection; "
                                     "`frac` of the HBM peak is therefore small by construction (DESIGN.md section 3, per-step timeline)")
        conv_roof["total_ms_in_profile_pass"] = round(c128["ms"], 1)
        # `roofline` = the dominant kernel of THIS workload by GPU time in the profiling passes (at N=100 000 the batched Ward
        # update, vector-ALU bound; at configs[1]'s N=10 000 the Cout >= 128 convolutions, MFMA bound); the other one sits beside it
        # (the conv time of the single-stream profiling pass is scaled to the timed region, where two forward passes overlap)
        conv_ms_timed = c128["ms"] * result.get("embed_ms", 0.0) / max(result.get("embed_ms_single_stream", 0.0), 1e-9)
        ward_dominates = ward_roof is not None and upd["ms"] > conv_ms_timed
        roof = ward_roof if ward_dominates else conv_roof
        out["roofline"] = roof
        out["roofline_conv" if ward_dominates else "roofline_ward_update"] = conv_roof if ward_dominates else ward_roof
        if dist_prof and dist_prof["launches"]:
            # ComputeInitialDistanceMatrix as matrix-core lower bounds: one launch per clustering call
            i8 = ctx.last_ward_layout()[2]
            rate = dist_prof["flops"] / max(dist_prof["ms"], 1e-9) / 1e9  # T(FL)OP/s of the GEMM form
            peak = PEAK_I8_TOPS if i8 else PEAK_F32_TFLOPS
            out["roofline_distance"] = {
                "bound": "mfma", "kernel": "dist_bound_i8_kernel (v_mfma_i32_16x16x64_i8 on a 3 x 7-bit fixed-point image of the centred rows: 6 digit products per pair, exact)"
                if i8 else "dist_bound_kernel (v_mfma_f32_32x32x2_f32)",
                "achieved": round(rate, 1), "peak": peak, "unit": "TOP/s" if i8 else "TFLOP/s", "frac": round(rate / peak, 4),
                "launches": dist_prof["launches"], "avg_launch_us": round(dist_prof["ms"] * 1e3 / dist_prof["launches"], 1),
                "algorithmic_ops_per_launch": round(dist_prof["flops"] / dist_prof["launches"], 0),
                "algorithmic_unit": ("2 x 6 x 2048 int8 multiply-adds per pair of images (n (n - 1) / 2 pairs): the three digit classes of the 21-bit fixed-point dot product "
                                     "the bound needs" if i8 else "2 x D fp32 multiply-adds per pair of images (n (n - 1) / 2 pairs)"),
                "initial_row_minima_ms": round(rowmin_prof["ms"], 2) if rowmin_prof and rowmin_prof["launches"] else None,
                "measured": "HIP events around the launch in the extra untimed clustering pass (with the ward-update brackets)"}
        if not args.no_cpu_baseline and world == 1:
            own = None
            if not args.embed_only and args.prec == "bf16" and keep.get("E_full") is not None:
                own = keep["E_full"][:min(4000, n_total)].cpu().numpy()  # rows of the E the last timed step produced (copied before the fp32 pass below)
            out["cpu_baseline"], par = cpu_baseline(ctx=ctx, ward_mode={"auto": 0, "exact": 1, "bound": 2, "lwbound": 4}[args.ward_dist], own_E=own)
            # the throughput of the parity precision itself: one untimed 10 000-image pass of the fp32 (f32 MFMA) forward
            n10 = min(n_local, 10000)
            ctx.embed_u8_dev(imgs.data_ptr(), n10, E_local.data_ptr(), DIM, _lib.PREC_FP32)
            par["embed_fp32_img_per_s_10k"] = round(n10 / max(ctx.last_stage_ms()["embed_ms"], 1e-9) * 1e3, 1)
            par["note"] = ("checked in this run against oracle/ (CPU restatement of clustering.go / the ONNX graph): cluster ids, member order and the merge "
                           "sequence of the exact Ward path on the cpu_baseline inputs, forced onto the kernels of the timed step (ICL_DIST_LWBOUND: bounds in the "
                           "initial matrix and in the new clusters' rows, exact evaluation on demand); the first 4 000 rows of the E this run's timed steps produced "
                           "(bf16 ResNet embeddings) through both bound modes against oracle/ward_fast.c incl. every merge value; the fp32 embedding path on 4 images "
                           "(tolerance 1e-4 of the output scale).  The timed steps above run the bf16 embedding (configs[1]) and the same exact Ward path.")
            out["parity"] = par
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    ctx.close()


if __name__ == "__main__":
    main()
