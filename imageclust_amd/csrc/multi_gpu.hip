// multi_gpu.hip -- several MI355X behind ONE handle of the C-ABI ("icl_create(const int* devs, int ndev, ...)",
// 8e rows 1-2).  A Go service is one process: internal/workflow calls GetImageEmbedding / PerformClusteringWithConstraints
// (workflow.go:161,89) and cannot start one process per GPU, so the group drives N contexts from N host threads:
//   * embed: images shard by contiguous index ranges (no exchange: every GPU holds the weights);
//   * cluster: every GPU holds E (uploaded once to GPU 0 and passed on by peer copies, or -- icl_group_embed_cluster --
//     assembled on the GPUs from the embedding shards without touching the host).  Below 6 GPUs GPU 0 fills the whole initial
//     distance matrix itself from matrix-core bounds (faster than waiting for exact rows over one xGMI link per peer); from 6 GPUs
//     on GPU 0 computes the first area-balanced run of 128-row tile rows (icl_ward_rows_partition) and every other GPU the exact
//     values of its run into a buffer of its OWN memory, which GPU 0 reads over xGMI straight into its matrix rows
//     (icl_ward_unpack_spans_dev on peer-mapped memory; bounded copies where the devices are no peers).  GPU 0 holds the 4 n^2-byte
//     matrix and O(n d) beside it for any number of parts.  Results are bit-identical to one GPU: values decide every
//     comparison, wherever they were computed.
// Entries of `devices` may repeat (a test on a 1-GPU box builds a group of two contexts on device 0: the same code path,
// the peer copy degenerates to a device-to-device copy).
// The process-per-GPU path of bench.py uses the same building blocks (icl_ward_distance_rows_dev / icl_ward_unpack_spans_dev /
// icl_cluster_prefilled_dev) with RCCL send/recv as the transport.
#include "icl_common.h"
#include "distance.h" // icl_dist_i8_usable

#include <cstring>
#include <new>
#include <thread>

struct icl_group {
    std::vector<icl_ctx *> ctx;
    std::vector<char> peer0; // GPU 0 can read context i's device memory directly (same device, or peer access enabled)
    int tiles_mode = ICL_TILES_AUTO;
    int merge_mode = ICL_MERGE_GPU0;
    std::string err;
    std::mutex mu;
};
#define ICL_GROUP_DIST_MIN 4 /* GPUs from which the distance rows are dealt out by default (flagged bound rows, 0.15 s / G + 20 GB (G - 1) / G over one link per sender vs 0.15 s local) */

#define ICL_GROUP_MAX 64 /* contexts of a group (icl_group_create checks) */
static int group_fail(icl_group *g, int code, const std::string &msg)
{
    if (g) {
        std::lock_guard<std::mutex> lk(g->mu);
        g->err = msg;
    }
    return code;
}
// the group's entry points build strings, vectors and threads: nothing of that may throw across the C ABI
template <typename F>
static int group_no_throw(icl_group *g, const char *what, F &&body)
{
    try {
        return body();
    } catch (...) {
        if (g) {
            std::lock_guard<std::mutex> lk(g->mu);
            g->err.clear(); // (no allocation)
        }
        icl_fail(nullptr, ICL_ERR_NOMEM, "%s: out of host memory", what);
        return ICL_ERR_NOMEM;
    }
}

extern "C" int icl_group_create(const int32_t *devices, int32_t ndev, icl_group **out)
{
    if (!devices || ndev < 1 || ndev > ICL_GROUP_MAX || !out) return icl_fail(nullptr, ICL_ERR_ARG, "icl_group_create: bad argument");
    icl_group *g = new (std::nothrow) icl_group();
    if (!g) return icl_fail(nullptr, ICL_ERR_NOMEM, "icl_group_create: out of memory");
    for (int i = 0; i < ndev; ++i) {
        icl_ctx *c = nullptr;
        const int rc = icl_create(devices[i], &c);
        if (rc != ICL_OK) {
            for (icl_ctx *p : g->ctx) icl_destroy(p);
            delete g;
            return rc; // icl_create left its message in the thread-local error string
        }
        try {
            g->ctx.push_back(c);
        } catch (...) {
            icl_destroy(c);
            for (icl_ctx *p : g->ctx) icl_destroy(p);
            delete g;
            return icl_fail(nullptr, ICL_ERR_NOMEM, "icl_group_create: out of memory");
        }
    }
    // peer access between distinct devices (xGMI inside a node); failure is not fatal: copies then stage through the host
    try {
        g->peer0.assign((size_t)ndev, 0);
    } catch (...) {
        for (icl_ctx *p : g->ctx) icl_destroy(p);
        delete g;
        return icl_fail(nullptr, ICL_ERR_NOMEM, "icl_group_create: out of memory");
    }
    for (int i = 0; i < ndev; ++i)
        for (int j = 0; j < ndev; ++j) {
            bool ok = devices[i] == devices[j];
            if (!ok) {
                icl_device_guard dg(devices[i]);
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devices[i], devices[j]) == hipSuccess && can) {
                    const hipError_t e = hipDeviceEnablePeerAccess(devices[j], 0);
                    ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
                }
                (void)hipGetLastError(); // "already enabled" is fine
            }
            if (i == 0) g->peer0[(size_t)j] = ok ? 1 : 0;
        }
    *out = g;
    return ICL_OK;
}

extern "C" void icl_group_destroy(icl_group *g)
{
    if (!g) return;
    for (icl_ctx *c : g->ctx) icl_destroy(c);
    delete g;
}

extern "C" int icl_group_set_options(icl_group *g, int tiles_mode, int merge_mode)
{
    if (!g || tiles_mode < ICL_TILES_AUTO || tiles_mode > ICL_TILES_DISTRIBUTED || merge_mode < ICL_MERGE_GPU0 || merge_mode > ICL_MERGE_SHARDED)
        return group_fail(g, ICL_ERR_ARG, "icl_group_set_options: bad argument");
    if (merge_mode == ICL_MERGE_SHARDED && (int)g->ctx.size() > ICL_SHARD_MAX) return group_fail(g, ICL_ERR_UNSUPPORTED, "the sharded merge loop takes at most 16 GPUs");
    std::lock_guard<std::mutex> lk(g->mu);
    g->tiles_mode = tiles_mode;
    g->merge_mode = merge_mode;
    return ICL_OK;
}
extern "C" int32_t icl_group_size(icl_group *g) { return g ? (int32_t)g->ctx.size() : 0; }
extern "C" icl_ctx *icl_group_ctx(icl_group *g, int32_t i) { return (g && i >= 0 && i < (int32_t)g->ctx.size()) ? g->ctx[(size_t)i] : nullptr; }
extern "C" const char *icl_group_last_error(icl_group *g) { return g ? g->err.c_str() : ""; }

// run f(i, ctx_i) on one host thread per context; first failure wins
template <typename F>
static int for_each_ctx(icl_group *g, F &&f)
{
    const int n = (int)g->ctx.size();
    int rc[ICL_GROUP_MAX];
    for (int i = 0; i < n; ++i) rc[i] = ICL_OK;
    std::vector<std::thread> th;
    try {
        for (int i = 1; i < n; ++i) th.emplace_back([&, i] { rc[i] = f(i, g->ctx[(size_t)i]); });
    } catch (...) {
        for (auto &t : th) t.join();
        return group_fail(g, ICL_ERR_NOMEM, "could not start a host thread per GPU");
    }
    rc[0] = f(0, g->ctx[0]);
    for (auto &t : th) t.join();
    for (int i = 0; i < n; ++i)
        if (rc[i] != ICL_OK) return group_fail(g, rc[i], std::string("GPU ") + std::to_string(i) + ": " + icl_last_error(g->ctx[(size_t)i]));
    return ICL_OK;
}

extern "C" int icl_group_load_synthetic(icl_group *g, uint64_t seed)
{
    return group_no_throw(g, "icl_group_load_synthetic", [&]() -> int {
    if (!g) return ICL_ERR_ARG;
    return for_each_ctx(g, [&](int, icl_ctx *c) { return icl_model_load_synthetic(c, seed); });
    });
}
extern "C" int icl_group_load_onnx(icl_group *g, const char *path)
{
    return group_no_throw(g, "icl_group_load_onnx", [&]() -> int {
    if (!g || !path) return ICL_ERR_ARG;
    return for_each_ctx(g, [&](int, icl_ctx *c) { return icl_model_load_onnx(c, path); });
    });
}
extern "C" int icl_group_load_blob(icl_group *g, const void *blob, int64_t bytes)
{
    return group_no_throw(g, "icl_group_load_blob", [&]() -> int {
    if (!g || !blob) return ICL_ERR_ARG;
    return for_each_ctx(g, [&](int, icl_ctx *c) { return icl_model_load_blob(c, blob, bytes); });
    });
}

// contiguous index range of part i of n items over `parts` (the first n % parts parts hold one more)
static void shard_range(int64_t n, int parts, int i, int64_t &lo, int64_t &hi)
{
    const int64_t base = n / parts, extra = n % parts;
    lo = i * base + std::min<int64_t>(i, extra);
    hi = lo + base + (i < extra ? 1 : 0);
}

extern "C" int icl_group_embed_u8(icl_group *g, const uint8_t *hwc_rgb, int64_t n, int head, int prec, float *out)
{
    return group_no_throw(g, "icl_group_embed_u8", [&]() -> int {
    if (!g || n < 0 || (n && (!hwc_rgb || !out))) return group_fail(g, ICL_ERR_ARG, "icl_group_embed_u8: bad argument");
    const int parts = (int)g->ctx.size();
    return for_each_ctx(g, [&](int i, icl_ctx *c) {
        int64_t lo, hi;
        shard_range(n, parts, i, lo, hi);
        if (hi == lo) return (int)ICL_OK;
        return icl_embed_u8(c, hwc_rgb + lo * (int64_t)ICL_IMG_BYTES, hi - lo, head, prec, out + lo * head);
    });
    });
}

// The distance build + merge loop of a group on embeddings that are ALREADY resident on every GPU (dE[i]: n x d on GPU i).
// Local build: GPU 0 alone, matrix-core bounds (icl_cluster_dev).  Distributed build: GPUs 1.. compute the exact rows of their
// area-balanced runs into buffers of their own memory; GPU 0 then reads those spans over xGMI straight into its matrix rows
// (all peers concurrently, one link each) -- or, for a device that is no peer, through a bounded landing buffer --, computes
// its own run from bounds and runs the exact merge loop.  Nothing is staged on GPU 0.
static bool group_shards_merges(icl_group *g) { return g->ctx.size() > 1 && g->merge_mode == ICL_MERGE_SHARDED; }
static bool group_deals_rows(icl_group *g, int64_t n, int d) // (also: every GPU needs all of E)
{
    const int parts = (int)g->ctx.size();
    // AUTO since round 5: where GPU 0 can fill the matrix from the integer GEMM (D <= 2048: 63 ms at n = 100 000) it does -- receiving 20 GB
    // (G - 1) / G over its links takes as long as computing them --; the f32 bound rows (0.15 s locally) are still dealt out from 4 GPUs on
    return parts > 1 && (group_shards_merges(g) || g->tiles_mode == ICL_TILES_DISTRIBUTED ||
                         (g->tiles_mode == ICL_TILES_AUTO && parts >= ICL_GROUP_DIST_MIN && !icl_dist_i8_usable(n, d)));
}
// The strip-sharded exact merge loop (ward.hip, "replicated state, sharded blocks"): every GPU runs the WHOLE clustering call on its
// own replica of the state -- its own distance matrix (4 n^2 bytes fit every 288 GB GPU up to configs[4]'s 250 000), built locally from
// the matrix-core bounds -- but its update launches compute only the 64-cluster blocks b == rank (mod G) of the rows being created;
// after each update launch the replicas pull the other blocks' entries out of each other's matrices (peer-mapped memory over xGMI,
// one event wait per peer and step) and finish the step identically.  The per-step vector arithmetic divides by G, the exchange is
// <= 16 rows x n_live x 4 bytes x (G-1)/G per GPU.  Replica 0's outputs are returned; all replicas compute the same ones.
static int group_cluster_sharded(icl_group *g, const std::vector<float *> &dE, int64_t n, int32_t d, int32_t min_size, int32_t max_size,
                                 int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    const int parts = (int)g->ctx.size();
    icl_ward_shard sh;
    sh.G = parts;
    int rc = ICL_OK;
    for (int i = 0; i < parts && rc == ICL_OK; ++i) {
        icl_device_guard dg(g->ctx[(size_t)i]->device);
        for (int k = 0; k < 2 && rc == ICL_OK; ++k)
            if (hipEventCreateWithFlags(&sh.ev[i][k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&sh.evp[i][k], hipEventDisableTiming) != hipSuccess)
                rc = group_fail(g, ICL_ERR_HIP, "sharded merge loop: event creation failed");
    }
    std::vector<std::vector<int32_t>> scratch((size_t)parts);
    std::vector<int32_t> ncl((size_t)parts, 0);
    if (rc == ICL_OK) {
        for (int i = 1; i < parts; ++i) scratch[(size_t)i].assign((size_t)(2 * n), 0);
        for (int i = 0; i < parts; ++i) {
            g->ctx[(size_t)i]->shard = &sh;
            g->ctx[(size_t)i]->shard_rank = i;
        }
        rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
            int32_t *cid = i == 0 ? cluster_id : scratch[(size_t)i].data(), *mr = i == 0 ? member_rank : scratch[(size_t)i].data() + n;
            return icl_cluster_dev(c, dE[(size_t)i], n, d, min_size, max_size, ICL_UPDATE_EXACT, cid, mr, &ncl[(size_t)i]);
        });
        for (int i = 0; i < parts; ++i) g->ctx[(size_t)i]->shard = nullptr;
        if (rc == ICL_OK) {
            *n_clusters = ncl[0];
            for (int i = 1; i < parts; ++i) // the replicas ran the same loop on the same data
                if (ncl[(size_t)i] != ncl[0] || memcmp(scratch[(size_t)i].data(), cluster_id, (size_t)n * 4) != 0)
                    rc = group_fail(g, ICL_ERR_HIP, "sharded merge loop: replica " + std::to_string(i) + " disagrees with replica 0 (engine bug)");
        }
    }
    for (int i = 0; i < parts; ++i) {
        icl_device_guard dg(g->ctx[(size_t)i]->device);
        for (int k = 0; k < 2; ++k) {
            if (sh.ev[i][k]) (void)hipEventDestroy(sh.ev[i][k]);
            if (sh.evp[i][k]) (void)hipEventDestroy(sh.evp[i][k]);
        }
    }
    return rc;
}
static int group_cluster_resident(icl_group *g, const std::vector<float *> &dE, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                                  int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    const int parts = (int)g->ctx.size();
    icl_ctx *c0 = g->ctx[0];
    if (group_shards_merges(g) && update == ICL_UPDATE_EXACT) return group_cluster_sharded(g, dE, n, d, min_size, max_size, cluster_id, member_rank, n_clusters);
    if (!group_deals_rows(g, n, d)) {
        const int rc = icl_cluster_dev(c0, dE[0], n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
        return rc == ICL_OK ? rc : group_fail(g, rc, icl_last_error(c0));
    }
    int rc = icl_ward_prepare(c0, n, d);
    if (rc != ICL_OK) return group_fail(g, rc, icl_last_error(c0));
    std::vector<float *> dSpan((size_t)parts, nullptr);
    std::vector<int64_t> lo((size_t)parts, 0), hi((size_t)parts, 0), cnt((size_t)parts, 0);
    for (int i = 0; i < parts && rc == ICL_OK; ++i) {
        int64_t off = 0;
        rc = icl_ward_rows_partition(n, parts, i, &lo[(size_t)i], &hi[(size_t)i]);
        if (rc == ICL_OK) rc = icl_ward_span(lo[(size_t)i], hi[(size_t)i], &off, &cnt[(size_t)i]);
    }
    if (rc != ICL_OK) return group_fail(g, rc, "row partition failed");
    rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
        if (i == 0 || hi[(size_t)i] == lo[(size_t)i]) return ICL_OK; // GPU 0's own run is computed by the cluster call below
        void *p = nullptr;
        ICL_TRY(icl_dev_malloc(c, std::max<int64_t>(cnt[(size_t)i] * 4, 16), &p));
        dSpan[(size_t)i] = (float *)p;
        return icl_ward_distance_rows_dev(c, dE[(size_t)i], n, d, lo[(size_t)i], hi[(size_t)i], dSpan[(size_t)i]);
    });
    if (rc == ICL_OK) { // the spans GPU 0 can read where they lie: all at once
        int64_t plo[ICL_GROUP_MAX], phi[ICL_GROUP_MAX];
        const float *pp[ICL_GROUP_MAX];
        int np = 0;
        for (int i = 1; i < parts; ++i)
            if (dSpan[(size_t)i] && g->peer0[(size_t)i]) {
                plo[np] = lo[(size_t)i];
                phi[np] = hi[(size_t)i];
                pp[np++] = dSpan[(size_t)i];
            }
        if (np) rc = icl_ward_unpack_spans_dev(c0, np, plo, phi, pp);
        if (rc != ICL_OK) group_fail(g, rc, icl_last_error(c0));
    }
    if (rc == ICL_OK) { // no peer access to a device: runs of whole rows through one landing buffer of at most 256 MiB (+ one row)
        void *land = nullptr;
        int64_t land_floats = 0;
        for (int i = 1; i < parts && rc == ICL_OK; ++i) {
            if (!dSpan[(size_t)i] || g->peer0[(size_t)i]) continue;
            int64_t r0 = lo[(size_t)i];
            while (r0 < hi[(size_t)i] && rc == ICL_OK) {
                int64_t r1 = r0 + 1, off0 = 0, c1 = 0, offb = 0, cb = 0;
                (void)icl_ward_span(lo[(size_t)i], r0, &offb, &cb); // floats of this span before row r0
                while (r1 < hi[(size_t)i] && icl_ward_span(r0, r1 + 1, &off0, &c1) == ICL_OK && c1 <= (64LL << 20)) ++r1;
                (void)icl_ward_span(r0, r1, &off0, &c1);
                if (c1 > land_floats) {
                    if (land) (void)icl_dev_free(c0, land);
                    land = nullptr;
                    rc = icl_dev_malloc(c0, c1 * 4, &land);
                    land_floats = rc == ICL_OK ? c1 : 0;
                }
                if (rc == ICL_OK && c1 > 0) {
                    icl_device_guard dg(c0->device);
                    if (hipMemcpyPeer(land, c0->device, dSpan[(size_t)i] + cb, g->ctx[(size_t)i]->device, (size_t)c1 * 4) != hipSuccess)
                        rc = icl_fail(c0, ICL_ERR_HIP, "copy of distance rows [%lld, %lld) from GPU %d failed", (long long)r0, (long long)r1, g->ctx[(size_t)i]->device);
                    const float *lp = (const float *)land;
                    if (rc == ICL_OK) rc = icl_ward_unpack_spans_dev(c0, 1, &r0, &r1, &lp);
                }
                r0 = r1;
            }
        }
        if (land) (void)icl_dev_free(c0, land);
        if (rc != ICL_OK) group_fail(g, rc, icl_last_error(c0));
    }
    for (int i = 0; i < parts; ++i)
        if (dSpan[(size_t)i]) (void)icl_dev_free(g->ctx[(size_t)i], dSpan[(size_t)i]);
    if (rc == ICL_OK) {
        rc = icl_cluster_prefilled_dev(c0, dE[0], n, d, min_size, max_size, update, lo[0], hi[0], cluster_id, member_rank, n_clusters);
        if (rc != ICL_OK) group_fail(g, rc, icl_last_error(c0));
    }
    return rc;
}

extern "C" int icl_group_cluster(icl_group *g, const float *E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int update,
                                 int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return group_no_throw(g, "icl_group_cluster", [&]() -> int {
    if (!g || n < 0 || d < 0 || !n_clusters || (n && (!E || !cluster_id || !member_rank))) return group_fail(g, ICL_ERR_ARG, "icl_group_cluster: bad argument");
    const int parts = (int)g->ctx.size();
    icl_ctx *c0 = g->ctx[0];
    int64_t kk = 0;
    if (parts == 1 || update != ICL_UPDATE_EXACT || n < 2 * 128 * parts || icl_calc_optimal_clusters(n, min_size, max_size, &kk) != ICL_OK) {
        // one GPU, FAST mode (its MFMA tile is built on one GPU), inputs too small to deal out, or constraint errors: plain call
        const int rc = icl_cluster(c0, E, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
        return rc == ICL_OK ? rc : group_fail(g, rc, icl_last_error(c0));
    }
    // E crosses PCIe ONCE (into GPU 0); the other GPUs get it by peer copies (xGMI when the devices are peers) -- only when they
    // compute distance rows
    const bool deal = group_deals_rows(g, n, d);
    std::vector<float *> dE((size_t)parts, nullptr);
    auto cleanup = [&] {
        for (int i = 0; i < parts; ++i)
            if (dE[(size_t)i]) (void)icl_dev_free(g->ctx[(size_t)i], dE[(size_t)i]);
    };
    const int64_t ebytes = n * (int64_t)d * 4;
    int rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
        if (i && !deal) return ICL_OK;
        void *p = nullptr;
        ICL_TRY(icl_dev_malloc(c, std::max<int64_t>(ebytes, 16), &p));
        dE[(size_t)i] = (float *)p;
        return i == 0 ? icl_memcpy_h2d(c, p, E, ebytes) : (int)ICL_OK;
    });
    if (rc == ICL_OK && deal)
        rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
            if (i == 0) return ICL_OK;
            icl_device_guard dg(c->device);
            if (hipMemcpyPeer(dE[(size_t)i], c->device, dE[0], c0->device, (size_t)ebytes) != hipSuccess)
                return icl_fail(c, ICL_ERR_HIP, "peer copy of E from GPU %d failed: %s", c0->device, hipGetErrorString(hipGetLastError()));
            return ICL_OK;
        });
    if (rc == ICL_OK) rc = group_cluster_resident(g, dE, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
    cleanup();
    return rc;
    });
}

// workflow.go:84-94 in one call: createEmbeddings (the per-image GetImageEmbedding fan-out, :149-185) followed by
// PerformClusteringWithConstraints (:89) -- with the embeddings staying ON the GPUs in between.  Images shard by contiguous
// index ranges; every GPU embeds its shard straight into its own full-size E buffer; the shards are exchanged by peer copies
// (an all-gather written as N x (N-1) point-to-point copies: xGMI is a mesh of links, every byte crosses exactly one);
// then the distance rows / merge loop of group_cluster_resident.  Nothing crosses PCIe between embed and cluster; E_out
// (host, n x 2048, may be NULL) receives the pooled embeddings afterwards.  Results are bit-identical to
// icl_embed_u8 + icl_cluster on one GPU.
extern "C" int icl_group_embed_cluster(icl_group *g, const uint8_t *hwc_rgb, int64_t n, int prec, int32_t min_size, int32_t max_size, int update,
                                       float *E_out, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters)
{
    return group_no_throw(g, "icl_group_embed_cluster", [&]() -> int {
    if (!g || n < 0 || !n_clusters || (n && (!hwc_rgb || !cluster_id || !member_rank))) return group_fail(g, ICL_ERR_ARG, "icl_group_embed_cluster: bad argument");
    const int parts = (int)g->ctx.size();
    const int32_t d = ICL_HEAD_POOLED;
    icl_ctx *c0 = g->ctx[0];
    int64_t kk = 0;
    if (n == 0) {
        *n_clusters = 0;
        return ICL_OK;
    }
    // every GPU needs all of E only when the distance rows are dealt out (icl_group_set_options); otherwise the shards go to GPU 0
    const bool resident = group_deals_rows(g, n, ICL_HEAD_POOLED) && update == ICL_UPDATE_EXACT && n >= 2 * 128 * parts && icl_calc_optimal_clusters(n, min_size, max_size, &kk) == ICL_OK;
    std::vector<float *> dE((size_t)parts, nullptr);
    auto cleanup = [&] {
        for (int i = 0; i < parts; ++i)
            if (dE[(size_t)i]) (void)icl_dev_free(g->ctx[(size_t)i], dE[(size_t)i]);
    };
    const int64_t ebytes = n * (int64_t)d * 4;
    // 1. every GPU embeds its shard into its own n x 2048 buffer (only GPU 0 needs the full buffer when the rest is not dealt out).
    // The buffers exist BEFORE the host threads start: the workers of GPUs 1.. copy into GPU 0's buffer in the non-resident path.
    int rc = ICL_OK;
    for (int i = 0; i < parts && rc == ICL_OK; ++i)
        if (i == 0 || resident) {
            void *p = nullptr;
            rc = icl_dev_malloc(g->ctx[(size_t)i], std::max<int64_t>(ebytes, 16), &p);
            dE[(size_t)i] = (float *)p;
            if (rc != ICL_OK) group_fail(g, rc, std::string("GPU ") + std::to_string(i) + ": " + icl_last_error(g->ctx[(size_t)i]));
        }
    if (rc == ICL_OK)
      rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
        int64_t lo, hi;
        shard_range(n, parts, i, lo, hi);
        if (hi == lo) return ICL_OK;
        void *di = nullptr;
        ICL_TRY(icl_dev_malloc(c, (hi - lo) * (int64_t)ICL_IMG_BYTES, &di));
        int r2 = icl_memcpy_h2d(c, di, hwc_rgb + lo * (int64_t)ICL_IMG_BYTES, (hi - lo) * (int64_t)ICL_IMG_BYTES);
        float *dst = dE[(size_t)i] ? dE[(size_t)i] + lo * d : nullptr;
        void *tmp = nullptr;
        if (r2 == ICL_OK && !dst) { // not dealt out: the shard goes to a buffer of its own and is copied to GPU 0 below
            r2 = icl_dev_malloc(c, (hi - lo) * (int64_t)d * 4, &tmp);
            dst = (float *)tmp;
        }
        if (r2 == ICL_OK) r2 = icl_embed_u8_dev(c, (const uint8_t *)di, hi - lo, d, prec, dst);
        if (r2 == ICL_OK && tmp) {
            icl_device_guard dg(c->device);
            if (hipMemcpyPeer(dE[0] + lo * d, c0->device, tmp, c->device, (size_t)((hi - lo) * (int64_t)d * 4)) != hipSuccess)
                r2 = icl_fail(c, ICL_ERR_HIP, "peer copy of an embedding shard to GPU %d failed", c0->device);
        }
        (void)icl_dev_free(c, di);
        if (tmp) (void)icl_dev_free(c, tmp);
        return r2;
    });
    // 2. the all-gather of E as point-to-point copies: GPU i sends its shard to every other GPU (all pairs concurrently)
    if (rc == ICL_OK && resident)
        rc = for_each_ctx(g, [&](int i, icl_ctx *c) -> int {
            int64_t lo, hi;
            shard_range(n, parts, i, lo, hi);
            if (hi == lo) return ICL_OK;
            icl_device_guard dg(c->device);
            hipStream_t cs = nullptr;
            hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
            for (int j = 0; j < parts && e == hipSuccess; ++j)
                if (j != i)
                    e = hipMemcpyPeerAsync(dE[(size_t)j] + lo * d, g->ctx[(size_t)j]->device, dE[(size_t)i] + lo * d, c->device, (size_t)((hi - lo) * (int64_t)d * 4), cs);
            if (e == hipSuccess) e = hipStreamSynchronize(cs);
            if (cs) (void)hipStreamDestroy(cs);
            return e == hipSuccess ? (int)ICL_OK : icl_fail(c, ICL_ERR_HIP, "all-gather of E (peer copies from GPU %d) failed: %s", c->device, hipGetErrorString(e));
        });
    // 3. cluster on the resident embeddings
    if (rc == ICL_OK) {
        if (resident) rc = group_cluster_resident(g, dE, n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
        else {
            rc = icl_cluster_dev(c0, dE[0], n, d, min_size, max_size, update, cluster_id, member_rank, n_clusters);
            if (rc != ICL_OK) group_fail(g, rc, icl_last_error(c0));
        }
    }
    if (rc == ICL_OK && E_out) {
        rc = icl_memcpy_d2h(c0, E_out, dE[0], ebytes);
        if (rc != ICL_OK) group_fail(g, rc, icl_last_error(c0));
    }
    cleanup();
    return rc;
    });
}
