// icl_common.h -- internal definitions shared by the translation units of libimageclust_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/icl_model_format.h"
#include "../../include/imageclust.h"

#define ICL_MAXF 3.40282346638528859811704183484516925e+38f /* math.MaxFloat32 */

struct icl_ctx;
int icl_fail(icl_ctx *ctx, int code, const char *fmt, ...);
static inline hipStream_t icl_main_stream(const icl_ctx *ctx); // ctx->stream, defined behind icl_ctx (icl_dev_mem.h is read before icl_ctx is complete)

#define ICL_HIP(ctx, call)                                                                                     \
    do {                                                                                                       \
        hipError_t e__ = (call);                                                                               \
        if (e__ != hipSuccess)                                                                                 \
            return icl_fail(ctx, ICL_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, \
                            __LINE__);                                                                         \
    } while (0)

#define ICL_TRY(expr)            \
    do {                         \
        int rc__ = (expr);       \
        if (rc__) return rc__;   \
    } while (0)

// dev_guard + icl_dev_alloc, icl_dev_grow, icl_ws_layout: the host side's owners of device memory
#include "icl_dev_mem.h"

struct icl_prof_slot {
    double ms = 0, flops = 0, bytes = 0;
    int64_t launches = 0;
};

struct icl_pending_event {
    hipEvent_t a, b;
    int kclass;
};

struct icl_model;  // resnet_model.h
struct icl_ward_ws; // ward.hip
struct icl_ingest_ws; // jpeg_gpu.hip
struct icl_requests_ws; // requests.hip
struct icl_jenc_ws; // jpeg_encode_gpu.hip

// Strip-sharded merge loop (ward.hip "replicated state, sharded blocks"; multi_gpu.hip): what the G replicas of one group call share.
#define ICL_SHARD_MAX 16
struct icl_ward_shard {
    int G = 0;
    const float *D[ICL_SHARD_MAX] = {};   // replica r's distance matrix, published once its workspace exists
    hipEvent_t ev[ICL_SHARD_MAX][2] = {}; // replica r's "update launch of this step is complete" (two alternate)
    hipEvent_t evp[ICL_SHARD_MAX][2] = {}; // replica r's "pull of this step is complete": the peers' NEXT update launch waits for it
    // host barrier over the G driving threads; a replica that fails releases the others
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    long long gen = 0;
    bool failed = false;
    bool wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        const long long my = gen;
        if (++arrived == G) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        cv.wait(lk, [&] { return gen != my || failed; });
        return !failed;
    }
    void fail()
    {
        std::lock_guard<std::mutex> lk(mu);
        failed = true;
        cv.notify_all();
    }
};

struct icl_sk_slot { // scratch of the split convolution launches of one stream (conv_p8.h)
    hipStream_t stream = nullptr;
    void *part = nullptr;
    int *flag = nullptr;
    int cap = 0, epoch = 0;
};

// Everything the last icl_cluster reports about its merge loop (cluster_locked, ward.hip, writes it; the icl_last_* entry points read
// it).  One value, so that a call which must leave the reports alone (icl_cluster_many) saves and restores all of them.
struct icl_ward_report {
    std::vector<int32_t> merges;   // pairs (icl_last_merges)
    std::vector<float> merge_vals; // Ward distance of each merged pair (icl_last_merge_values)
    int64_t bound_viol = 0;        // icl_last_ward_bound_violations
    int32_t mode[2] = {0, 0};      // icl_last_ward_mode: which update kernel the merge loop ran (ICL_ROWS_*), whether the initial matrix held bounds
    int64_t layout[3] = {0, 0, 0}; // complete rows (columns by creation id)?, row pitch in floats, int8 bounds? (icl_last_ward_layout)
    int64_t stats[4] = {0, 0, 0, 0}; // merges, steps, single-pick steps, sum of live clusters over steps (icl_last_ward_stats)
    double dist_ms = 0, merge_ms = 0; // icl_last_timings
};

// What a batched file call counts (ingest_files, jpeg_gpu.hip) and icl_last_ingest_stats / _entropy_stats / _png_stats report.
struct ingest_totals {
    int64_t gpu_jpegs = 0, host_files = 0, upload = 0; // JPEGs rebuilt on the GPU, files decoded on the host, bytes uploaded
    int64_t decode_ns = 0;                             // host thread time in stage A / host decode
    int64_t gpu_entropy = 0, host_entropy = 0, redone_jpegs = 0, stream_bytes = 0; // JPEGs entropy-decoded on the GPU, by host stage A, redone on the host
    int64_t gpu_pngs = 0, host_pngs = 0, redone_pngs = 0, png_bytes = 0;           // PNGs decoded on the GPU, by the host route, redone on the host; zlib bytes
};
// What icl_downsize_images[_mem] counts (jpeg_gpu.hip) and icl_last_downsize_stats reports.
struct dz_totals {
    int64_t passthrough = 0, gpu_rebuilt = 0, host_decoded = 0, second_attempts = 0, bytes_in = 0, bytes_out = 0;
    int64_t decode_ns = 0;          // host decode, thread time
    double gpu_ms = 0, out_ms = 0;  // GPU rebuild + encode; download + copy
};

struct icl_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr; // side stream: the second forward pass in flight (resnet.hip)
    hipStream_t stream3 = nullptr; // side stream: distance rows of already-embedded images beside the forward passes (icl_embed_cluster_dev; created on first use)
    hipEvent_t ev_s3 = nullptr;
    // called by the embed loop after it has enqueued a batch: (first image, images, event recorded behind the batch); set only by icl_embed_cluster_dev
    std::function<int(int64_t, int64_t, hipEvent_t)> embed_hook;
    hipStream_t cur_stream = nullptr; // stream the convolution launches of the forward pass being enqueued go to (nullptr: stream)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::mutex mu;
    std::string err;
    hipDeviceProp_t prop;
    int batch = 256;
    int64_t conv_launches[2] = {0, 0}; // [0] conv_wr_kernel and conv_p8_kernel, [1] the 128 x BN kernels (conv_choice::counter; icl_conv_stats)
    int conv_wr = 1; // the streaming kernel for the HBM-bound c3 layers (conv_wr.h); ICL_CONV_WR=0 turns it off for A/B runs
    int conv_sk = 0; // latency mode: the 7 x 7 layers' tiles on two workgroups each (conv_p8.h, SPLIT; icl_set_conv_options | ICL_CONV_SPLIT, ICL_CONV_SK=1)
    int conv_sk_min_k = 2048; // ... for layers with at least this K (the K = 1024 layer loses: 30 -> 37 us; ICL_CONV_SK_MINK = 512 ... for A/B runs)
    int64_t conv_sk_launches = 0;
    int fwd_prune = 1; // the bf16 forward pass computes only the pixels a strided block 0 reads of the block in front of it (prune_map.h; icl_set_forward_prune, ICL_PRUNE=0)
    int64_t pruned_blocks = 0; // bottlenecks run in that form (icl_forward_prune_stats)
    icl_sk_slot sk[8];
    int conv_p8 = 1; // icl_set_conv_options: 0 never, 1 auto, 2 every supported shape (conv_p8.h)
    int ward_dist = 0; // icl_set_ward_options: 0 auto, 1 every initial distance by the exact kernel, 2 distance bounds + on-demand exact evaluation
    // profiling
    int prof_mask = 0;
    icl_prof_slot prof[ICL_K_NCLASS];
    std::vector<icl_pending_event> pending;
    std::vector<hipEvent_t> event_pool;
    double last_embed_ms = 0;
    icl_ward_report last; // of the last icl_cluster
    int64_t ward_wide_fail_n = 0; // smallest n at which the 8 n^2-byte matrix could not be allocated on this device (0: never failed)
    // subsystems
    icl_model *model = nullptr;
    icl_ward_ws *ward = nullptr;
    icl_ward_shard *shard = nullptr; // set by the group around a sharded cluster call: this context is replica shard_rank of shard->G
    int shard_rank = 0;
    icl_dev_grow ward_rowoff; // row offsets of the packed triangle for ranks that only compute distance rows (ward.hip)
    int64_t ward_rowoff_n = 0;
    void *file_batcher = nullptr; // icl_embed_file's coalescing queue (embed_file.hip)
    icl_dev_grow many; // workspace of icl_cluster_many (ward_many.hip; grown on demand, released by icl_destroy)
    int many_mid = 0;                 // icl_set_many_options: ICL_MANY_MID_AUTO / _OFF / _ON (environment: ICL_MANY_MID=auto|off|on)
    int64_t many_stats[4] = {0, 0, 0, 0}; // last icl_cluster_many[_dev]: problems on the small, mid and large-N routes, mid-route groups
    icl_ingest_ws *ingest = nullptr; // buffers of the batched file path (jpeg_gpu.hip; created on first use)
    ingest_totals ingest_last;        // last batched file call (icl_last_ingest_stats, icl_last_entropy_stats, icl_last_png_stats)
    int entropy_mode = 0;                 // icl_set_ingest_options: ICL_ENTROPY_HOST / ICL_ENTROPY_GPU (environment: ICL_JPEG_ENTROPY=gpu)
    int png_mode = 0;                     // icl_set_png_options: ICL_PNG_HOST / ICL_PNG_GPU (environment: ICL_PNG_INFLATE=gpu)
    icl_requests_ws *requests = nullptr; // device buffers and stage events of icl_cluster_requests (requests.hip; created on first use)
    double requests_ms[3] = {0, 0, 0};   // last icl_cluster_requests: files -> dense rows, assembly, clustering (icl_last_requests_ms)
    icl_jenc_ws *jenc = nullptr;         // buffers of the GPU JPEG encoder (jpeg_encode_gpu.hip; created on first use)
    dz_totals downsize_last;             // last icl_downsize_images[_mem] (icl_last_downsize_stats)
    icl_dev_grow nearest;                // device copies of sizes / exclude and the partial lists of icl_nearest (nearest.hip; as many)
    int nearest_splits = 0;              // icl_set_nearest_options: column splits per band of query rows (0: the engine decides)
    int64_t nearest_stats[4] = {0, 0, 0, 0}; // last icl_nearest[_dev]: splits used, tiles run, pairs evaluated, workspace bytes (icl_last_nearest_stats)
    icl_dev_grow pairs;                  // device copies of sizes / exclude, counts, tile flags and seg_ptr of icl_pairs_within and icl_pairs_between, whichever runs under ctx->mu (pairs.hip; as many)
    int64_t pairs_stats[4] = {0, 0, 0, 0}; // last icl_pairs_within[_dev]: tiles run in pass 1, tiles with a hit, pairs evaluated, workspace bytes (icl_last_pairs_stats)
    icl_dev_grow fit;                    // device copies of the host arrays, partial lists and keys of icl_cluster_fit / icl_ward_values_at (fit.hip; as many)
    int64_t fit_stats[4] = {0, 0, 0, 0}; // last icl_cluster_fit[_dev]: splits used, tiles run, pairs evaluated, workspace bytes (icl_last_fit_stats)
    int64_t between_stats[5] = {0, 0, 0, 0, 0}; // last icl_pairs_between[_dev]: splits used, tiles run in the count pass, tiles with a hit, pairs evaluated, workspace bytes (icl_last_pairs_between_stats)
    std::vector<const void *> lds_optin; // kernels whose > 64 KiB dynamic-LDS opt-in has been made on this context's device
    int fwd_prune_fused = 1;   // with fwd_prune: the fused stage-1 bottleneck in front of stage 2 runs as bneck56_kernel<false, 2> (icl_set_forward_prune_fused, ICL_PRUNE_FUSED=0)
    int64_t pruned_fused = 0;  // launches of that instantiation by the forward pass (icl_forward_prune_fused_stats)
    int stem_max_blocks = 0;   // tests only (icl_set_stem_max_blocks): at most this many workgroups in a stem kernel's persistent grid, 0 = no cap
    icl_dev_grow fold;                   // device copies of row_ptr, the member list and the members' sizes of icl_fold_centroids (fold.hip)
    int64_t fold_stats[4] = {0, 0, 0, 0}; // last icl_fold_centroids[_dev]: groups, member rows read, longest group, workspace bytes (icl_last_fold_stats)
};

static inline hipStream_t icl_main_stream(const icl_ctx *ctx) { return ctx->stream; }

// RAII: select the context's device for the duration of a call without leaking the change to the caller.
struct icl_device_guard {
    int prev = -1;
    bool ok = true;
    explicit icl_device_guard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~icl_device_guard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// Profiling bracket: when enabled records two events around a launch and attributes algorithmic work.
struct icl_prof_scope {
    icl_ctx *c;
    int k;
    hipEvent_t a = nullptr, b = nullptr;
    icl_prof_scope(icl_ctx *ctx, int kclass, double flops, double bytes);
    ~icl_prof_scope();
};
void icl_prof_collect(icl_ctx *ctx); // resolves pending events (requires the stream to be idle)

// subsystem teardown hooks
void icl_model_free(icl_ctx *ctx);
void icl_ward_free(icl_ctx *ctx);
void icl_file_batcher_free(icl_ctx *ctx);
void icl_ingest_free(icl_ctx *ctx);
void icl_requests_free(icl_ctx *ctx);
void icl_jenc_free(icl_ctx *ctx);

// The two batched halves icl_cluster_requests (requests.hip) joins; both expect ctx->mu held and the context's device selected.
// Each tells its caller apart what the return code alone cannot: "the list was processed and an item of it failed" from "the call stopped".
struct icl_item_failure { // the lowest failed file / problem of a call that ran to its end (index -1: none failed)
    int64_t index = -1;
    int rc = ICL_OK;
    std::string why; // the item's own reason, without the caller's prefix
};
// Where the file pipeline leaves its rows: u8 images on the device (icl_load_images_224_dev), embeddings on the host (icl_embed_files)
// or on the device (icl_embed_files_dev, icl_cluster_requests).  head and prec belong to the embedding sinks.
struct ingest_sink {
    enum kind_t { U8_DEV, EMB_HOST, EMB_DEV } kind;
    void *dst;
    int head, prec;
    bool embeds() const { return kind != U8_DEV; }
    size_t row_bytes() const { return embeds() ? (size_t)head * 4 : (size_t)ICL_IMG_BYTES; }
    void *row(int64_t i) const { return (uint8_t *)dst + (size_t)i * row_bytes(); }
};
// One image of an ingest call: a file (path != NULL), or the caller's own bytes (path == NULL: data[0 .. bytes), used in place, never
// copied).  A memory source stays owned by the caller and must remain valid and unchanged until the call returns: the repair pass of
// ingest_files reads it a second time.  data == NULL or bytes <= 0 is that image's own failure (ICL_ERR_IO, "empty image buffer"), as a
// missing file is.  index is the image's place in the caller's list: it names a memory source in messages.
struct ingest_src {
    const char *path;
    const uint8_t *data;
    int64_t bytes;
    int64_t index;
};
// What a message calls the source: its path, or "image <index> (in memory, <bytes> bytes)" written into buf (image_io.hip).
const char *ingest_src_name(const ingest_src &s, char *buf, size_t cap);
// A caller's list of images as an extern "C" entry point receives it: files (paths) or memory sources (data, bytes).
struct ingest_list {
    bool mem;
    const char *const *paths;
    const uint8_t *const *data;
    const int64_t *bytes;
    int64_t n;
    static ingest_list files(const char *const *paths, int64_t n) { return ingest_list{false, paths, nullptr, nullptr, n}; }
    static ingest_list memory(const uint8_t *const *data, const int64_t *bytes, int64_t n) { return ingest_list{true, nullptr, data, bytes, n}; }
    // What ICL_ERR_ARG covers for a list: NO_ARRAYS for n < 0 or a missing array of a list that is not empty, the index of the first NULL
    // path, else OK.  (An empty or NULL entry of a memory list is that image's own failure.)
    enum : int64_t { OK = -1, NO_ARRAYS = -2 };
    int64_t first_bad() const
    {
        if (n < 0 || (n && (mem ? !data || !bytes : !paths))) return NO_ARRAYS;
        for (int64_t i = 0; !mem && i < n; ++i)
            if (!paths[i]) return i;
        return OK;
    }
    std::vector<ingest_src> srcs() const // (of a checked list)
    {
        std::vector<ingest_src> v((size_t)n);
        for (int64_t i = 0; i < n; ++i) v[(size_t)i] = mem ? ingest_src{nullptr, data[i], bytes[i], i} : ingest_src{paths[i], nullptr, 0, i};
        return v;
    }
};
// jpeg_gpu.hip: the ingest pipeline behind those entry points: one ingest_pass in the context's entropy and PNG modes (per slab:
// slab_collect -> run_slab_decode -> slab_deliver), then a repair pass in host mode over the images the GPU entropy or PNG check rejected.
// (The batched downsizer of the same file runs its rounds likewise: dz_collect -> dz_rebuild -> dz_deliver.)  Returns the code of
// the lowest failed image (status[] carries every image's; failed rows are zero (u8) or NaN) after the whole list has been processed --
// lowest (may be NULL) then names that image -- or the error that stopped it (lowest->index stays -1).
int ingest_files(icl_ctx *ctx, const ingest_src *srcs, int64_t n, int32_t threads, const ingest_sink &sink, int32_t *status, const char *what,
                 icl_item_failure *lowest = nullptr);
static inline void icl_ingest_stats_reset(icl_ctx *ctx) { ctx->ingest_last = ingest_totals(); } // what a batched file call reports
// ward_many.hip: icl_cluster_many[_dev] after the argument check (d_E on the device, or h_E on the host and uploaded there).  Returns the
// code of the lowest failed problem once every problem has its results -- lowest (may be NULL) then names it -- or the error that
// stopped the call (lowest->index stays -1; the per-problem outputs are not valid).
int cluster_many_locked(icl_ctx *ctx, int32_t nprob, const float *d_E, const float *h_E, int64_t e_len, const int64_t *e_off, const int32_t *n,
                        const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank,
                        int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status, icl_item_failure *lowest = nullptr);
// nearest.hip, for every band walk (band_select.h, band_plan::run): the launch of nearest_merge_kernel over [splits][nq][k] partial
// lists on the context's stream.  Expects ctx->mu held and the device selected.
int nearest_merge_launch(icl_ctx *ctx, const float *d_pv, const int32_t *d_pj, int64_t nq, int k, int splits, float *d_val, int32_t *d_idx);

// the rules every clustering call shares: CalculateOptimalClusters, the admission of a seeded problem, the final cluster list
#include "ward_seeds.h"

static inline int64_t icl_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// hipFuncAttributeMaxDynamicSharedMemorySize once per (context, kernel): the attribute belongs to the device's copy of the code
// object, and a group drives one context per GPU (process-wide `static bool` flags would opt in on the first device only).
static inline void icl_lds_optin(icl_ctx *ctx, const void *fn, int bytes)
{
    for (const void *f : ctx->lds_optin)
        if (f == fn) return;
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    ctx->lds_optin.push_back(fn);
}

// splitmix64: the counter-based hash behind every synthetic input.
__host__ __device__ static inline uint64_t icl_splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// One byte of the synthetic image set: image n, byte offset off in HWC order.
__host__ __device__ static inline uint8_t icl_synth_pixel(uint64_t seed, int64_t n, uint32_t off, int mode)
{
    uint64_t h = icl_splitmix64(seed ^ ((uint64_t)n * (uint64_t)ICL_IMG_BYTES + off));
    if (mode == ICL_SYNTH_NOISE) return (uint8_t)(h >> 56);
    // structured: 1000 base patterns made of 16x16-pixel colour blocks, plus +-8 of per-image noise
    uint32_t c = off % 3u, x = (off / 3u) % ICL_IMG_W, y = off / (3u * ICL_IMG_W);
    uint64_t cls = (uint64_t)(n % 1000);
    uint64_t hb = icl_splitmix64((seed * 0x2545F4914F6CDD1Dull) ^ (cls * 4096ull + ((y >> 4) * 14u + (x >> 4)) * 3u + c));
    int base = (int)(hb >> 56);
    int noise = (int)((h >> 56) & 15u) - 8;
    int v = base + noise;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    return (uint8_t)v;
}

// No C++ exception crosses the C ABI: entry points that allocate host memory (std::vector, std::string, std::thread) run their body
// through this guard.
template <typename F>
static int no_throw(icl_ctx *ctx, const char *what, F &&body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return icl_fail(ctx, ICL_ERR_NOMEM, "%s: out of host memory", what);
    } catch (...) {
        return icl_fail(ctx, ICL_ERR_IO, "%s: unexpected failure", what);
    }
}
