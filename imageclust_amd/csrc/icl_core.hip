// icl_core.hip -- context, error, memory, profiling and synthetic-input entry points of the C-ABI.
#include "icl_common.h"

#include <cstring>

static thread_local std::string g_tls_err;

int icl_fail(icl_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_tls_err = buf;
    return code;
}

extern "C" const char *icl_version(void) { return "imageclust_hip 0.1 (gfx950)"; }

extern "C" const char *icl_last_error(icl_ctx *ctx) { return ctx ? ctx->err.c_str() : g_tls_err.c_str(); }

extern "C" int icl_create(int device, icl_ctx **out)
{
    if (!out) return icl_fail(nullptr, ICL_ERR_ARG, "icl_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return icl_fail(nullptr, ICL_ERR_HIP, "icl_create: no HIP device available (%s); this library has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return icl_fail(nullptr, ICL_ERR_ARG, "icl_create: device %d out of range [0,%d)", device, ndev);
    icl_ctx *c = new icl_ctx();
    c->device = device;
    icl_device_guard g(device);
    if (!g.ok) {
        delete c;
        return icl_fail(nullptr, ICL_ERR_HIP, "icl_create: hipSetDevice(%d) failed", device);
    }
    e = hipGetDeviceProperties(&c->prop, device);
    if (e != hipSuccess) {
        delete c;
        return icl_fail(nullptr, ICL_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    }
    if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
        std::string arch = c->prop.gcnArchName;
        delete c;
        return icl_fail(nullptr, ICL_ERR_HIP, "icl_create: device %d is %s; this library is built for gfx950 only", device, arch.c_str());
    }
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return icl_fail(nullptr, ICL_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    if (hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return icl_fail(nullptr, ICL_ERR_HIP, "icl_create: side stream / events");
    }
    if (const char *ew = getenv("ICL_CONV_WR")) c->conv_wr = atoi(ew) != 0;
    if (const char *es = getenv("ICL_CONV_SK")) c->conv_sk = atoi(es) != 0;
    if (const char *ep = getenv("ICL_PRUNE")) c->fwd_prune = atoi(ep) != 0; // A/B runs: the default of icl_set_forward_prune
    if (const char *ef = getenv("ICL_PRUNE_FUSED")) c->fwd_prune_fused = atoi(ef) != 0; // A/B runs: the default of icl_set_forward_prune_fused
    if (const char *ek = getenv("ICL_CONV_SK_MINK")) c->conv_sk_min_k = std::max(512, atoi(ek));
    if (const char *e8 = getenv("ICL_CONV_P8")) { // A/B runs: the default of icl_set_conv_options
        const int v = atoi(e8);
        if (v >= ICL_CONV_P8_OFF && v <= ICL_CONV_P8_ALL) c->conv_p8 = v;
    }
    if (const char *ej = getenv("ICL_JPEG_ENTROPY")) c->entropy_mode = strcmp(ej, "gpu") == 0 ? ICL_ENTROPY_GPU : ICL_ENTROPY_HOST;
    if (const char *ep = getenv("ICL_PNG_INFLATE")) c->png_mode = strcmp(ep, "gpu") == 0 ? ICL_PNG_GPU : ICL_PNG_HOST;
    if (const char *em = getenv("ICL_MANY_MID"))
        c->many_mid = strcmp(em, "on") == 0 ? ICL_MANY_MID_ON : strcmp(em, "off") == 0 ? ICL_MANY_MID_OFF : ICL_MANY_MID_AUTO;
    *out = c;
    return ICL_OK;
}

extern "C" void icl_destroy(icl_ctx *ctx)
{
    if (!ctx) return;
    icl_device_guard g(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    icl_model_free(ctx);
    icl_ward_free(ctx);
    icl_file_batcher_free(ctx);
    icl_ingest_free(ctx);
    ctx->many.release();
    icl_requests_free(ctx);
    icl_jenc_free(ctx);
    ctx->nearest.release();
    ctx->pairs.release();
    ctx->fit.release();
    ctx->fold.release();
    for (auto &p : ctx->pending) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    for (auto ev : ctx->event_pool) (void)hipEventDestroy(ev);
    for (auto &s : ctx->sk) {
        if (s.part) (void)hipFree(s.part);
        if (s.flag) (void)hipFree(s.flag);
    }
    (void)hipStreamDestroy(ctx->stream);
    (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->ev_s3) (void)hipEventDestroy(ctx->ev_s3);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
    delete ctx;
}

extern "C" void *icl_stream(icl_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int icl_sync(icl_ctx *ctx)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icl_prof_collect(ctx);
    return ICL_OK;
}

extern "C" int icl_device_info(icl_ctx *ctx, char *name, int cap, int *n_cu, int64_t *hbm)
{
    if (!ctx) return ICL_ERR_ARG;
    if (name && cap > 0) snprintf(name, (size_t)cap, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (n_cu) *n_cu = ctx->prop.multiProcessorCount;
    if (hbm) *hbm = (int64_t)ctx->prop.totalGlobalMem;
    return ICL_OK;
}

extern "C" int icl_dev_malloc(icl_ctx *ctx, int64_t bytes, void **dptr)
{
    if (!ctx || !dptr || bytes < 0) return icl_fail(ctx, ICL_ERR_ARG, "icl_dev_malloc: bad argument");
    icl_device_guard g(ctx->device);
    *dptr = nullptr;
    if (bytes == 0) return ICL_OK;
    hipError_t e = hipMalloc(dptr, (size_t)bytes);
    if (e != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "hipMalloc(%lld) failed: %s", (long long)bytes, hipGetErrorString(e));
    return ICL_OK;
}

extern "C" int icl_dev_free(icl_ctx *ctx, void *dptr)
{
    if (!ctx) return ICL_ERR_ARG;
    icl_device_guard g(ctx->device);
    if (dptr) {
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ICL_HIP(ctx, hipFree(dptr));
    }
    return ICL_OK;
}

extern "C" int icl_memcpy_h2d(icl_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
    if (!ctx || bytes < 0 || (bytes && (!dst || !src))) return icl_fail(ctx, ICL_ERR_ARG, "icl_memcpy_h2d: bad argument");
    icl_device_guard g(ctx->device);
    if (bytes) {
        ICL_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ICL_OK;
}

extern "C" int icl_memcpy_d2h(icl_ctx *ctx, void *dst, const void *src, int64_t bytes)
{
    if (!ctx || bytes < 0 || (bytes && (!dst || !src))) return icl_fail(ctx, ICL_ERR_ARG, "icl_memcpy_d2h: bad argument");
    icl_device_guard g(ctx->device);
    if (bytes) {
        ICL_HIP(ctx, hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ICL_OK;
}

extern "C" int icl_set_batch(icl_ctx *ctx, int batch)
{
    if (!ctx || batch < 1 || batch > 1024) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_batch: batch must be in [1,1024]");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->batch = batch;
    return ICL_OK;
}

extern "C" int icl_set_conv_options(icl_ctx *ctx, int p8_mode)
{
    const int mode = p8_mode & ~ICL_CONV_SPLIT;
    if (!ctx || p8_mode < 0 || mode < ICL_CONV_P8_OFF || mode > ICL_CONV_P8_ALL)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_set_conv_options: p8_mode must be 0, 1 or 2 (| ICL_CONV_SPLIT)");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->conv_p8 = mode;
    ctx->conv_sk = (p8_mode & ICL_CONV_SPLIT) ? 1 : 0;
    return ICL_OK;
}

extern "C" int icl_set_forward_prune(icl_ctx *ctx, int on)
{
    if (!ctx || on < 0 || on > 1) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_forward_prune: on must be 0 or 1");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->fwd_prune = on;
    return ICL_OK;
}

extern "C" int icl_forward_prune_stats(icl_ctx *ctx, int64_t *pruned_blocks)
{
    if (!ctx || !pruned_blocks) return icl_fail(ctx, ICL_ERR_ARG, "icl_forward_prune_stats: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    *pruned_blocks = ctx->pruned_blocks;
    return ICL_OK;
}

extern "C" int icl_set_forward_prune_fused(icl_ctx *ctx, int on)
{
    if (!ctx || on < 0 || on > 1) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_forward_prune_fused: on must be 0 or 1");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->fwd_prune_fused = on;
    return ICL_OK;
}

extern "C" int icl_set_stem_max_blocks(icl_ctx *ctx, int max_blocks)
{
    if (!ctx || max_blocks < 0) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_stem_max_blocks: max_blocks must be 0 (no cap) or positive");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->stem_max_blocks = max_blocks;
    return ICL_OK;
}

extern "C" int icl_forward_prune_fused_stats(icl_ctx *ctx, int64_t *pruned_launches)
{
    if (!ctx || !pruned_launches) return icl_fail(ctx, ICL_ERR_ARG, "icl_forward_prune_fused_stats: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    *pruned_launches = ctx->pruned_fused;
    return ICL_OK;
}

extern "C" int icl_conv_split_launches(icl_ctx *ctx, int64_t *launches)
{
    if (!ctx || !launches) return icl_fail(ctx, ICL_ERR_ARG, "icl_conv_split_launches: NULL argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    *launches = ctx->conv_sk_launches;
    return ICL_OK;
}

extern "C" int icl_conv_stats(icl_ctx *ctx, int64_t *p8_launches, int64_t *other_launches)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "icl_conv_stats: ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (p8_launches) *p8_launches = ctx->conv_launches[0];
    if (other_launches) *other_launches = ctx->conv_launches[1];
    return ICL_OK;
}

// ---- profiling ------------------------------------------------------------------------------------------
static hipEvent_t take_event(icl_ctx *c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

icl_prof_scope::icl_prof_scope(icl_ctx *ctx, int kclass, double flops, double bytes) : c(ctx), k(kclass)
{
    if (!((c->prof_mask >> k) & 1)) return;
    c->prof[k].flops += flops;
    c->prof[k].bytes += bytes;
    c->prof[k].launches += 1;
    a = take_event(c);
    b = take_event(c);
    (void)hipEventRecord(a, c->stream);
}

icl_prof_scope::~icl_prof_scope()
{
    if (!a) return;
    (void)hipEventRecord(b, c->stream);
    c->pending.push_back({a, b, k});
}

void icl_prof_collect(icl_ctx *ctx)
{
    for (auto &p : ctx->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) ctx->prof[p.kclass].ms += ms;
        ctx->event_pool.push_back(p.a);
        ctx->event_pool.push_back(p.b);
    }
    ctx->pending.clear();
}

extern "C" int icl_prof_enable(icl_ctx *ctx, int class_mask)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->prof_mask = class_mask;
    return ICL_OK;
}

extern "C" int icl_prof_reset(icl_ctx *ctx)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icl_prof_collect(ctx);
    for (auto &s : ctx->prof) s = icl_prof_slot();
    return ICL_OK;
}

extern "C" int icl_prof_query(icl_ctx *ctx, int k, double *ms, int64_t *launches, double *flops, double *bytes)
{
    if (!ctx || k < 0 || k >= ICL_K_NCLASS) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icl_prof_collect(ctx);
    if (ms) *ms = ctx->prof[k].ms;
    if (launches) *launches = ctx->prof[k].launches;
    if (flops) *flops = ctx->prof[k].flops;
    if (bytes) *bytes = ctx->prof[k].bytes;
    return ICL_OK;
}

extern "C" int icl_last_stage_ms(icl_ctx *ctx, double *embed_ms, double *dist_ms, double *merge_ms)
{
    if (!ctx) return ICL_ERR_ARG;
    if (embed_ms) *embed_ms = ctx->last_embed_ms;
    if (dist_ms) *dist_ms = ctx->last.dist_ms;
    if (merge_ms) *merge_ms = ctx->last.merge_ms;
    return ICL_OK;
}

// ---- synthetic images --------------------------------------------------------------------------------------
extern "C" int icl_synth_images(uint64_t seed, int64_t first, int64_t n, int mode, uint8_t *out)
{
    if (n < 0 || first < 0 || (n && !out) || (mode != ICL_SYNTH_NOISE && mode != ICL_SYNTH_STRUCTURED))
        return icl_fail(nullptr, ICL_ERR_ARG, "icl_synth_images: bad argument");
    for (int64_t i = 0; i < n; ++i)
        for (uint32_t off = 0; off < (uint32_t)ICL_IMG_BYTES; ++off)
            out[i * ICL_IMG_BYTES + off] = icl_synth_pixel(seed, first + i, off, mode);
    return ICL_OK;
}

__global__ void synth_images_kernel(uint64_t seed, int64_t first, int64_t n, int mode, uint8_t *__restrict__ out)
{
    // one thread = 4 consecutive bytes of one image (150528 is a multiple of 4)
    const int64_t total = n * (int64_t)(ICL_IMG_BYTES / 4);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t img = t / (ICL_IMG_BYTES / 4);
        uint32_t off = (uint32_t)(t % (ICL_IMG_BYTES / 4)) * 4u;
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) w |= (uint32_t)icl_synth_pixel(seed, first + img, off + b, mode) << (8 * b);
        reinterpret_cast<uint32_t *>(out)[t] = w;
    }
}

extern "C" int icl_synth_images_dev(icl_ctx *ctx, uint64_t seed, int64_t first, int64_t n, int mode, uint8_t *d_out)
{
    if (!ctx || n < 0 || first < 0 || (n && !d_out) || (mode != ICL_SYNTH_NOISE && mode != ICL_SYNTH_STRUCTURED))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_synth_images_dev: bad argument");
    if (n == 0) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    int64_t total = n * (int64_t)(ICL_IMG_BYTES / 4);
    int blocks = (int)std::min<int64_t>(icl_ceil_div(total, 256), 256 * 16);
    hipLaunchKernelGGL(synth_images_kernel, dim3(blocks), dim3(256), 0, ctx->stream, seed, first, n, mode, d_out);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}
