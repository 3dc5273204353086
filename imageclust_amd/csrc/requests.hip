// requests.hip -- icl_cluster_requests: workflow.Run (workflow.go:84-94) for a queue of requests in one call, file paths to cluster ids.
//
// A request is a handful of images with labels.  The reference embeds every image (GetImageEmbedding, the "dense0" head), appends a
// one-hot vector over the request's label set (GenerateLabelVector, CombineEmbeddings: embeddings.go:166-183) and clusters the combined
// rows (PerformClusteringWithConstraints).  Both batched halves exist -- ingest_files (jpeg_gpu.hip) turns paths into dense rows on the
// device, cluster_many_locked (ward_many.hip) clusters many problems of exactly this shape -- and this file joins them with one kernel:
//
//   paths --ingest_files, EMB_DEV sink--> dense [n_total][head] --requests_assemble_kernel--> E (request r: n[r] rows of d[r] = head + L[r]
//   floats at e_off[r], rows contiguous, requests back to back: icl_requests_layout) --cluster_many_locked--> ids, ranks, merge logs
//
// The combined rows never leave the device in between (E_out, when asked for, is a copy for the caller).  A request one of whose files
// cannot be read fails as a whole (workflow.go:162-181): it is left out of the problem list the Ward kernels get, so the NaN rows of its
// failed files are written to E but never read.  Everything a request's result depends on is computed by the two halves as they are, so
// the results equal icl_embed_files + CombineEmbeddings on the host + icl_cluster_many bit for bit.
#include <algorithm>
#include <climits>
#include <cstring>

#include "icl_common.h"

// One row of E per workgroup: the dense part is copied, the label columns are zeroed, then -- behind a barrier, so that the 1.0f of a
// listed column is ordered after that column's 0.0f whichever threads wrote them -- the listed columns are set.  d is odd for half of
// all requests, so a row starts on a 4-byte boundary in general: dword stores only.  Duplicate indices store the same value twice; -1
// ("label not in the set", embeddings.go:169) is skipped.  (The host has checked every index against its request's label set; the
// kernel's own `j < L` costs one compare per label and keeps a store inside its row whatever it is handed.)
struct rq_image {
    int64_t dst; // float offset of the image's row in E
    int32_t d;   // row length: head + the request's label-set size
    int32_t pad;
};

__global__ __launch_bounds__(256) void requests_assemble_kernel(const float *__restrict__ dense, int head, const rq_image *__restrict__ tab,
                                                                const int64_t *__restrict__ label_off, const int32_t *__restrict__ label_idx,
                                                                float *__restrict__ E)
{
    const int64_t i = blockIdx.x;
    const rq_image im = tab[i];
    const float *src = dense + i * (int64_t)head;
    float *row = E + im.dst;
    for (int c = threadIdx.x; c < head; c += blockDim.x) row[c] = src[c];
    const int L = im.d - head;
    for (int c = threadIdx.x; c < L; c += blockDim.x) row[head + c] = 0.0f;
    __syncthreads();
    const int64_t lo = label_off[i], hi = label_off[i + 1];
    for (int64_t q = lo + threadIdx.x; q < hi; q += blockDim.x) {
        const int32_t j = label_idx[q];
        if (j >= 0 && j < L) row[head + j] = 1.0f;
    }
}

struct icl_requests_ws {
    icl_dev_grow buf; // grow-only, as the workspace of icl_cluster_many
    hipEvent_t ev[4] = {};
};

void icl_requests_free(icl_ctx *ctx)
{
    if (!ctx || !ctx->requests) return;
    ctx->requests->buf.release();
    for (hipEvent_t e : ctx->requests->ev)
        if (e) (void)hipEventDestroy(e);
    delete ctx->requests;
    ctx->requests = nullptr;
}

static int rq_ensure(icl_ctx *ctx, size_t bytes, char **out)
{
    if (!ctx->requests) ctx->requests = new icl_requests_ws;
    icl_requests_ws *w = ctx->requests;
    for (hipEvent_t &e : w->ev)
        if (!e) ICL_HIP(ctx, hipEventCreate(&e));
    ICL_TRY(w->buf.ensure(ctx, bytes, "icl_cluster_requests: device buffers", (size_t)1 << 20));
    *out = w->buf.as<char>();
    return ICL_OK;
}

// d, e_off, e_len; false when a size is negative or a row length does not fit int32_t
static bool rq_layout(int32_t nreq, const int32_t *n, const int32_t *n_labels, int head, int64_t *e_off, int32_t *d, int64_t *e_len)
{
    int64_t pos = 0;
    for (int32_t r = 0; r < nreq; ++r) {
        if (n[r] < 0 || n_labels[r] < 0 || (int64_t)head + n_labels[r] > INT32_MAX) return false;
        const int64_t dr = (int64_t)head + n_labels[r];
        if (e_off) e_off[r] = pos;
        if (d) d[r] = (int32_t)dr;
        pos += (int64_t)n[r] * dr;
    }
    if (e_len) *e_len = pos;
    return true;
}

extern "C" int icl_requests_layout(int32_t nreq, const int32_t *n, const int32_t *n_labels, int head, int64_t *e_off, int32_t *d, int64_t *e_len)
{
    if (nreq < 0 || head < 0 || (nreq && (!n || !n_labels))) return icl_fail(nullptr, ICL_ERR_ARG, "icl_requests_layout: bad argument");
    for (int32_t r = 0; r < nreq; ++r) // (checked first: nothing is written when an entry is bad)
        if (n[r] < 0 || n_labels[r] < 0 || (int64_t)head + n_labels[r] > INT32_MAX)
            return icl_fail(nullptr, ICL_ERR_ARG, "icl_requests_layout: request %d has n %d, n_labels %d", r, n[r], n_labels[r]);
    rq_layout(nreq, n, n_labels, head, e_off, d, e_len);
    return ICL_OK;
}

// what ICL_ERR_ARG covers: nothing is written when it fails.  The images (imgs: files or, for icl_cluster_requests_mem, memory sources)
// number the sum of n[]: imgs.n is set here, once n[] has been checked.
static int rq_check_args(icl_ctx *ctx, const char *what, int32_t nreq, ingest_list &imgs, const int32_t *n, const int32_t *n_labels, const int64_t *label_off,
                         const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size, int head, int prec, int32_t threads,
                         int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *status)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    if (nreq < 0 || threads < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: nreq %d, threads %d", what, nreq, threads);
    if (head != ICL_HEAD_POOLED && head != ICL_HEAD_DENSE0) return icl_fail(ctx, ICL_ERR_ARG, "%s: head must be 2048 or 1000", what);
    if (prec != ICL_PREC_FP32 && prec != ICL_PREC_BF16 && prec != ICL_PREC_BF16X3)
        return icl_fail(ctx, ICL_ERR_ARG, "%s: prec must be ICL_PREC_FP32, ICL_PREC_BF16 or ICL_PREC_BF16X3", what);
    if (nreq == 0) return ICL_OK;
    if (!n || !n_labels || !label_off || !min_size || !max_size || !n_clusters || !n_merges || !status)
        return icl_fail(ctx, ICL_ERR_ARG, "%s: null per-request array", what);
    int64_t rows = 0;
    for (int32_t r = 0; r < nreq; ++r) {
        if (n[r] < 0 || n_labels[r] < 0 || (int64_t)head + n_labels[r] > INT32_MAX)
            return icl_fail(ctx, ICL_ERR_ARG, "%s: request %d has n %d, n_labels %d", what, r, n[r], n_labels[r]);
        rows += n[r];
    }
    if (rows >= ((int64_t)1 << 30)) return icl_fail(ctx, ICL_ERR_ARG, "%s: %lld images in all", what, (long long)rows);
    imgs.n = rows;
    const int64_t bad = imgs.first_bad();
    if (rows && (bad == ingest_list::NO_ARRAYS || !cluster_id || !member_rank))
        return icl_fail(ctx, ICL_ERR_ARG, imgs.mem ? "%s: null data / bytes / cluster_id / member_rank" : "%s: null paths / cluster_id / member_rank", what);
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    if (label_off[0] < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: label_off[0] is %lld", what, (long long)label_off[0]);
    for (int64_t i = 0; i < rows; ++i)
        if (label_off[i + 1] < label_off[i])
            return icl_fail(ctx, ICL_ERR_ARG, "%s: label_off[%lld] = %lld lies below label_off[%lld] = %lld", what, (long long)i + 1,
                            (long long)label_off[i + 1], (long long)i, (long long)label_off[i]);
    if (label_off[rows] > label_off[0] && !label_idx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null label_idx", what);
    int64_t i = 0;
    for (int32_t r = 0; r < nreq; ++r)
        for (int32_t k = 0; k < n[r]; ++k, ++i)
            for (int64_t q = label_off[i]; q < label_off[i + 1]; ++q)
                if (label_idx[q] < -1 || label_idx[q] >= n_labels[r])
                    return icl_fail(ctx, ICL_ERR_ARG, "%s: request %d, image %d: label index %d outside [-1, %d)", what, r, k, label_idx[q], n_labels[r]);
    return ICL_OK;
}

// ctx->mu held, device selected, a model loaded, nreq > 0
static int cluster_requests_locked(icl_ctx *ctx, const char *what, int32_t nreq, const ingest_src *srcs, const int32_t *n, const int32_t *n_labels,
                                   const int64_t *label_off, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size, int head,
                                   int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges,
                                   int32_t *merges, int32_t *status, int32_t *file_status, float *E_out)
{
    std::vector<int64_t> e_off((size_t)nreq), img((size_t)nreq + 1, 0);
    std::vector<int32_t> d((size_t)nreq);
    int64_t e_len = 0;
    rq_layout(nreq, n, n_labels, head, e_off.data(), d.data(), &e_len);
    for (int32_t r = 0; r < nreq; ++r) img[(size_t)r + 1] = img[(size_t)r] + n[r];
    const int64_t rows = img[(size_t)nreq], nlab = rows ? label_off[rows] : 0;

    // ---- device buffers: [E] [dense rows] [image table] [label_off] [label_idx]; E first, on the allocation's 256-byte boundary ----
    icl_ws_layout L(256);
    const size_t o_e = L.take((size_t)e_len * 4), o_dense = L.take((size_t)rows * head * 4), o_tab = L.take((size_t)rows * sizeof(rq_image)),
                 o_loff = L.take((size_t)(rows + 1) * 8), o_lidx = L.take((size_t)nlab * 4);
    char *ws = nullptr;
    ICL_TRY(rq_ensure(ctx, L.total, &ws));
    hipEvent_t *ev = ctx->requests->ev;
    float *d_E = (float *)(ws + o_e), *d_dense = (float *)(ws + o_dense);
    hipStream_t st = ctx->stream;

    // ---- files -> dense rows (failed files: NaN rows, their code in fstat) ----
    std::vector<int32_t> fstat((size_t)rows, -1);
    icl_item_failure bad_file; // the call's lowest failed file
    ICL_HIP(ctx, hipEventRecord(ev[0], st));
    if (rows) {
        const int rc = ingest_files(ctx, srcs, rows, threads, ingest_sink{ingest_sink::EMB_DEV, d_dense, head, prec}, fstat.data(), what, &bad_file);
        if (rc != ICL_OK && bad_file.index < 0) return rc; // not a file's failure: the pipeline stopped
    }
    ICL_HIP(ctx, hipEventRecord(ev[1], st));

    // ---- dense rows + labels -> E ----
    std::vector<int32_t> req_st((size_t)nreq, ICL_OK);
    if (rows) {
        std::vector<rq_image> tab((size_t)rows);
        for (int32_t r = 0; r < nreq; ++r)
            for (int32_t k = 0; k < n[r]; ++k) {
                const int64_t i = img[(size_t)r] + k;
                tab[(size_t)i] = rq_image{e_off[(size_t)r] + (int64_t)k * d[(size_t)r], d[(size_t)r], 0};
                if (fstat[(size_t)i] != ICL_OK && req_st[(size_t)r] == ICL_OK) req_st[(size_t)r] = fstat[(size_t)i];
            }
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_tab, tab.data(), tab.size() * sizeof(rq_image), hipMemcpyHostToDevice, st));
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_loff, label_off, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, st));
        if (nlab) ICL_HIP(ctx, hipMemcpyAsync(ws + o_lidx, label_idx, (size_t)nlab * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(requests_assemble_kernel, dim3((unsigned)rows), dim3(256), 0, st, (const float *)d_dense, head, (const rq_image *)(ws + o_tab),
                           (const int64_t *)(ws + o_loff), (const int32_t *)(ws + o_lidx), d_E);
        ICL_HIP(ctx, hipGetLastError());
        ICL_HIP(ctx, hipStreamSynchronize(st)); // tab is a local; the caller's label arrays are pageable memory
    }
    ICL_HIP(ctx, hipEventRecord(ev[2], st));

    // ---- clustering: the requests whose files were all read, as problems of icl_cluster_many_dev ----
    std::vector<int32_t> live;
    for (int32_t r = 0; r < nreq; ++r)
        if (req_st[(size_t)r] == ICL_OK) live.push_back(r);
    const int32_t np = (int32_t)live.size();
    std::vector<int64_t> p_off((size_t)np);
    std::vector<int32_t> p_n((size_t)np), p_d((size_t)np), p_min((size_t)np), p_max((size_t)np), p_nc((size_t)np, 0), p_nm((size_t)np, 0), p_st((size_t)np, ICL_OK);
    int64_t p_rows = 0;
    for (int32_t p = 0; p < np; ++p) {
        const int32_t r = live[(size_t)p];
        p_off[(size_t)p] = e_off[(size_t)r];
        p_n[(size_t)p] = n[r];
        p_d[(size_t)p] = d[(size_t)r];
        p_min[(size_t)p] = min_size[r];
        p_max[(size_t)p] = max_size[r];
        p_rows += n[r];
    }
    std::vector<int32_t> p_cid((size_t)std::max<int64_t>(p_rows, 1), -1), p_rank((size_t)std::max<int64_t>(p_rows, 1), -1), p_mg;
    if (merges) p_mg.assign((size_t)std::max<int64_t>(2 * p_rows, 1), 0);
    icl_item_failure bad_prob; // the lowest failed problem, i.e. the lowest request that failed in the clustering
    ctx->many_stats[0] = ctx->many_stats[1] = ctx->many_stats[2] = ctx->many_stats[3] = 0;
    if (np) {
        const int rc = cluster_many_locked(ctx, np, d_E, nullptr, e_len, p_off.data(), p_n.data(), p_d.data(), p_min.data(), p_max.data(), p_cid.data(),
                                           p_rank.data(), p_nc.data(), p_nm.data(), merges ? p_mg.data() : nullptr, p_st.data(), &bad_prob);
        if (rc != ICL_OK && bad_prob.index < 0) return rc; // not a problem's failure: the launches themselves failed
    }
    ICL_HIP(ctx, hipEventRecord(ev[3], st));
    ICL_HIP(ctx, hipStreamSynchronize(st));
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) ICL_HIP(ctx, hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
    for (int k = 0; k < 3; ++k) ctx->requests_ms[k] = ms[k];
    if (E_out && e_len) ICL_HIP(ctx, hipMemcpy(E_out, d_E, (size_t)e_len * 4, hipMemcpyDeviceToHost));

    // ---- results in request order ----
    int64_t from = 0; // first image of live request p in the compacted outputs
    for (int32_t r = 0, p = 0; r < nreq; ++r) {
        int32_t *cid = cluster_id + img[(size_t)r], *rank = member_rank + img[(size_t)r];
        if (req_st[(size_t)r] != ICL_OK) {
            std::fill(cid, cid + n[r], -1);
            std::fill(rank, rank + n[r], -1);
            n_clusters[r] = n_merges[r] = 0;
            status[r] = req_st[(size_t)r];
            continue;
        }
        if (n[r]) {
            memcpy(cid, p_cid.data() + from, 4 * (size_t)n[r]);
            memcpy(rank, p_rank.data() + from, 4 * (size_t)n[r]);
        }
        n_clusters[r] = p_nc[(size_t)p];
        n_merges[r] = p_nm[(size_t)p];
        if (merges && p_nm[(size_t)p]) memcpy(merges + 2 * img[(size_t)r], p_mg.data() + 2 * from, 8 * (size_t)p_nm[(size_t)p]);
        status[r] = p_st[(size_t)p];
        from += n[r];
        ++p;
    }
    if (file_status && rows) memcpy(file_status, fstat.data(), 4 * (size_t)rows);
    // the lowest failed request: a file failure there is the call's lowest failed file (a lower one would have failed a lower request),
    // a clustering failure the lowest failed problem (the live requests keep their order)
    for (int32_t r = 0; r < nreq; ++r) {
        if (status[r] == ICL_OK) continue;
        if (req_st[(size_t)r] != ICL_OK)
            return icl_fail(ctx, status[r], "%s: request %d: file %lld of %lld: %s", what, r, (long long)bad_file.index, (long long)rows, bad_file.why.c_str());
        return icl_fail(ctx, status[r], "%s: request %d: %s", what, r, bad_prob.why.c_str());
    }
    return ICL_OK;
}

// both entry points (imgs: the caller's arrays; its n is found by the argument check)
static int cluster_requests(icl_ctx *ctx, const char *what, int32_t nreq, ingest_list &imgs, const int32_t *n,
                            const int32_t *n_labels, const int64_t *label_off, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size, int head,
                            int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges,
                            int32_t *status, int32_t *file_status, float *E_out)
{
    return no_throw(ctx, what, [&]() -> int {
        ICL_TRY(rq_check_args(ctx, what, nreq, imgs, n, n_labels, label_off, label_idx, min_size, max_size, head, prec, threads, cluster_id,
                              member_rank, n_clusters, n_merges, status));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (!ctx->model) return icl_fail(ctx, ICL_ERR_NOMODEL, "no model loaded (call icl_model_load_* first)");
        icl_ingest_stats_reset(ctx);
        ctx->many_stats[0] = ctx->many_stats[1] = ctx->many_stats[2] = ctx->many_stats[3] = 0;
        ctx->requests_ms[0] = ctx->requests_ms[1] = ctx->requests_ms[2] = 0;
        if (nreq == 0) return ICL_OK;
        const std::vector<ingest_src> srcs = imgs.srcs();
        return cluster_requests_locked(ctx, what, nreq, srcs.data(), n, n_labels, label_off, label_idx, min_size, max_size, head, prec, threads, cluster_id,
                                       member_rank, n_clusters, n_merges, merges, status, file_status, E_out);
    });
}

extern "C" int icl_cluster_requests(icl_ctx *ctx, int32_t nreq, const char *const *paths, const int32_t *n, const int32_t *n_labels,
                                    const int64_t *label_off, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size, int head,
                                    int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges,
                                    int32_t *merges, int32_t *status, int32_t *file_status, float *E_out)
{
    ingest_list imgs = ingest_list::files(paths, 0);
    return cluster_requests(ctx, "icl_cluster_requests", nreq, imgs, n, n_labels, label_off, label_idx, min_size, max_size, head, prec, threads,
                            cluster_id, member_rank, n_clusters, n_merges, merges, status, file_status, E_out);
}

extern "C" int icl_cluster_requests_mem(icl_ctx *ctx, int32_t nreq, const uint8_t *const *data, const int64_t *bytes, const int32_t *n, const int32_t *n_labels,
                                        const int64_t *label_off, const int32_t *label_idx, const int32_t *min_size, const int32_t *max_size, int head,
                                        int prec, int32_t threads, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges,
                                        int32_t *merges, int32_t *status, int32_t *file_status, float *E_out)
{
    ingest_list imgs = ingest_list::memory(data, bytes, 0);
    return cluster_requests(ctx, "icl_cluster_requests_mem", nreq, imgs, n, n_labels, label_off, label_idx, min_size, max_size, head, prec, threads,
                            cluster_id, member_rank, n_clusters, n_merges, merges, status, file_status, E_out);
}

extern "C" int icl_last_requests_ms(icl_ctx *ctx, double *embed_ms, double *assemble_ms, double *cluster_ms)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_requests_ms: null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (embed_ms) *embed_ms = ctx->requests_ms[0];
    if (assemble_ms) *assemble_ms = ctx->requests_ms[1];
    if (cluster_ms) *cluster_ms = ctx->requests_ms[2];
    return ICL_OK;
}
