// nearest.hip -- icl_nearest: for each query row the k library rows of smallest WardDistance, exact, with no distance matrix.
//
// Values are the reference's (clustering.go:136-157; ward_value.h), from the exact tile ward_dist_exact_kernel (ward.hip) runs, here on
// a rectangle (ward_exact_tile.h).  The walk over bands of 128 query rows, its LDS layout and its launch are band_select.h's; this unit
// supplies the walk's policy (a row skips its excluded column), the kernel that joins the column splits' partial lists, and the entry
// points.  What a list keeps and in which order is decided by nearest_select.h alone, on the host (icl_nearest_from_matrix) as on the
// device.
// Compiled with -ffp-contract=off -fno-slp-vectorize like ward.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "band_select.h"

#define NR_MERGE_ROWS 64

struct nr_args : band_args { // sel: exclude (null: none)
    float *val;
    int32_t *idx;
};

struct nr_policy {
    using args = nr_args;
    static __device__ __forceinline__ void band_start(const args &, int64_t, int64_t, int64_t) {}
    static __device__ __forceinline__ int items(int32_t e_size) { return e_size; }
    static __device__ __forceinline__ int64_t row_key(const args &a, int64_t i) { return a.sel ? (int64_t)a.sel[i] : -1; }
    static __device__ __forceinline__ int64_t quarter_key(const args &, int64_t, int64_t ex, int64_t, int, const float *, int) { return ex; }
    static __device__ __forceinline__ bool left_out(int64_t j, int, int64_t ex, int q_size, int32_t e_size, int32_t max_size)
    {
        return ns_left_out(j, ex, q_size, e_size, max_size);
    }
};

// Joins the splits' partial lists of each row by the shared rule.  One lane per row, the row's list in LDS.  A partial list is
// ascending, so the first of its entries the list refuses ends it.
__global__ __launch_bounds__(NR_MERGE_ROWS) void nearest_merge_kernel(const float *__restrict__ pv, const int32_t *__restrict__ pj, int64_t nq,
                                                                      int k, int splits, float *__restrict__ val, int32_t *__restrict__ idx)
{
    extern __shared__ __attribute__((aligned(16))) float nr_smem[];
    const int ks = k | 1;
    float *rv = nr_smem + threadIdx.x * ks;
    int32_t *rj = reinterpret_cast<int32_t *>(nr_smem + NR_MERGE_ROWS * ks) + threadIdx.x * ks;
    const int64_t i = (int64_t)blockIdx.x * NR_MERGE_ROWS + threadIdx.x;
    if (i >= nq) return;
    int c = 0;
    for (int s = 0; s < splits; ++s) {
        const float *sv = pv + ((int64_t)s * nq + i) * k;
        const int32_t *sj = pj + ((int64_t)s * nq + i) * k;
        for (int p = 0; p < k; ++p) {
            const int32_t j = sj[p];
            if (j < 0 || !ns_insert(rv, rj, k, c, sv[p], j)) break;
        }
    }
    ns_fill_tail(rv, rj, k, c);
    for (int p = 0; p < k; ++p) {
        val[i * k + p] = rv[p];
        idx[i * k + p] = rj[p];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// What ICL_ERR_ARG covers apart from the pointers: the reason, or nullptr.
static const char *nr_bad_arg(int64_t nq, int64_t n, int32_t k, const int32_t *q_size, const int32_t *e_size, const int64_t *exclude)
{
    if (nq < 0 || n < 0) return "negative nq or n";
    if (n >= (1LL << 31)) return "n must be below 2^31";
    if (k < 1 || k > NS_KMAX) return "k must be 1 .. 64";
    for (int64_t i = 0; q_size && i < nq; ++i)
        if (q_size[i] <= 0) return "a q_size entry is not above 0";
    for (int64_t j = 0; e_size && j < n; ++j)
        if (e_size[j] <= 0) return "an e_size entry is not above 0";
    for (int64_t i = 0; exclude && i < nq; ++i)
        if (exclude[i] < -1 || exclude[i] >= n) return "an exclude entry is outside [-1, n)";
    return nullptr;
}

// The merge of every band walk's partial lists (band_plan::run): the kernel has its one definition here.
int nearest_merge_launch(icl_ctx *ctx, const float *d_pv, const int32_t *d_pj, int64_t nq, int k, int splits, float *d_val, int32_t *d_idx)
{
    hipLaunchKernelGGL(nearest_merge_kernel, dim3((unsigned)icl_ceil_div(nq, NR_MERGE_ROWS)), dim3(NR_MERGE_ROWS),
                       (size_t)2 * NR_MERGE_ROWS * (k | 1) * 4, ctx->stream, d_pv, d_pj, nq, k, splits, d_val, d_idx);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

// ctx->mu held, the device selected, the arguments checked, nq > 0.
static int nearest_dev_locked(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size,
                              int64_t n, int32_t d, int32_t k, int32_t max_size, const int64_t *exclude, int32_t *d_idx, float *d_val)
{
    band_plan plan;
    ICL_TRY(plan.decide(ctx, "icl_nearest", nq, n, k));
    std::vector<int32_t> ex32(exclude, exclude + (exclude ? nq : 0)); // (n < 2^31)
    // [q_size] [e_size] [exclude] [partial values] [partial indices], each on a 16-byte boundary; the first three go up in one copy
    icl_ws_upload up;
    const size_t o_qs = up.add(q_size, nq), o_es = up.add(e_size, n), o_ex = up.add(exclude ? ex32.data() : nullptr, nq), b_meta = up.L.total;
    const size_t o_val = up.L.take(plan.part_bytes), o_idx = up.L.take(plan.part_bytes), need = up.L.total;
    if (need) ICL_TRY(ctx->nearest.ensure(ctx, need, "icl_nearest: workspace"));
    char *ws = ctx->nearest.as<char>(); // (used only where need > 0)
    ICL_TRY(up.go(ctx, ws, b_meta));
    nr_args a;
    a.Q = d_Q;
    a.E = d_E;
    a.qs = q_size ? (const int32_t *)(ws + o_qs) : nullptr;
    a.es = e_size ? (const int32_t *)(ws + o_es) : nullptr;
    a.sel = exclude ? (const int32_t *)(ws + o_ex) : nullptr;
    a.nq = nq;
    a.n = n;
    a.d = d;
    a.k = k;
    a.max_size = max_size;
    ICL_TRY(plan.run<nr_policy>(ctx, a, (float *)(ws + o_val), (int32_t *)(ws + o_idx), d_val, d_idx));
    ctx->nearest_stats[0] = plan.splits;
    ctx->nearest_stats[1] = plan.nbands * plan.ntiles;
    ctx->nearest_stats[2] = nq * n;
    ctx->nearest_stats[3] = (int64_t)need;
    return ICL_OK;
}

static int nearest_check(icl_ctx *ctx, const char *what, const void *Q, const int32_t *q_size, int64_t nq, const void *E, const int32_t *e_size,
                         int64_t n, int32_t d, int32_t k, const int64_t *exclude, const void *idx, const void *val)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : nr_bad_arg(nq, n, k, q_size, e_size, exclude);
    if (!why && ((nq > 0 && (!Q || !idx || !val)) || (n > 0 && !E))) why = "a null pointer";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

extern "C" int icl_nearest_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size,
                               int64_t n, int32_t d, int32_t k, int32_t max_size, const int64_t *exclude, int32_t *d_idx, float *d_val)
{
    return no_throw(ctx, "icl_nearest_dev", [&]() -> int {
        ICL_TRY(nearest_check(ctx, "icl_nearest_dev", d_Q, q_size, nq, d_E, e_size, n, d, k, exclude, d_idx, d_val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->nearest_stats) s = 0;
        if (nq == 0) return ICL_OK;
        return nearest_dev_locked(ctx, d_Q, q_size, nq, d_E, e_size, n, d, k, max_size, exclude, d_idx, d_val);
    });
}

extern "C" int icl_nearest(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *E, const int32_t *e_size, int64_t n,
                           int32_t d, int32_t k, int32_t max_size, const int64_t *exclude, int32_t *idx, float *val)
{
    return no_throw(ctx, "icl_nearest", [&]() -> int {
        ICL_TRY(nearest_check(ctx, "icl_nearest", Q, q_size, nq, E, e_size, n, d, k, exclude, idx, val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->nearest_stats) s = 0;
        if (nq == 0) return ICL_OK;
        dev_guard dQ, dE, dI, dV;
        const size_t bq = (size_t)nq * d * 4, be = (size_t)n * d * 4, bo = (size_t)nq * k * 4;
        ICL_TRY(icl_dev_upload(ctx, dQ, Q, bq, "icl_nearest: Q"));
        if (n) ICL_TRY(icl_dev_upload(ctx, dE, E, be, "icl_nearest: E"));
        ICL_TRY(icl_dev_alloc(ctx, dI, bo, "icl_nearest: idx"));
        ICL_TRY(icl_dev_alloc(ctx, dV, bo, "icl_nearest: val"));
        ICL_TRY(nearest_dev_locked(ctx, (const float *)dQ.p, q_size, nq, (const float *)dE.p, e_size, n, d, k, max_size, exclude, (int32_t *)dI.p,
                                   (float *)dV.p));
        ICL_HIP(ctx, hipMemcpyAsync(idx, dI.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(val, dV.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    });
}

extern "C" int icl_nearest_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, const int32_t *q_size, const int32_t *e_size, int32_t k,
                                       int32_t max_size, const int64_t *exclude, int32_t *idx, float *val)
{
    if (nr_bad_arg(nq, n, k, q_size, e_size, exclude) || ld < n || (nq > 0 && (!idx || !val)) || (nq > 0 && n > 0 && !D)) return ICL_ERR_ARG;
    for (int64_t i = 0; i < nq; ++i) {
        float *rv = val + i * k;
        int32_t *rj = idx + i * k;
        const int64_t ex = exclude ? exclude[i] : -1, sq = q_size ? q_size[i] : 1;
        int c = 0;
        for (int64_t j = 0; j < n; ++j)
            if (!ns_left_out(j, ex, sq, e_size ? e_size[j] : 1, max_size)) ns_insert(rv, rj, k, c, D[i * ld + j], (int32_t)j);
        ns_fill_tail(rv, rj, k, c);
    }
    return ICL_OK;
}

extern "C" int icl_set_nearest_options(icl_ctx *ctx, int32_t column_splits)
{
    if (!ctx || column_splits < 0) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_nearest_options: column_splits must be 0 (the engine decides) or above");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->nearest_splits = column_splits;
    return ICL_OK;
}

extern "C" int icl_last_nearest_stats(icl_ctx *ctx, int64_t info[4])
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_nearest_stats: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < 4; ++q) info[q] = ctx->nearest_stats[q];
    return ICL_OK;
}
