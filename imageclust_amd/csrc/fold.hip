// fold.hip -- icl_fold_centroids: the centroid of every cluster given as a member list, MergeClusters (clustering.go:29-47) folded over
// the members in list order (DESIGN.md "Editing a held clustering").
//
// Values are ward_value.h's ward_merge_elem, one rounded product, product, sum and quotient per member and column, the running item
// total kept as an integer and converted for each step.  The fold is not associative, so a group's chain is never cut along the member
// axis: a workgroup is one group x one chunk of columns (fold_plan.h), a thread owns one column or four consecutive ones and carries
// their chains in registers.  Every output element is one fixed expression tree: no geometry changes a bit.
// It is a gather-bound stream -- every member row is read once, every output row written once.  The loads of a row do not depend on
// the chain, so FOLD_BATCH rows are requested before the first of their steps runs; the members' indices and sizes come from LDS,
// FOLD_STAGE at a time, read from global memory once per workgroup.  Plain vector stores only: no atomics, no flags, nothing that has
// to be co-resident.
// Compiled with -ffp-contract=off -fno-slp-vectorize like ward_many.hip: every product, sum and quotient is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"

#include "fold_plan.h"
#include "ward_value.h"

template <int PER> struct fold_row {
    float v[PER];
};

template <int PER> __device__ __forceinline__ fold_row<PER> fold_load(const float *__restrict__ p)
{
    fold_row<PER> r;
    if constexpr (PER == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p); // (d % 4 == 0, E 16-byte aligned: fold_geom::vec)
        r.v[0] = q.x;
        r.v[1] = q.y;
        r.v[2] = q.z;
        r.v[3] = q.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int PER> __device__ __forceinline__ void fold_store(float *__restrict__ p, const fold_row<PER> &r)
{
    if constexpr (PER == 4)
        *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else
        *p = r.v[0];
}

// One batch: the rows s_idx[t0 .. t0 + nb) are requested, then their steps run in member order.  FULL: nb == FOLD_BATCH, no tests
// between the loads.  first: member t0 opens the group -- its row is copied, not merged with anything.
template <int PER, bool FULL>
__device__ __forceinline__ void fold_batch(const float *__restrict__ E, int64_t d, int64_t col, const int32_t *s_idx, const int32_t *s_sz, int t0, int nb,
                                           bool first, fold_row<PER> &c, int32_t &S)
{
    fold_row<PER> row[FOLD_BATCH];
#pragma unroll
    for (int q = 0; q < FOLD_BATCH; ++q)
        if (FULL || q < nb) row[q] = fold_load<PER>(E + (int64_t)s_idx[t0 + q] * d + col);
#pragma unroll
    for (int q = 0; q < FOLD_BATCH; ++q) {
        if (!FULL && q >= nb) break;
        const int32_t s = s_sz[t0 + q];
        if (q == 0 && first) {
            c = row[0];
            S = s;
            continue;
        }
        const float fa = (float)S, fb = (float)s;
        S += s; // (at most INT32_MAX: fold_bad_arg)
        const float fs = (float)S;
#pragma unroll
        for (int e = 0; e < PER; ++e) c.v[e] = ward_merge_elem(fa, c.v[e], fb, row[q].v[e], fs);
    }
}

// msize[p]: the item count of member[p] (null: all 1).  blocks = K * chunks; workgroup b takes group b / chunks and the columns of chunk
// b % chunks, and goes on with block b + gridDim.x.
template <int PER>
__global__ __launch_bounds__(FOLD_THREADS) void fold_kernel(const float *__restrict__ E, int32_t d, const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ member, const int32_t *__restrict__ msize, int64_t blocks,
                                                           int64_t chunks, float *__restrict__ C)
{
    __shared__ int32_t s_idx[FOLD_STAGE];
    __shared__ int32_t s_sz[FOLD_STAGE];
    for (int64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const int64_t g = b / chunks;
        const int64_t col = ((b - g * chunks) * blockDim.x + threadIdx.x) * PER;
        const bool live = col < d; // (PER == 4: d % 4 == 0, so the four columns are inside together)
        const int64_t p0 = row_ptr[g], p1 = row_ptr[g + 1];
        fold_row<PER> c;
#pragma unroll
        for (int e = 0; e < PER; ++e) c.v[e] = 0.0f; // an empty group: +0.0
        int32_t S = 0;
        for (int64_t ps = p0; ps < p1; ps += FOLD_STAGE) {
            const int ns = (int)(p1 - ps < FOLD_STAGE ? p1 - ps : FOLD_STAGE);
            __syncthreads(); // the readers of the stage before this one have left it
            for (int j = threadIdx.x; j < ns; j += blockDim.x) {
                s_idx[j] = member[ps + j];
                s_sz[j] = msize ? msize[ps + j] : 1;
            }
            __syncthreads();
            if (!live) continue; // (it keeps meeting the barriers)
            int t0 = 0;
            for (; t0 + FOLD_BATCH <= ns; t0 += FOLD_BATCH) fold_batch<PER, true>(E, d, col, s_idx, s_sz, t0, FOLD_BATCH, ps == p0 && t0 == 0, c, S);
            if (t0 < ns) fold_batch<PER, false>(E, d, col, s_idx, s_sz, t0, ns - t0, ps == p0 && t0 == 0, c, S);
        }
        if (live) fold_store<PER>(C + g * (int64_t)d + col, c);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int fold_check(icl_ctx *ctx, const char *what, const void *E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr,
                      const int32_t *member, int64_t K, const void *C_out, int64_t *rows, int64_t *longest)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    if (const char *why = fold_bad_arg(E, size, n, d, row_ptr, member, K, C_out, rows, longest)) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

// ctx->mu held, the device selected, the arguments checked, K > 0.
static int fold_dev_locked(icl_ctx *ctx, const float *d_E, const int32_t *size, int32_t d, const int64_t *row_ptr, const int32_t *member, int64_t K,
                           float *d_C, int64_t rows, int64_t longest)
{
    std::vector<int32_t> msize; // the members' item counts, in member order: the kernel reads them beside the indices
    if (size && rows) {
        msize.resize((size_t)rows);
        for (int64_t p = 0; p < rows; ++p) msize[(size_t)p] = size[member[p]];
    }
    icl_ws_upload up; // [row_ptr] [member] [member sizes], each on a 16-byte boundary
    const size_t o_rp = up.add((const int32_t *)row_ptr, 2 * (K + 1)), o_mb = up.add(member, rows);
    const size_t o_ms = up.add(msize.empty() ? nullptr : msize.data(), rows), need = up.L.total;
    ICL_TRY(ctx->fold.ensure(ctx, need, "icl_fold_centroids: workspace"));
    char *ws = ctx->fold.as<char>();
    ICL_TRY(up.go(ctx, ws, need));
    const bool aligned = ((uintptr_t)d_E | (uintptr_t)d_C) % 16 == 0;
    const fold_geom g = fold_geometry(K, d, aligned, ctx->prop.multiProcessorCount);
    const int64_t *rp = (const int64_t *)(ws + o_rp);
    const int32_t *mb = (const int32_t *)(ws + o_mb), *ms = msize.empty() ? nullptr : (const int32_t *)(ws + o_ms);
    if (g.vec)
        hipLaunchKernelGGL(fold_kernel<4>, dim3((unsigned)g.grid), dim3((unsigned)g.threads), 0, ctx->stream, d_E, d, rp, mb, ms, g.blocks, g.chunks, d_C);
    else
        hipLaunchKernelGGL(fold_kernel<1>, dim3((unsigned)g.grid), dim3((unsigned)g.threads), 0, ctx->stream, d_E, d, rp, mb, ms, g.blocks, g.chunks, d_C);
    ICL_HIP(ctx, hipGetLastError());
    ctx->fold_stats[0] = K;
    ctx->fold_stats[1] = rows;
    ctx->fold_stats[2] = longest;
    ctx->fold_stats[3] = (int64_t)need;
    return ICL_OK;
}

extern "C" int icl_fold_centroids_dev(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr,
                                      const int32_t *member, int64_t K, float *d_C_out, int32_t *size_out)
{
    return no_throw(ctx, "icl_fold_centroids_dev", [&]() -> int {
        int64_t rows = 0, longest = 0;
        ICL_TRY(fold_check(ctx, "icl_fold_centroids_dev", d_E, size, n, d, row_ptr, member, K, d_C_out, &rows, &longest));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->fold_stats) s = 0;
        if (K == 0) return ICL_OK;
        ICL_TRY(fold_dev_locked(ctx, d_E, size, d, row_ptr, member, K, d_C_out, rows, longest));
        if (size_out) fold_totals(size, row_ptr, member, K, size_out);
        return ICL_OK;
    });
}

extern "C" int icl_fold_centroids(icl_ctx *ctx, const float *E, const int32_t *size, int64_t n, int32_t d, const int64_t *row_ptr,
                                  const int32_t *member, int64_t K, float *C_out, int32_t *size_out)
{
    return no_throw(ctx, "icl_fold_centroids", [&]() -> int {
        int64_t rows = 0, longest = 0;
        ICL_TRY(fold_check(ctx, "icl_fold_centroids", E, size, n, d, row_ptr, member, K, C_out, &rows, &longest));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->fold_stats) s = 0;
        if (K == 0) return ICL_OK;
        dev_guard dE, dC;
        const size_t bc = (size_t)K * d * 4;
        // (no member: no row is read, and E may be null)
        ICL_TRY(rows ? icl_dev_upload(ctx, dE, E, (size_t)n * d * 4, "icl_fold_centroids: E") : icl_dev_alloc(ctx, dE, 16, "icl_fold_centroids: E"));
        ICL_TRY(icl_dev_alloc(ctx, dC, bc, "icl_fold_centroids: C_out"));
        ICL_TRY(fold_dev_locked(ctx, dE.as<float>(), size, d, row_ptr, member, K, dC.as<float>(), rows, longest));
        ICL_HIP(ctx, hipMemcpyAsync(C_out, dC.p, bc, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (size_out) fold_totals(size, row_ptr, member, K, size_out);
        return ICL_OK;
    });
}

extern "C" int icl_last_fold_stats(icl_ctx *ctx, int64_t info[4])
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_fold_stats: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < 4; ++q) info[q] = ctx->fold_stats[q];
    return ICL_OK;
}
