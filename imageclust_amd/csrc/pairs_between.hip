// pairs_between.hip -- icl_pairs_between: every pair (query row, library row) whose WardDistance is at most a threshold, exact and
// complete, as a CSR list over the queries, with no distance matrix and no cap on a query's partners.
//
// Values are icl_nearest's bit for bit: the exact tile (ward_exact_tile.h) on the rectangle, then ward_scale (ward_value.h).  Which pairs
// are listed is decided by ps_listed_between (pairs_select.h) alone, on the host (icl_pairs_between_from_matrix) as on the device.
//
// GEOMETRY: the band walk's (band_select.h), for both passes.  A workgroup is (band of 128 query rows, split s) and walks the library's
// 128-column tiles  s * ntiles / splits .. (s + 1) * ntiles / splits,  indexed as in band_select_kernel -- band = block % nbands,
// split = block / nbands -- so the bands that run together read the same library tiles at about the same time.  splits comes from
// band_splits() (band_plan.h), and icl_set_nearest_options' forced count applies here as it does to icl_nearest.  A split is a column
// RANGE and the ranges are taken in ascending order: that is what makes a row's segments, laid end to end, ascending in j.
//
// One walk body (pairs_between_kernel<FILL>), two epilogues:
//   COUNT  per tile: the exact tile, the rule, the hits added to 128 per-row counters in LDS, and the tile's flag byte
//          hit[band * ntiles + t] = 0 or 1.  After the walk seg_count[i * splits + s] is stored for the band's rows.  Every flag and every
//          count has exactly one writer in the launch -- tile t of a band belongs to one split, row i of split s to one workgroup -- so
//          the stores are plain: no global atomic, and no memset of the count area.
//   PREFIX on the host over the nq * splits counts in (i, s) order (pb_prefix, pairs_between_plan.h): seg_ptr, row_ptr, *total and the
//          capacity decision.
//   FILL   the same geometry, launched only for the (band, split) pairs that counted a hit.  It walks the segment's flagged tiles in
//          ascending t, recomputes each and writes every hit at  seg_ptr[i * splits + s] + (the row's hits in the segment's tiles already
//          walked) + (its hits of lower j in this tile, from a 128-bit mask per row in LDS: pb_mask_rank).  No atomic decides a place
//          and nothing is sorted.
// Compiled with nearest.o's flags (-ffp-contract=off -fno-slp-vectorize): every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"
#include "band_plan.h"
#include "pairs_between_plan.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile
#include "ward_value.h"

#include <algorithm>
#include <vector>

static_assert(PB_ROWS == DT_TILE, "pairs_between_plan.h's masks are worked out for the exact tile's 128 columns");

struct pb_args {
    const float *Q, *L;
    const int32_t *qs, *ls, *ex; // device copies of the row sizes, the column sizes and exclude (each may be null: all 1 / none)
    int64_t nq, n;
    int d, vec;
    float thr;
    int64_t ntiles, nbands;
    int splits;
    int32_t *seg_count;     // [nq * splits]   count pass: hits of row i in split s's tiles
    uint8_t *hit;           // [nbands * ntiles]   count pass: tile t of the band had a hit
    const int32_t *work;    // fill pass: the workgroups of the count pass's grid that counted a hit, ascending
    const int64_t *seg_ptr; // [nq * splits + 1]   fill pass
    int32_t *col;
    float *val;
};

// row / column of accumulator index a (0..7) of thread coordinate t (ty / tx), as ward_exact_tile.h lays them out
__device__ __forceinline__ int pb_lane_index(int a, int t) { return a < 4 ? t * 4 + a : 64 + t * 4 + (a - 4); }

template <bool FILL> static __global__ __launch_bounds__(256) void pairs_between_kernel(pb_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ int32_t cnt[DT_TILE]; // the row's hits in the tiles walked so far
    __shared__ int32_t qsz[DT_TILE], esz[DT_TILE], exc[DT_TILE];
    __shared__ uint32_t mask[FILL ? DT_TILE : 1][4]; // the tile's hits: bit c of row r's 128
    __shared__ int64_t sbase[FILL ? DT_TILE : 1];    // seg_ptr of the row's segment
    __shared__ int32_t slen[FILL ? DT_TILE : 1];     // the segment's hits in all (the count pass's figure: no place beyond it is ever written)

    // workgroups of one split are neighbours: the bands that run together read the same library tiles at about the same time
    const int64_t block = FILL ? (int64_t)a.work[blockIdx.x] : (int64_t)blockIdx.x;
    const int64_t band = block % a.nbands, split = block / a.nbands;
    const int64_t t_lo = split * a.ntiles / a.splits, t_hi = (split + 1) * a.ntiles / a.splits;
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    if (tid < DT_TILE) {
        const int64_t i = i0 + tid;
        cnt[tid] = 0;
        qsz[tid] = (a.qs && i < a.nq) ? a.qs[i] : 1;
        exc[tid] = (a.ex && i < a.nq) ? a.ex[i] : -1;
        if (FILL) {
            const int64_t sg = i * a.splits + split;
            sbase[tid] = i < a.nq ? a.seg_ptr[sg] : 0;
            slen[tid] = i < a.nq ? (int32_t)(a.seg_ptr[sg + 1] - a.seg_ptr[sg]) : 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) mask[tid][w] = 0;
        }
    }
    __syncthreads();

    for (int64_t t = t_lo; t < t_hi; ++t) {
        if (FILL && !a.hit[band * a.ntiles + t]) continue; // (the same answer in every thread)
        const int64_t j0 = t * DT_TILE;
        if (tid < DT_TILE) esz[tid] = (a.ls && j0 + tid < a.n) ? a.ls[j0 + tid] : 1; // (read after the tile's barriers)

        float acc[8][8];
        ward_exact_tile(a.Q, a.nq, i0, a.L, a.n, j0, a.d, a.vec != 0, As, Bs, acc);

        // Padded rows and columns (i >= nq, j >= n) are never offered.
        if (!FILL) {
            int any = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = pb_lane_index(r, ty);
                if (i0 + row >= a.nq) continue;
                const int sa = qsz[row];
                const int64_t ex = exc[row];
                int c = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int cl = pb_lane_index(q, tx);
                    const int64_t j = j0 + cl;
                    if (j >= a.n) continue;
                    c += ps_listed_between(j, ex, ward_scale(acc[r][q], sa, esz[cl]), a.thr) ? 1 : 0;
                }
                if (c) {
                    atomicAdd(&cnt[row], c); // (LDS; integer sums do not depend on order)
                    any = 1;
                }
            }
            const int some = __syncthreads_or(any); // (also stands between this tile's readers of esz and the next tile's writers)
            if (tid == 0) a.hit[band * a.ntiles + t] = some ? 1 : 0;
        } else {
            // the count pass's test again, into the rows' masks
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = pb_lane_index(r, ty);
                if (i0 + row >= a.nq) continue;
                const int sa = qsz[row];
                const int64_t ex = exc[row];
#pragma unroll
                for (int bh = 0; bh < 2; ++bh) {
                    uint32_t nib = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cl = bh * 64 + tx * 4 + q;
                        const int64_t j = j0 + cl;
                        if (j < a.n && ps_listed_between(j, ex, ward_scale(acc[r][bh * 4 + q], sa, esz[cl]), a.thr)) nib |= 1u << q;
                    }
                    if (nib) atomicOr(&mask[row][bh * 2 + (tx >> 3)], nib << ((tx & 7) * 4));
                }
            }
            __syncthreads();
            // a hit's place: behind the row's hits of the segment's tiles walked before, and behind its hits of lower j in this tile
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = pb_lane_index(r, ty);
                const uint32_t m[4] = {mask[row][0], mask[row][1], mask[row][2], mask[row][3]};
                if (!(m[0] | m[1] | m[2] | m[3])) continue;
                const int sa = qsz[row];
                const int c0 = cnt[row], len = slen[row];
                const int64_t sb = sbase[row];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int cl = pb_lane_index(q, tx);
                    if (!((m[cl >> 5] >> (cl & 31)) & 1u)) continue;
                    const int p = c0 + pb_mask_rank(m, cl);
                    if (p < len) {
                        a.col[sb + p] = (int32_t)(j0 + cl);
                        a.val[sb + p] = ward_scale(acc[r][q], sa, esz[cl]);
                    }
                }
            }
            __syncthreads();
            if (tid < DT_TILE) {
                int c = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    c += __popc(mask[tid][w]);
                    mask[tid][w] = 0;
                }
                cnt[tid] += c;
            }
            // (the next tile's barriers stand between this update and its readers)
        }
    }

    if (!FILL) {
        __syncthreads();
        const int64_t i = i0 + tid;
        if (tid < DT_TILE && i < a.nq) a.seg_count[i * a.splits + split] = cnt[tid];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct pb_plan { // one call's geometry and where the workspace's parts are
    pb_args a;
    int64_t nbands = 0, ntiles = 0, fill_pairs = 0; // fill_pairs: the pairs i < nq, j < n of the tiles with a hit
    int splits = 0;
    size_t need = 0;
    char *d_seg_ptr = nullptr, *d_work = nullptr;
    std::vector<int64_t> seg_ptr; // [nq * splits + 1]
    std::vector<int32_t> work;    // the count grid's workgroups that counted a hit
};

static int pb_check(icl_ctx *ctx, const char *what, const void *Q, const int32_t *q_size, int64_t nq, const void *L, const int32_t *l_size,
                    int64_t n, int32_t d, float threshold, const int64_t *exclude, const int64_t *row_ptr, const void *col, const void *val,
                    int64_t cap, const int64_t *total)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : pb_bad_arg(nq, n, threshold, q_size, l_size, exclude, row_ptr, col, val, cap, total);
    if (!why && nq > 0 && n > 0 && (!Q || !L)) why = "a null pointer";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

// ctx->mu held: the geometry, before anything is written (a grid that does not fit one launch is a bad argument).
static int pb_decide(icl_ctx *ctx, const char *what, int64_t nq, int64_t n, pb_plan &pl)
{
    pl.nbands = icl_ceil_div(nq, DT_TILE);
    pl.ntiles = icl_ceil_div(n, DT_TILE);
    pl.splits = band_splits(ctx->nearest_splits, ctx->prop.multiProcessorCount, pl.nbands, pl.ntiles);
    if (pl.nbands * pl.splits > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_ARG, "%s: the grid does not fit a launch (nq=%lld)", what, (long long)nq);
    return ICL_OK;
}

static void pb_empty(int64_t nq, int64_t *row_ptr, int64_t *total)
{
    for (int64_t i = 0; i <= nq; ++i) row_ptr[i] = 0;
    *total = 0;
}

// ctx->mu held, the device selected, the arguments checked, the geometry decided, nq > 0 and n > 0.  Count pass and prefix: row_ptr
// and *total complete on return.
static int pb_count_locked(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_L, const int32_t *l_size, int64_t n,
                           int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int64_t *total, pb_plan &pl)
{
    const int64_t nseg = nq * pl.splits, nflag = pl.nbands * pl.ntiles, ngrid = pl.nbands * pl.splits;
    std::vector<int32_t> ex32(exclude, exclude + (exclude ? nq : 0)); // (n < 2^31)
    // [q_size] [l_size] [exclude] [seg_count] [hit] [seg_ptr] [work], each on a 16-byte boundary; the first three go up in one copy
    icl_ws_upload up;
    const size_t o_qs = up.add(q_size, nq), o_ls = up.add(l_size, n), o_ex = up.add(exclude ? ex32.data() : nullptr, nq), b_meta = up.L.total;
    const size_t o_cnt = up.L.take((size_t)nseg * 4), o_hit = up.L.take((size_t)nflag), o_ptr = up.L.take((size_t)(nseg + 1) * 8);
    const size_t o_work = up.L.take((size_t)ngrid * 4);
    pl.need = up.L.total;
    ICL_TRY(ctx->between.ensure(ctx, pl.need, "icl_pairs_between: workspace"));
    char *ws = ctx->between.as<char>();
    ICL_TRY(up.go(ctx, ws, b_meta));
    pb_args &a = pl.a;
    a.Q = d_Q;
    a.L = d_L;
    a.qs = q_size ? (const int32_t *)(ws + o_qs) : nullptr;
    a.ls = l_size ? (const int32_t *)(ws + o_ls) : nullptr;
    a.ex = exclude ? (const int32_t *)(ws + o_ex) : nullptr;
    a.nq = nq;
    a.n = n;
    a.d = d;
    a.vec = (d & 3) == 0 && (((uintptr_t)d_Q | (uintptr_t)d_L) & 15) == 0;
    a.thr = threshold;
    a.ntiles = pl.ntiles;
    a.nbands = pl.nbands;
    a.splits = pl.splits;
    a.seg_count = (int32_t *)(ws + o_cnt);
    a.hit = (uint8_t *)(ws + o_hit);
    pl.d_seg_ptr = ws + o_ptr;
    pl.d_work = ws + o_work;
    a.work = (const int32_t *)pl.d_work;
    a.seg_ptr = (const int64_t *)pl.d_seg_ptr;
    a.col = nullptr;
    a.val = nullptr;
    hipLaunchKernelGGL(pairs_between_kernel<false>, dim3((unsigned)ngrid), dim3(256), 0, ctx->stream, a);
    ICL_HIP(ctx, hipGetLastError());
    std::vector<int32_t> cnt((size_t)nseg);
    std::vector<uint8_t> hit((size_t)nflag);
    ICL_HIP(ctx, hipMemcpyAsync(cnt.data(), a.seg_count, (size_t)nseg * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(hit.data(), a.hit, (size_t)nflag, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.seg_ptr.resize((size_t)nseg + 1);
    pb_prefix(nq, pl.splits, cnt.data(), pl.seg_ptr.data(), row_ptr, total);
    // the fill pass's workgroups: (band, split) with a flagged tile, in the count grid's order
    int64_t hits = 0;
    for (int64_t s = 0; s < pl.splits; ++s)
        for (int64_t b = 0; b < pl.nbands; ++b) {
            const int64_t nr = std::min<int64_t>(DT_TILE, nq - b * DT_TILE);
            bool some = false;
            for (int64_t t = s * pl.ntiles / pl.splits; t < (s + 1) * pl.ntiles / pl.splits; ++t)
                if (hit[(size_t)(b * pl.ntiles + t)]) {
                    some = true;
                    ++hits;
                    pl.fill_pairs += nr * std::min<int64_t>(DT_TILE, n - t * DT_TILE);
                }
            if (some) pl.work.push_back((int32_t)(s * pl.nbands + b));
        }
    ctx->between_stats[0] = pl.splits;
    ctx->between_stats[1] = nflag;
    ctx->between_stats[2] = hits;
    ctx->between_stats[3] = nq * n;
    ctx->between_stats[4] = (int64_t)pl.need;
    return ICL_OK;
}

// The fill pass behind a count pass of the same call (*total > 0 entries fit d_col / d_val).  The host arrays are uploaded and done
// with at return; the kernel itself is enqueued on the context's stream.
static int pb_fill_locked(icl_ctx *ctx, pb_plan &pl, int32_t *d_col, float *d_val)
{
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_seg_ptr, pl.seg_ptr.data(), pl.seg_ptr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_work, pl.work.data(), pl.work.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.a.col = d_col;
    pl.a.val = d_val;
    hipLaunchKernelGGL(pairs_between_kernel<true>, dim3((unsigned)pl.work.size()), dim3(256), 0, ctx->stream, pl.a);
    ICL_HIP(ctx, hipGetLastError());
    ctx->between_stats[3] += pl.fill_pairs;
    return ICL_OK;
}

extern "C" int icl_pairs_between_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_L, const int32_t *l_size,
                                     int64_t n, int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *d_col, float *d_val,
                                     int64_t cap, int64_t *total)
{
    return no_throw(ctx, "icl_pairs_between_dev", [&]() -> int {
        ICL_TRY(pb_check(ctx, "icl_pairs_between_dev", d_Q, q_size, nq, d_L, l_size, n, d, threshold, exclude, row_ptr, d_col, d_val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (nq == 0 || n == 0) {
            for (int64_t &s : ctx->between_stats) s = 0;
            pb_empty(nq, row_ptr, total);
            return ICL_OK;
        }
        pb_plan pl;
        ICL_TRY(pb_decide(ctx, "icl_pairs_between_dev", nq, n, pl));
        for (int64_t &s : ctx->between_stats) s = 0;
        ICL_TRY(pb_count_locked(ctx, d_Q, q_size, nq, d_L, l_size, n, d, threshold, exclude, row_ptr, total, pl));
        if (*total > cap) {
            if (!d_col && !d_val) return ICL_OK; // the size query
            return icl_fail(ctx, ICL_ERR_ARG, "icl_pairs_between_dev: %lld pairs do not fit cap = %lld (row_ptr and total are complete)",
                            (long long)*total, (long long)cap);
        }
        if (*total == 0) return ICL_OK;
        return pb_fill_locked(ctx, pl, d_col, d_val);
    });
}

extern "C" int icl_pairs_between(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *L, const int32_t *l_size, int64_t n,
                                 int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *col, float *val, int64_t cap,
                                 int64_t *total)
{
    return no_throw(ctx, "icl_pairs_between", [&]() -> int {
        ICL_TRY(pb_check(ctx, "icl_pairs_between", Q, q_size, nq, L, l_size, n, d, threshold, exclude, row_ptr, col, val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (nq == 0 || n == 0) {
            for (int64_t &s : ctx->between_stats) s = 0;
            pb_empty(nq, row_ptr, total);
            return ICL_OK;
        }
        pb_plan pl;
        ICL_TRY(pb_decide(ctx, "icl_pairs_between", nq, n, pl));
        for (int64_t &s : ctx->between_stats) s = 0;
        dev_guard dQ, dL, dC, dV;
        ICL_TRY(icl_dev_upload(ctx, dQ, Q, (size_t)nq * d * 4, "icl_pairs_between: Q"));
        ICL_TRY(icl_dev_upload(ctx, dL, L, (size_t)n * d * 4, "icl_pairs_between: L"));
        ICL_TRY(pb_count_locked(ctx, (const float *)dQ.p, q_size, nq, (const float *)dL.p, l_size, n, d, threshold, exclude, row_ptr, total, pl));
        if (*total > cap) {
            if (!col && !val) return ICL_OK; // the size query
            return icl_fail(ctx, ICL_ERR_ARG, "icl_pairs_between: %lld pairs do not fit cap = %lld (row_ptr and total are complete)",
                            (long long)*total, (long long)cap);
        }
        if (*total == 0) return ICL_OK;
        const size_t bo = (size_t)*total * 4;
        ICL_TRY(icl_dev_alloc(ctx, dC, bo, "icl_pairs_between: col"));
        ICL_TRY(icl_dev_alloc(ctx, dV, bo, "icl_pairs_between: val"));
        ICL_TRY(pb_fill_locked(ctx, pl, (int32_t *)dC.p, (float *)dV.p));
        ICL_HIP(ctx, hipMemcpyAsync(col, dC.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(val, dV.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    });
}

extern "C" int icl_pairs_between_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, float threshold, const int64_t *exclude,
                                             int64_t *row_ptr, int32_t *col, float *val, int64_t cap, int64_t *total)
{
    return pb_from_matrix(D, nq, n, ld, threshold, exclude, row_ptr, col, val, cap, total) ? ICL_ERR_ARG : ICL_OK;
}

extern "C" int icl_last_pairs_between_stats(icl_ctx *ctx, int64_t info[5])
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_pairs_between_stats: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < 5; ++q) info[q] = ctx->between_stats[q];
    return ICL_OK;
}
