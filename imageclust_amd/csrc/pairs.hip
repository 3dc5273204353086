// pairs.hip -- icl_pairs_within: every pair of rows whose WardDistance is at most a threshold, exact and complete, as a CSR list over the
// strict lower triangle, with no distance matrix and no cap on a row's partners.
//
// Values are the reference's (clustering.go:136-157; ward_value.h) from the exact tile (ward_exact_tile.h) on the lower triangle's
// 128 x 128 tiles in dist_tile.h's band order, as ward_dist_exact_kernel (ward.hip) runs it; the epilogue is this unit's own.  Two passes:
//   COUNT  one workgroup per tile: the hits of each tile row are summed in LDS and added to row_count[i] with one integer atomic per
//          row and tile that has hits (integer sums do not depend on order); a tile with a hit sets its flag.
//   PREFIX on the host over the n counts: row_ptr, *total and the capacity decision.
//   FILL   one workgroup per TILE ROW that has a hit walks that row's flagged tiles in ascending column order, recomputes each, and
//          writes every hit at  row_ptr[i] + (hits of row i in the tiles already walked) + (hits of row i left of it in this tile),
//          the last from a 128-bit mask per row in LDS.  A row's segment is therefore ascending in j by construction: no atomic
//          decides a place and nothing is sorted.
// Which pairs are listed is decided by pairs_select.h alone, on the host (icl_pairs_within_from_matrix) as on the device.
// Compiled with -ffp-contract=off -fno-slp-vectorize like ward.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"
#include "dist_tile.h"  // tri_tile_count, tri_band_decode
#include "mfma_tile.h"  // xcd_remap
#include "pairs_select.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile
#include "ward_value.h"

#include <algorithm>
#include <cstring>

struct pw_args {
    const float *E;
    const int32_t *sz; // device copy of size (null: all 1)
    int64_t n;
    int d, vec;
    float thr;
    int64_t T;                  // tile rows
    int32_t *row_count;         // [n]   count pass: hits of row i
    uint8_t *hit;               // [T (T + 1) / 2]   count pass: tile ti (ti + 1) / 2 + tj had a hit
    unsigned long long *totals; // [2]   count pass: tiles with a hit, pairs j < i < n of those tiles
    const int32_t *rows;        // fill pass: the tile rows that have a hit
    const int64_t *row_ptr;     // [n + 1]
    int32_t *col;
    float *val;
};

// row / column of accumulator index a (0..7) of thread coordinate t (ty / tx), as ward_exact_tile.h lays them out
__device__ __forceinline__ int pw_lane_index(int a, int t) { return a < 4 ? t * 4 + a : 64 + t * 4 + (a - 4); }

__global__ __launch_bounds__(256) void pairs_count_kernel(pw_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ int32_t cnt[DT_TILE];
    int ti, tj;
    tri_band_decode(xcd_remap((int)blockIdx.x, (int)gridDim.x), 0, a.T, ti, tj);
    const int64_t i0 = (int64_t)ti * DT_TILE, j0 = (int64_t)tj * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    if (tid < DT_TILE) cnt[tid] = 0; // (the tile synchronises before anybody adds)
    float acc[8][8];
    ward_exact_tile(a.E, a.n, i0, a.E, a.n, j0, a.d, a.vec != 0, As, Bs, acc);

    // Padded rows and columns (i >= n, j >= n) are never offered, and on the diagonal tile only j < i is (ps_listed).
    int any = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int row = pw_lane_index(r, ty);
        const int64_t i = i0 + row;
        if (i >= a.n) continue;
        const int sa = a.sz ? a.sz[i] : 1;
        int c = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int64_t j = j0 + pw_lane_index(q, tx);
            if (j >= a.n) continue;
            c += ps_listed(i, j, ward_scale(acc[r][q], sa, a.sz ? a.sz[j] : 1), a.thr) ? 1 : 0;
        }
        if (c) {
            atomicAdd(&cnt[row], c);
            any = 1;
        }
    }
    if (!__syncthreads_or(any)) return;
    if (tid < DT_TILE && cnt[tid] > 0) atomicAdd(&a.row_count[i0 + tid], cnt[tid]); // (cnt > 0 only where i0 + tid < n)
    if (tid == 0) {
        a.hit[(int64_t)ti * (ti + 1) / 2 + tj] = 1;
        const int64_t nr = a.n - i0 < DT_TILE ? a.n - i0 : DT_TILE, nc = a.n - j0 < DT_TILE ? a.n - j0 : DT_TILE;
        atomicAdd(&a.totals[0], 1ull);
        atomicAdd(&a.totals[1], (unsigned long long)(ti == tj ? nr * (nr - 1) / 2 : nr * nc));
    }
}

__global__ __launch_bounds__(256) void pairs_fill_kernel(pw_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ uint32_t mask[DT_TILE][4]; // the tile's hits: bit c of row r's 128
    __shared__ int64_t rbase[DT_TILE];    // row_ptr[i]
    __shared__ int32_t rlen[DT_TILE];     // row i's hits in all (the count pass's figure: no place beyond it is ever written)
    __shared__ int32_t cur[DT_TILE];      // row i's hits in the tiles walked so far
    __shared__ uint8_t flag[256];
    const int ti = a.rows[blockIdx.x];
    const int64_t i0 = (int64_t)ti * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int w_lo = tx >> 3, sh = (tx & 7) * 4; // this thread's 4 columns of a half: word bh * 2 + w_lo of the row's mask, bits sh .. sh + 3

    if (tid < DT_TILE) {
        const int64_t i = i0 + tid;
        cur[tid] = 0;
        rbase[tid] = i < a.n ? a.row_ptr[i] : 0;
        rlen[tid] = i < a.n ? (int32_t)(a.row_ptr[i + 1] - a.row_ptr[i]) : 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) mask[tid][w] = 0;
    }
    const uint8_t *hrow = a.hit + (int64_t)ti * (ti + 1) / 2;
    for (int base = 0; base <= ti; base += 256) {
        __syncthreads();
        flag[tid] = base + tid <= ti ? hrow[base + tid] : 0;
        __syncthreads();
        for (int f = 0; f < 256; ++f) {
            if (!flag[f]) continue; // (the same answer in every thread)
            const int tj = base + f;
            const int64_t j0 = (int64_t)tj * DT_TILE;
            float acc[8][8];
            ward_exact_tile(a.E, a.n, i0, a.E, a.n, j0, a.d, a.vec != 0, As, Bs, acc);

            // the count pass's test again, into the rows' masks
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = pw_lane_index(r, ty);
                const int64_t i = i0 + row;
                if (i >= a.n) continue;
                const int sa = a.sz ? a.sz[i] : 1;
#pragma unroll
                for (int bh = 0; bh < 2; ++bh) {
                    uint32_t nib = 0;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t j = j0 + bh * 64 + tx * 4 + q;
                        if (j < a.n && ps_listed(i, j, ward_scale(acc[r][bh * 4 + q], sa, a.sz ? a.sz[j] : 1), a.thr)) nib |= 1u << q;
                    }
                    if (nib) atomicOr(&mask[row][bh * 2 + w_lo], nib << sh);
                }
            }
            __syncthreads();
            // a hit's place: behind the row's hits of the tiles walked before, and behind its hits of lower j in this tile
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int row = pw_lane_index(r, ty);
                const uint32_t m[4] = {mask[row][0], mask[row][1], mask[row][2], mask[row][3]};
                if (!(m[0] | m[1] | m[2] | m[3])) continue;
                const int64_t i = i0 + row;
                const int sa = a.sz ? a.sz[i] : 1;
                const int c0 = cur[row], len = rlen[row];
                const int64_t rb = rbase[row];
#pragma unroll
                for (int bh = 0; bh < 2; ++bh) {
                    const uint32_t mw = w_lo ? m[bh * 2 + 1] : m[bh * 2];
                    if (!((mw >> sh) & 15u)) continue;
                    int before = c0 + (bh ? __popc(m[0]) + __popc(m[1]) : 0) + (w_lo ? __popc(m[bh * 2]) : 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int b = sh + q;
                        if (!((mw >> b) & 1u)) continue;
                        const int p = before + __popc(mw & ((1u << b) - 1u));
                        if (p < len) {
                            const int64_t j = j0 + bh * 64 + tx * 4 + q;
                            a.col[rb + p] = (int32_t)j;
                            a.val[rb + p] = ward_scale(acc[r][bh * 4 + q], sa, a.sz ? a.sz[j] : 1);
                        }
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
                cur[tid] += c;
            }
            // (the next tile's barriers stand between this update and its readers)
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// What ICL_ERR_ARG covers for the output side, shared by the three forms: the reason, or nullptr.
static const char *pw_bad_out(int64_t n, float threshold, const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (n < 0) return "negative n";
    if (n >= (1LL << 31)) return "n must be below 2^31";
    if (threshold != threshold) return "the threshold is NaN";
    if (cap < 0) return "negative cap";
    if (!row_ptr || !total) return "a null pointer";
    if ((!col || !val) && (col || val || cap != 0)) return "col and val may be null only together and with cap == 0 (the size query)";
    return nullptr;
}

static int pw_check(icl_ctx *ctx, const char *what, const void *E, const int32_t *size, int64_t n, int32_t d, float threshold,
                    const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : pw_bad_out(n, threshold, row_ptr, col, val, cap, total);
    if (!why && n > 1 && !E) why = "a null pointer";
    for (int64_t i = 0; !why && size && i < n; ++i)
        if (size[i] <= 0) why = "a size entry is not above 0";
    if (!why && tri_tile_count(0, icl_ceil_div(n, DT_TILE)) < 0) why = "the tile grid does not fit a launch";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

struct pw_plan { // where the workspace's parts are, decided once per call
    pw_args a;
    int64_t ntiles = 0, fill_pairs = 0; // fill_pairs: the pairs j < i < n of the tiles with a hit
    size_t need = 0;
    char *d_row_ptr = nullptr, *d_rows = nullptr;
};

// ctx->mu held, the device selected, the arguments checked, n > 1.  Count pass and prefix: row_ptr and *total complete on return.
static int pw_count_locked(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                           int64_t *total, pw_plan &pl)
{
    const int64_t T = icl_ceil_div(n, DT_TILE), ntiles = tri_tile_count(0, T);
    // [size] [row_count | totals | hit] [row_ptr] [tile rows], each on a 16-byte boundary.  The three pieces the count pass adds to are
    // taken one after the other, so they are one contiguous range: o_cnt .. o_ptr, cleared by the single memset below.
    icl_ws_layout L(16);
    const size_t o_sz = L.take(size ? (size_t)n * 4 : 0), o_cnt = L.take((size_t)n * 4), o_tot = L.take(16), o_hit = L.take((size_t)ntiles);
    const size_t o_ptr = L.take((size_t)(n + 1) * 8), o_rows = L.take((size_t)T * 4);
    pl.need = L.total;
    pl.ntiles = ntiles;
    ICL_TRY(ctx->pairs.ensure(ctx, pl.need, "icl_pairs_within: workspace"));
    char *ws = ctx->pairs.as<char>();
    if (size) { // the caller's array may go away at return: a copy that has finished by then (the read-back below waits for it)
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_sz, size, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    ICL_HIP(ctx, hipMemsetAsync(ws + o_cnt, 0, o_ptr - o_cnt, ctx->stream));
    pw_args &a = pl.a;
    a.E = d_E;
    a.sz = size ? (const int32_t *)(ws + o_sz) : nullptr;
    a.n = n;
    a.d = d;
    a.vec = (d & 3) == 0 && ((uintptr_t)d_E & 15) == 0;
    a.thr = threshold;
    a.T = T;
    a.row_count = (int32_t *)(ws + o_cnt);
    a.totals = (unsigned long long *)(ws + o_tot);
    a.hit = (uint8_t *)(ws + o_hit);
    pl.d_row_ptr = ws + o_ptr;
    pl.d_rows = ws + o_rows;
    a.rows = (const int32_t *)pl.d_rows;
    a.row_ptr = (const int64_t *)pl.d_row_ptr;
    a.col = nullptr;
    a.val = nullptr;
    hipLaunchKernelGGL(pairs_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
    ICL_HIP(ctx, hipGetLastError());
    std::vector<int32_t> cnt((size_t)n);
    unsigned long long tot[2] = {0, 0};
    ICL_HIP(ctx, hipMemcpyAsync(cnt.data(), a.row_count, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(tot, a.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    row_ptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) row_ptr[i + 1] = row_ptr[i] + cnt[(size_t)i];
    *total = row_ptr[n];
    ctx->pairs_stats[0] = ntiles;
    ctx->pairs_stats[1] = (int64_t)tot[0];
    ctx->pairs_stats[2] = n * (n - 1) / 2;
    ctx->pairs_stats[3] = (int64_t)pl.need;
    pl.fill_pairs = (int64_t)tot[1];
    return ICL_OK;
}

// The fill pass behind a count pass of the same call (row_ptr as it left it, *total > 0 of them fit d_col / d_val).  The host arrays
// are uploaded and done with at return; the kernel itself is enqueued on the context's stream.
static int pw_fill_locked(icl_ctx *ctx, const int64_t *row_ptr, int64_t n, pw_plan &pl, int32_t *d_col, float *d_val)
{
    std::vector<int32_t> rows; // the tile rows with a hit, longest first: a row's workgroup walks up to ti + 1 tiles
    for (int64_t ti = pl.a.T - 1; ti >= 0; --ti)
        if (row_ptr[std::min<int64_t>(n, (ti + 1) * DT_TILE)] > row_ptr[ti * DT_TILE]) rows.push_back((int32_t)ti);
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_row_ptr, row_ptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.a.col = d_col;
    pl.a.val = d_val;
    hipLaunchKernelGGL(pairs_fill_kernel, dim3((unsigned)rows.size()), dim3(256), 0, ctx->stream, pl.a);
    ICL_HIP(ctx, hipGetLastError());
    ctx->pairs_stats[2] += pl.fill_pairs;
    return ICL_OK;
}

static void pw_empty(int64_t n, int64_t *row_ptr, int64_t *total)
{
    for (int64_t i = 0; i <= n; ++i) row_ptr[i] = 0;
    *total = 0;
}

extern "C" int icl_pairs_within_dev(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                                    int32_t *d_col, float *d_val, int64_t cap, int64_t *total)
{
    return no_throw(ctx, "icl_pairs_within_dev", [&]() -> int {
        ICL_TRY(pw_check(ctx, "icl_pairs_within_dev", d_E, size, n, d, threshold, row_ptr, d_col, d_val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->pairs_stats) s = 0;
        if (n <= 1) {
            pw_empty(n, row_ptr, total);
            return ICL_OK;
        }
        pw_plan pl;
        ICL_TRY(pw_count_locked(ctx, d_E, size, n, d, threshold, row_ptr, total, pl));
        if (*total > cap) {
            if (!d_col && !d_val) return ICL_OK; // the size query
            return icl_fail(ctx, ICL_ERR_ARG, "icl_pairs_within_dev: %lld pairs do not fit cap = %lld (row_ptr and total are complete)",
                            (long long)*total, (long long)cap);
        }
        if (*total == 0) return ICL_OK;
        return pw_fill_locked(ctx, row_ptr, n, pl, d_col, d_val);
    });
}

extern "C" int icl_pairs_within(icl_ctx *ctx, const float *E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                                int32_t *col, float *val, int64_t cap, int64_t *total)
{
    return no_throw(ctx, "icl_pairs_within", [&]() -> int {
        ICL_TRY(pw_check(ctx, "icl_pairs_within", E, size, n, d, threshold, row_ptr, col, val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->pairs_stats) s = 0;
        if (n <= 1) {
            pw_empty(n, row_ptr, total);
            return ICL_OK;
        }
        dev_guard dE, dC, dV;
        ICL_TRY(icl_dev_upload(ctx, dE, E, (size_t)n * d * 4, "icl_pairs_within: E"));
        pw_plan pl;
        ICL_TRY(pw_count_locked(ctx, (const float *)dE.p, size, n, d, threshold, row_ptr, total, pl));
        if (*total > cap) {
            if (!col && !val) return ICL_OK; // the size query
            return icl_fail(ctx, ICL_ERR_ARG, "icl_pairs_within: %lld pairs do not fit cap = %lld (row_ptr and total are complete)",
                            (long long)*total, (long long)cap);
        }
        if (*total == 0) return ICL_OK;
        const size_t bo = (size_t)*total * 4;
        ICL_TRY(icl_dev_alloc(ctx, dC, bo, "icl_pairs_within: col"));
        ICL_TRY(icl_dev_alloc(ctx, dV, bo, "icl_pairs_within: val"));
        ICL_TRY(pw_fill_locked(ctx, row_ptr, n, pl, (int32_t *)dC.p, (float *)dV.p));
        ICL_HIP(ctx, hipMemcpyAsync(col, dC.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(val, dV.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    });
}

extern "C" int icl_pairs_within_from_matrix(const float *D, int64_t n, int64_t ld, float threshold, int64_t *row_ptr, int32_t *col, float *val,
                                            int64_t cap, int64_t *total)
{
    if (pw_bad_out(n, threshold, row_ptr, col, val, cap, total) || ld < n || (n > 1 && !D)) return ICL_ERR_ARG;
    int64_t t = 0;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < i; ++j) t += ps_listed(i, j, D[i * ld + j], threshold) ? 1 : 0;
    const bool fits = t <= cap;
    int64_t p = 0;
    row_ptr[0] = 0;
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t j = 0; j < i; ++j)
            if (ps_listed(i, j, D[i * ld + j], threshold)) {
                if (fits) {
                    col[p] = (int32_t)j;
                    val[p] = D[i * ld + j];
                }
                ++p;
            }
        row_ptr[i + 1] = p;
    }
    *total = p;
    return fits || (!col && !val) ? ICL_OK : ICL_ERR_ARG;
}

extern "C" int icl_pair_groups(int64_t n, const int64_t *row_ptr, const int32_t *col, int32_t *group, int64_t *n_groups)
{
    if (n < 0 || n >= (1LL << 31) || !row_ptr || !n_groups || (n > 0 && !group) || row_ptr[0] != 0) return ICL_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return ICL_ERR_ARG;
    if (row_ptr[n] > 0 && !col) return ICL_ERR_ARG;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p)
            if (col[p] < 0 || col[p] >= i) return ICL_ERR_ARG;
    try {
        // union-find whose root is always its component's smallest index: the lower root adopts the higher one
        std::vector<int32_t> par((size_t)n);
        for (int64_t i = 0; i < n; ++i) par[(size_t)i] = (int32_t)i;
        auto find = [&](int32_t x) {
            while (par[(size_t)x] != x) {
                par[(size_t)x] = par[(size_t)par[(size_t)x]];
                x = par[(size_t)x];
            }
            return x;
        };
        for (int64_t i = 0; i < n; ++i)
            for (int64_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p) {
                const int32_t a = find((int32_t)i), b = find(col[p]);
                if (a != b) par[(size_t)std::max(a, b)] = std::min(a, b);
            }
        int64_t ng = 0;
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t r = find((int32_t)i);
            group[i] = r;
            if (r != i && !seen[(size_t)r]) {
                seen[(size_t)r] = 1;
                ++ng;
            }
        }
        *n_groups = ng;
    } catch (const std::bad_alloc &) {
        return ICL_ERR_NOMEM;
    }
    return ICL_OK;
}

extern "C" int icl_last_pairs_stats(icl_ctx *ctx, int64_t info[4])
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_pairs_stats: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < 4; ++q) info[q] = ctx->pairs_stats[q];
    return ICL_OK;
}
