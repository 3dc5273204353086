// pairs.hip -- the two exact threshold joins, each a CSR list with no distance matrix and no cap on a row's partners:
//   icl_pairs_within   every pair of rows of one set whose WardDistance is at most a threshold, over the strict lower triangle;
//   icl_pairs_between  every pair (query row, library row) of two sets, over the rectangle.
//
// Values are the reference's (clustering.go:136-157; ward_value.h) from the exact tile (ward_exact_tile.h), bit for bit what
// ward_dist_exact_kernel (ward.hip) and icl_nearest give.  Which pairs are listed is decided by pairs_select.h alone, on the host
// (pairs_plan.h's _from_matrix forms) as on the device.  Both families run the same three steps:
//   COUNT  per 128 x 128 tile: the exact tile, the rule, the hits of each row summed in 128 LDS counters, and a flag byte for a tile
//          with a hit (pairs_tile_count).  The two families publish differently, so there are two count kernels:
//            within   one workgroup per tile of the triangle in dist_tile.h's band order; a row's hits are added to count[i] with one
//                     integer atomic per row and tile that has hits (integer sums do not depend on order); a tile without a hit
//                     leaves after one __syncthreads_or.
//            between  the band walk's geometry (band_select.h): a workgroup is (band of 128 query rows, split s) and walks the library
//                     tiles  s * ntiles / splits .. (s + 1) * ntiles / splits,  band = block % nbands, split = block / nbands, so the
//                     bands that run together read the same library tiles at about the same time.  Every flag and every count
//                     count[i * splits + s] has exactly one writer in the launch, so the stores are plain: no global atomic and no
//                     memset.  splits comes from band_splits() (band_plan.h); icl_set_nearest_options' forced count applies.
//   PREFIX on the host over the counts in (row, split) order (pairs_prefix, pairs_plan.h; within has one split): seg_ptr, row_ptr,
//          *total and the capacity decision.  A split is a column RANGE and the ranges are taken in ascending order: that is what
//          makes a row's segments, laid end to end, ascending in j.
//   FILL   one kernel body for both (pairs_fill_kernel<G>): a workgroup walks the flagged tiles of its band and column range in
//          ascending order, recomputes each and writes every hit at  seg_ptr[segment] + (the row's hits in the tiles already walked) +
//          (its hits of lower j in this tile, from a 128-bit mask per row in LDS: pairs_mask_rank).  No atomic decides a place and
//          nothing is sorted.  What differs is the geometry policy G: within (pairs_tri) a workgroup is a tile row of the triangle and
//          walks it up to the diagonal; between (pairs_rect) it is the count pass's (band, split).
// Compiled with -ffp-contract=off -fno-slp-vectorize like ward.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"
#include "band_plan.h"
#include "dist_tile.h"  // tri_tile_count, tri_band_decode
#include "mfma_tile.h"  // xcd_remap
#include "pairs_plan.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile, dt_lane_index
#include "ward_value.h"

#include <algorithm>
#include <vector>

static_assert(PAIRS_ROWS == DT_TILE, "pairs_plan.h's masks are worked out for the exact tile's 128 columns");

struct pairs_args { // within: A == B, rs == cs, ni == nj, no exclude, one split, nbands tile rows
    const float *A, *B;          // the rows' operand [ni][d] and the columns' [nj][d]
    const int32_t *rs, *cs, *ex; // device copies of the row sizes, the column sizes and exclude (each may be null: all 1 / none)
    int64_t ni, nj;
    int d, vec;
    float thr;
    int64_t ntiles, nbands; // tiles of 128 columns (between) / tiles of the triangle (within); bands of 128 rows
    int splits;
    int32_t *count;             // count pass: within [ni] hits of row i; between [ni * splits] hits of row i in split s's tiles
    uint8_t *hit;               // count pass: the tile had a hit (G::flags says where a band's flags are)
    const int32_t *work;        // fill pass: its workgroups (within: tile rows with a hit; between: the count grid's workgroups with one)
    const int64_t *seg_ptr;     // [ni * splits + 1]   fill pass
    int32_t *col;
    float *val;
    unsigned long long *totals; // [2]   within's count pass: tiles with a hit, pairs j < i < n of those tiles
};

// ---- the geometry policies ------------------------------------------------------------------------------------------------------
// What a fill workgroup walks, where its band's flags and a row's segment are, and the rule: listed(key of the row, j, value).
struct pairs_tri { // icl_pairs_within: tile row `band` of the lower triangle, up to its diagonal tile; the rule needs the row's index
    static __device__ __forceinline__ void range(const pairs_args &, int64_t block, int64_t &band, int64_t &split, int64_t &t_lo, int64_t &t_hi)
    {
        band = block;
        split = 0;
        t_lo = 0;
        t_hi = band + 1;
    }
    static __device__ __forceinline__ uint8_t *flags(const pairs_args &a, int64_t band) { return a.hit + band * (band + 1) / 2; }
    static __device__ __forceinline__ int64_t segment(const pairs_args &, int64_t i, int64_t) { return i; }
    static __device__ __forceinline__ int32_t key(const pairs_args &, int64_t i) { return (int32_t)i; } // (n < 2^31)
    static __device__ __forceinline__ bool listed(int64_t key, int64_t j, float v, float thr) { return ps_listed(key, j, v, thr); }
};

struct pairs_rect { // icl_pairs_between: (band, split) of the band walk; the rule needs the row's excluded column
    static __device__ __forceinline__ void range(const pairs_args &a, int64_t block, int64_t &band, int64_t &split, int64_t &t_lo, int64_t &t_hi)
    {
        band = block % a.nbands;
        split = block / a.nbands;
        t_lo = split * a.ntiles / a.splits;
        t_hi = (split + 1) * a.ntiles / a.splits;
    }
    static __device__ __forceinline__ uint8_t *flags(const pairs_args &a, int64_t band) { return a.hit + band * a.ntiles; }
    static __device__ __forceinline__ int64_t segment(const pairs_args &a, int64_t i, int64_t split) { return i * a.splits + split; }
    static __device__ __forceinline__ int32_t key(const pairs_args &a, int64_t i) { return (a.ex && i < a.ni) ? a.ex[i] : -1; }
    static __device__ __forceinline__ bool listed(int64_t key, int64_t j, float v, float thr) { return ps_listed_between(j, key, v, thr); }
};

// ---- what every pass does with a tile -------------------------------------------------------------------------------------------
// Sizes, keys and counters of the band's 128 rows and the tile's 128 columns live in LDS, indexed by the place inside the tile.
__device__ __forceinline__ void pairs_stage_sizes(int32_t *lds, const int32_t *sz, int64_t first, int64_t n)
{
    const int tid = threadIdx.x;
    if (tid < DT_TILE) lds[tid] = (sz && first + tid < n) ? sz[first + tid] : 1;
}

// COUNT: scale the thread's 8 x 8 sums, ask the rule, add each row's hits to cnt[row]; -> whether the tile has a hit, in every thread
// (it synchronises).  Padded rows and columns (i >= ni, j >= nj) are never offered.
template <class G>
__device__ __forceinline__ int pairs_tile_count(const float (&acc)[8][8], int64_t i0, int64_t ni, int64_t j0, int64_t nj, const int32_t *rsz,
                                                const int32_t *csz, const int32_t *key, float thr, int32_t *cnt)
{
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int any = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int row = dt_lane_index(r, ty);
        if (i0 + row >= ni) continue;
        const int sa = rsz[row];
        const int64_t k = key[row];
        int c = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int cl = dt_lane_index(q, tx);
            const int64_t j = j0 + cl;
            if (j >= nj) continue;
            c += G::listed(k, j, ward_scale(acc[r][q], sa, csz[cl]), thr) ? 1 : 0;
        }
        if (c) {
            atomicAdd(&cnt[row], c); // (LDS; integer sums do not depend on order)
            any = 1;
        }
    }
    return __syncthreads_or(any);
}

// FILL: the count pass's test again into a 128-bit mask per row; every hit to its place  sbase[row] + cur[row] + its rank in the mask,
// compared with the segment's length slen[row] (the count pass's figure: no place beyond it is ever written); then cur advances and
// the masks are cleared.  The next tile's barriers stand between that update and its readers.
template <class G>
__device__ __forceinline__ void pairs_tile_fill(const float (&acc)[8][8], int64_t i0, int64_t ni, int64_t j0, int64_t nj, const int32_t *rsz,
                                                const int32_t *csz, const int32_t *key, float thr, uint32_t (*mask)[4], int32_t *cur,
                                                const int64_t *sbase, const int32_t *slen, int32_t *col, float *val)
{
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int row = dt_lane_index(r, ty);
        if (i0 + row >= ni) continue;
        const int sa = rsz[row];
        const int64_t k = key[row];
#pragma unroll
        for (int bh = 0; bh < 2; ++bh) { // a thread's 4 neighbouring columns of a half are a nibble of the row's mask
            uint32_t nib = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int cl = bh * 64 + tx * 4 + q;
                const int64_t j = j0 + cl;
                if (j < nj && G::listed(k, j, ward_scale(acc[r][bh * 4 + q], sa, csz[cl]), thr)) nib |= 1u << q;
            }
            if (nib) atomicOr(&mask[row][bh * 2 + (tx >> 3)], nib << ((tx & 7) * 4));
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int row = dt_lane_index(r, ty);
        const uint32_t m[4] = {mask[row][0], mask[row][1], mask[row][2], mask[row][3]};
        if (!(m[0] | m[1] | m[2] | m[3])) continue;
        const int sa = rsz[row];
        const int c0 = cur[row], len = slen[row];
        const int64_t sb = sbase[row];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int cl = dt_lane_index(q, tx);
            if (!((m[cl >> 5] >> (cl & 31)) & 1u)) continue;
            const int p = c0 + pairs_mask_rank(m, cl);
            if (p < len) {
                col[sb + p] = (int32_t)(j0 + cl);
                val[sb + p] = ward_scale(acc[r][q], sa, csz[cl]);
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
}

// ---- the kernels ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pairs_count_kernel(pairs_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ int32_t cnt[DT_TILE], rsz[DT_TILE], csz[DT_TILE], key[DT_TILE];
    int ti, tj;
    tri_band_decode(xcd_remap((int)blockIdx.x, (int)gridDim.x), 0, a.nbands, ti, tj);
    const int64_t i0 = (int64_t)ti * DT_TILE, j0 = (int64_t)tj * DT_TILE;
    const int tid = threadIdx.x;

    if (tid < DT_TILE) {
        cnt[tid] = 0;
        key[tid] = pairs_tri::key(a, i0 + tid);
    }
    pairs_stage_sizes(rsz, a.rs, i0, a.ni);
    pairs_stage_sizes(csz, a.cs, j0, a.nj); // (the tile synchronises before anybody reads or adds)
    float acc[8][8];
    ward_exact_tile(a.A, a.ni, i0, a.B, a.nj, j0, a.d, a.vec != 0, As, Bs, acc);

    // on the diagonal tile only j < i is listed (ps_listed)
    if (!pairs_tile_count<pairs_tri>(acc, i0, a.ni, j0, a.nj, rsz, csz, key, a.thr, cnt)) return;
    if (tid < DT_TILE && cnt[tid] > 0) atomicAdd(&a.count[i0 + tid], cnt[tid]); // (cnt > 0 only where i0 + tid < n)
    if (tid == 0) {
        pairs_tri::flags(a, ti)[tj] = 1;
        const int64_t nr = a.ni - i0 < DT_TILE ? a.ni - i0 : DT_TILE, nc = a.nj - j0 < DT_TILE ? a.nj - j0 : DT_TILE;
        atomicAdd(&a.totals[0], 1ull);
        atomicAdd(&a.totals[1], (unsigned long long)(ti == tj ? nr * (nr - 1) / 2 : nr * nc));
    }
}

static __global__ __launch_bounds__(256) void pairs_between_count_kernel(pairs_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ int32_t cnt[DT_TILE], rsz[DT_TILE], csz[DT_TILE], key[DT_TILE]; // cnt: the row's hits in the tiles walked so far
    // workgroups of one split are neighbours: the bands that run together read the same library tiles at about the same time
    int64_t band, split, t_lo, t_hi;
    pairs_rect::range(a, (int64_t)blockIdx.x, band, split, t_lo, t_hi);
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;

    if (tid < DT_TILE) {
        cnt[tid] = 0;
        key[tid] = pairs_rect::key(a, i0 + tid);
    }
    pairs_stage_sizes(rsz, a.rs, i0, a.ni);
    __syncthreads();

    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * DT_TILE;
        pairs_stage_sizes(csz, a.cs, j0, a.nj); // (read after the tile's barriers)
        float acc[8][8];
        ward_exact_tile(a.A, a.ni, i0, a.B, a.nj, j0, a.d, a.vec != 0, As, Bs, acc);
        // (the epilogue's barrier also stands between this tile's readers of csz and the next tile's writers)
        const int some = pairs_tile_count<pairs_rect>(acc, i0, a.ni, j0, a.nj, rsz, csz, key, a.thr, cnt);
        if (tid == 0) pairs_rect::flags(a, band)[t] = some ? 1 : 0;
    }

    __syncthreads();
    const int64_t i = i0 + tid;
    if (tid < DT_TILE && i < a.ni) a.count[pairs_rect::segment(a, i, split)] = cnt[tid];
}

template <class G> static __global__ __launch_bounds__(256) void pairs_fill_kernel(pairs_args a)
{
    __shared__ __attribute__((aligned(16))) float As[DT_KC][DT_LD];
    __shared__ __attribute__((aligned(16))) float Bs[DT_KC][DT_LD];
    __shared__ int32_t cur[DT_TILE], rsz[DT_TILE], csz[DT_TILE], key[DT_TILE]; // cur: the row's hits in the tiles walked so far
    __shared__ uint32_t mask[DT_TILE][4]; // the tile's hits: bit c of row r's 128
    __shared__ int64_t sbase[DT_TILE];    // seg_ptr of the row's segment
    __shared__ int32_t slen[DT_TILE];     // the segment's hits in all
    __shared__ uint8_t flag[256];
    int64_t band, split, t_lo, t_hi;
    G::range(a, (int64_t)a.work[blockIdx.x], band, split, t_lo, t_hi);
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;

    if (tid < DT_TILE) {
        const int64_t i = i0 + tid, sg = G::segment(a, i, split);
        cur[tid] = 0;
        key[tid] = G::key(a, i);
        sbase[tid] = i < a.ni ? a.seg_ptr[sg] : 0;
        slen[tid] = i < a.ni ? (int32_t)(a.seg_ptr[sg + 1] - a.seg_ptr[sg]) : 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) mask[tid][w] = 0;
    }
    pairs_stage_sizes(rsz, a.rs, i0, a.ni);
    const uint8_t *frow = G::flags(a, band);
    for (int64_t base = t_lo; base < t_hi; base += 256) { // the band's flags, 256 at a time
        __syncthreads();
        flag[tid] = base + tid < t_hi ? frow[base + tid] : 0;
        __syncthreads();
        const int nf = (int)(t_hi - base < 256 ? t_hi - base : 256);
        for (int f = 0; f < nf; ++f) {
            if (!flag[f]) continue; // (the same answer in every thread)
            const int64_t j0 = (base + f) * DT_TILE;
            pairs_stage_sizes(csz, a.cs, j0, a.nj); // (read after the tile's barriers, written after the last tile's placement barrier)
            float acc[8][8];
            ward_exact_tile(a.A, a.ni, i0, a.B, a.nj, j0, a.d, a.vec != 0, As, Bs, acc);
            pairs_tile_fill<G>(acc, i0, a.ni, j0, a.nj, rsz, csz, key, a.thr, mask, cur, sbase, slen, a.col, a.val);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct pairs_plan { // one call: the launch arguments, where the workspace's parts are, what the count step leaves for the fill step
    pairs_args a = {};
    int64_t fill_pairs = 0; // the pairs of the tiles with a hit
    size_t need = 0;
    char *d_seg_ptr = nullptr, *d_work = nullptr;
    std::vector<int64_t> seg_ptr; // [ni * splits + 1]
    std::vector<int32_t> work;    // the fill pass's workgroups
};

static int pw_check(icl_ctx *ctx, const char *what, const void *E, const int32_t *size, int64_t n, int32_t d, float threshold,
                    const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : pairs_within_bad_arg(n, threshold, row_ptr, col, val, cap, total);
    if (!why && n > 1 && !E) why = "a null pointer";
    for (int64_t i = 0; !why && size && i < n; ++i)
        if (size[i] <= 0) why = "a size entry is not above 0";
    if (!why && tri_tile_count(0, icl_ceil_div(n, DT_TILE)) < 0) why = "the tile grid does not fit a launch";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

static int pb_check(icl_ctx *ctx, const char *what, const void *Q, const int32_t *q_size, int64_t nq, const void *L, const int32_t *l_size,
                    int64_t n, int32_t d, float threshold, const int64_t *exclude, const int64_t *row_ptr, const void *col, const void *val,
                    int64_t cap, const int64_t *total)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : pairs_between_bad_arg(nq, n, threshold, q_size, l_size, exclude, row_ptr, col, val, cap, total);
    if (!why && nq > 0 && n > 0 && (!Q || !L)) why = "a null pointer";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

// ctx->mu held: icl_pairs_between's geometry, before anything is written (a grid that does not fit one launch is a bad argument).
static int pb_decide(icl_ctx *ctx, const char *what, int64_t nq, int64_t n, pairs_plan &pl)
{
    pl.a.nbands = icl_ceil_div(nq, DT_TILE);
    pl.a.ntiles = icl_ceil_div(n, DT_TILE);
    pl.a.splits = band_splits(ctx->nearest_splits, ctx->prop.multiProcessorCount, pl.a.nbands, pl.a.ntiles);
    if (pl.a.nbands * pl.a.splits > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_ARG, "%s: the grid does not fit a launch (nq=%lld)", what, (long long)nq);
    return ICL_OK;
}

// What both count steps set from their operands (the workspace's pointers are the family's own business).
static void pairs_set_operands(pairs_args &a, const float *d_A, int64_t ni, const float *d_B, int64_t nj, int32_t d, float threshold)
{
    a.A = d_A;
    a.B = d_B;
    a.ni = ni;
    a.nj = nj;
    a.d = d;
    a.vec = (d & 3) == 0 && (((uintptr_t)d_A | (uintptr_t)d_B) & 15) == 0;
    a.thr = threshold;
}

// ctx->mu held, the device selected, the arguments checked, n > 1.  Count pass and prefix: row_ptr and *total complete on return.
static int pw_count_locked(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                           int64_t *total, pairs_plan &pl)
{
    const int64_t T = icl_ceil_div(n, DT_TILE), ntiles = tri_tile_count(0, T);
    // [size] [row_count | totals | hit] [row_ptr] [tile rows], each on a 16-byte boundary.  The three pieces the count pass adds to are
    // taken one after the other, so they are one contiguous range: o_cnt .. o_ptr, cleared by the single memset below.
    icl_ws_layout L(16);
    const size_t o_sz = L.take(size ? (size_t)n * 4 : 0), o_cnt = L.take((size_t)n * 4), o_tot = L.take(16), o_hit = L.take((size_t)ntiles);
    const size_t o_ptr = L.take((size_t)(n + 1) * 8), o_rows = L.take((size_t)T * 4);
    pl.need = L.total;
    ICL_TRY(ctx->pairs.ensure(ctx, pl.need, "icl_pairs_within: workspace"));
    char *ws = ctx->pairs.as<char>();
    if (size) { // the caller's array may go away at return: a copy that has finished by then (the read-back below waits for it)
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_sz, size, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    ICL_HIP(ctx, hipMemsetAsync(ws + o_cnt, 0, o_ptr - o_cnt, ctx->stream));
    pairs_args &a = pl.a;
    pairs_set_operands(a, d_E, n, d_E, n, d, threshold);
    a.rs = a.cs = size ? (const int32_t *)(ws + o_sz) : nullptr;
    a.nbands = T;
    a.ntiles = ntiles;
    a.splits = 1;
    a.count = (int32_t *)(ws + o_cnt);
    a.totals = (unsigned long long *)(ws + o_tot);
    a.hit = (uint8_t *)(ws + o_hit);
    pl.d_seg_ptr = ws + o_ptr;
    pl.d_work = ws + o_rows;
    hipLaunchKernelGGL(pairs_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream, a);
    ICL_HIP(ctx, hipGetLastError());
    std::vector<int32_t> cnt((size_t)n);
    unsigned long long tot[2] = {0, 0};
    ICL_HIP(ctx, hipMemcpyAsync(cnt.data(), a.count, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(tot, a.totals, sizeof tot, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.seg_ptr.resize((size_t)n + 1);
    pairs_prefix(n, 1, cnt.data(), pl.seg_ptr.data(), row_ptr, total);
    // the fill pass's workgroups: the tile rows with a hit, longest first (a row's workgroup walks up to ti + 1 tiles)
    for (int64_t ti = T - 1; ti >= 0; --ti)
        if (row_ptr[std::min<int64_t>(n, (ti + 1) * DT_TILE)] > row_ptr[ti * DT_TILE]) pl.work.push_back((int32_t)ti);
    ctx->pairs_stats[0] = ntiles;
    ctx->pairs_stats[1] = (int64_t)tot[0];
    ctx->pairs_stats[2] = n * (n - 1) / 2;
    ctx->pairs_stats[3] = (int64_t)pl.need;
    pl.fill_pairs = (int64_t)tot[1];
    return ICL_OK;
}

// ctx->mu held, the device selected, the arguments checked, the geometry decided, nq > 0 and n > 0.  Count pass and prefix: row_ptr
// and *total complete on return.
static int pb_count_locked(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_L, const int32_t *l_size, int64_t n,
                           int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int64_t *total, pairs_plan &pl)
{
    pairs_args &a = pl.a;
    const int64_t nseg = nq * a.splits, nflag = a.nbands * a.ntiles, ngrid = a.nbands * a.splits;
    std::vector<int32_t> ex32(exclude, exclude + (exclude ? nq : 0)); // (n < 2^31)
    // [q_size] [l_size] [exclude] [seg_count] [hit] [seg_ptr] [work], each on a 16-byte boundary; the first three go up in one copy
    icl_ws_upload up;
    const size_t o_qs = up.add(q_size, nq), o_ls = up.add(l_size, n), o_ex = up.add(exclude ? ex32.data() : nullptr, nq), b_meta = up.L.total;
    const size_t o_cnt = up.L.take((size_t)nseg * 4), o_hit = up.L.take((size_t)nflag), o_ptr = up.L.take((size_t)(nseg + 1) * 8);
    const size_t o_work = up.L.take((size_t)ngrid * 4);
    pl.need = up.L.total;
    ICL_TRY(ctx->pairs.ensure(ctx, pl.need, "icl_pairs_between: workspace"));
    char *ws = ctx->pairs.as<char>();
    ICL_TRY(up.go(ctx, ws, b_meta));
    pairs_set_operands(a, d_Q, nq, d_L, n, d, threshold);
    a.rs = q_size ? (const int32_t *)(ws + o_qs) : nullptr;
    a.cs = l_size ? (const int32_t *)(ws + o_ls) : nullptr;
    a.ex = exclude ? (const int32_t *)(ws + o_ex) : nullptr;
    a.count = (int32_t *)(ws + o_cnt);
    a.hit = (uint8_t *)(ws + o_hit);
    pl.d_seg_ptr = ws + o_ptr;
    pl.d_work = ws + o_work;
    hipLaunchKernelGGL(pairs_between_count_kernel, dim3((unsigned)ngrid), dim3(256), 0, ctx->stream, a);
    ICL_HIP(ctx, hipGetLastError());
    std::vector<int32_t> cnt((size_t)nseg);
    std::vector<uint8_t> hit((size_t)nflag);
    ICL_HIP(ctx, hipMemcpyAsync(cnt.data(), a.count, (size_t)nseg * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(hit.data(), a.hit, (size_t)nflag, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.seg_ptr.resize((size_t)nseg + 1);
    pairs_prefix(nq, a.splits, cnt.data(), pl.seg_ptr.data(), row_ptr, total);
    // the fill pass's workgroups: (band, split) with a flagged tile, in the count grid's order
    int64_t hits = 0;
    for (int64_t s = 0; s < a.splits; ++s)
        for (int64_t b = 0; b < a.nbands; ++b) {
            const int64_t nr = std::min<int64_t>(DT_TILE, nq - b * DT_TILE);
            bool some = false;
            for (int64_t t = s * a.ntiles / a.splits; t < (s + 1) * a.ntiles / a.splits; ++t)
                if (hit[(size_t)(b * a.ntiles + t)]) {
                    some = true;
                    ++hits;
                    pl.fill_pairs += nr * std::min<int64_t>(DT_TILE, n - t * DT_TILE);
                }
            if (some) pl.work.push_back((int32_t)(s * a.nbands + b));
        }
    ctx->between_stats[0] = a.splits;
    ctx->between_stats[1] = nflag;
    ctx->between_stats[2] = hits;
    ctx->between_stats[3] = nq * n;
    ctx->between_stats[4] = (int64_t)pl.need;
    return ICL_OK;
}

// The fill pass behind a count step of the same call (*total > 0 entries fit d_col / d_val).  The host arrays are uploaded and done
// with at return; the kernel itself is enqueued on the context's stream.  pairs_evaluated: the family's statistic.
template <class G> static int pairs_fill_locked(icl_ctx *ctx, pairs_plan &pl, int32_t *d_col, float *d_val, int64_t &pairs_evaluated)
{
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_seg_ptr, pl.seg_ptr.data(), pl.seg_ptr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(pl.d_work, pl.work.data(), pl.work.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    pl.a.work = (const int32_t *)pl.d_work;
    pl.a.seg_ptr = (const int64_t *)pl.d_seg_ptr;
    pl.a.col = d_col;
    pl.a.val = d_val;
    hipLaunchKernelGGL(pairs_fill_kernel<G>, dim3((unsigned)pl.work.size()), dim3(256), 0, ctx->stream, pl.a);
    ICL_HIP(ctx, hipGetLastError());
    pairs_evaluated += pl.fill_pairs;
    return ICL_OK;
}

// The body of the four entry points behind their checks, ctx->mu held and the device selected.  stats: the family's array, reset here.
// count() leaves row_ptr and *total complete; fill(d_col, d_val) enqueues the fill pass.  host_out: col / val are host arrays, so
// exactly *total entries are allocated on the device, filled and downloaded.
template <class Count, class Fill, size_t NS>
static int pairs_run(icl_ctx *ctx, const char *what, int64_t (&stats)[NS], bool empty, int64_t nrows, int64_t *row_ptr, int32_t *col, float *val,
                     bool host_out, int64_t cap, int64_t *total, Count count, Fill fill)
{
    for (int64_t &s : stats) s = 0;
    if (empty) {
        pairs_empty(nrows, row_ptr, total);
        return ICL_OK;
    }
    ICL_TRY(count());
    if (*total > cap) {
        if (!col && !val) return ICL_OK; // the size query
        return icl_fail(ctx, ICL_ERR_ARG, "%s: %lld pairs do not fit cap = %lld (row_ptr and total are complete)", what, (long long)*total,
                        (long long)cap);
    }
    if (*total == 0) return ICL_OK;
    if (!host_out) return fill(col, val);
    dev_guard dC, dV;
    const size_t bo = (size_t)*total * 4;
    ICL_TRY(icl_dev_alloc(ctx, dC, bo, "%s: col", what));
    ICL_TRY(icl_dev_alloc(ctx, dV, bo, "%s: val", what));
    ICL_TRY(fill((int32_t *)dC.p, (float *)dV.p));
    ICL_HIP(ctx, hipMemcpyAsync(col, dC.p, bo, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(val, dV.p, bo, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
}

// E on the device (host_rows: uploaded first, behind the statistics' reset and the empty case).
static int pw_run(icl_ctx *ctx, const char *what, bool host_rows, const float *E, const int32_t *size, int64_t n, int32_t d, float threshold,
                  int64_t *row_ptr, int32_t *col, float *val, int64_t cap, int64_t *total)
{
    return no_throw(ctx, what, [&]() -> int {
        ICL_TRY(pw_check(ctx, what, E, size, n, d, threshold, row_ptr, col, val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        pairs_plan pl;
        dev_guard dE;
        return pairs_run(
            ctx, what, ctx->pairs_stats, n <= 1, n, row_ptr, col, val, host_rows, cap, total,
            [&]() -> int {
                if (host_rows) ICL_TRY(icl_dev_upload(ctx, dE, E, (size_t)n * d * 4, "icl_pairs_within: E"));
                return pw_count_locked(ctx, host_rows ? (const float *)dE.p : E, size, n, d, threshold, row_ptr, total, pl);
            },
            [&](int32_t *d_col, float *d_val) { return pairs_fill_locked<pairs_tri>(ctx, pl, d_col, d_val, ctx->pairs_stats[2]); });
    });
}

static int pb_run(icl_ctx *ctx, const char *what, bool host_rows, const float *Q, const int32_t *q_size, int64_t nq, const float *L,
                  const int32_t *l_size, int64_t n, int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *col, float *val,
                  int64_t cap, int64_t *total)
{
    return no_throw(ctx, what, [&]() -> int {
        ICL_TRY(pb_check(ctx, what, Q, q_size, nq, L, l_size, n, d, threshold, exclude, row_ptr, col, val, cap, total));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        const bool empty = nq == 0 || n == 0;
        pairs_plan pl;
        if (!empty) ICL_TRY(pb_decide(ctx, what, nq, n, pl)); // (refused before the statistics are reset)
        dev_guard dQ, dL;
        return pairs_run(
            ctx, what, ctx->between_stats, empty, nq, row_ptr, col, val, host_rows, cap, total,
            [&]() -> int {
                if (host_rows) {
                    ICL_TRY(icl_dev_upload(ctx, dQ, Q, (size_t)nq * d * 4, "icl_pairs_between: Q"));
                    ICL_TRY(icl_dev_upload(ctx, dL, L, (size_t)n * d * 4, "icl_pairs_between: L"));
                }
                return pb_count_locked(ctx, host_rows ? (const float *)dQ.p : Q, q_size, nq, host_rows ? (const float *)dL.p : L, l_size, n, d,
                                       threshold, exclude, row_ptr, total, pl);
            },
            [&](int32_t *d_col, float *d_val) { return pairs_fill_locked<pairs_rect>(ctx, pl, d_col, d_val, ctx->between_stats[3]); });
    });
}

extern "C" int icl_pairs_within_dev(icl_ctx *ctx, const float *d_E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                                    int32_t *d_col, float *d_val, int64_t cap, int64_t *total)
{
    return pw_run(ctx, "icl_pairs_within_dev", false, d_E, size, n, d, threshold, row_ptr, d_col, d_val, cap, total);
}

extern "C" int icl_pairs_within(icl_ctx *ctx, const float *E, const int32_t *size, int64_t n, int32_t d, float threshold, int64_t *row_ptr,
                                int32_t *col, float *val, int64_t cap, int64_t *total)
{
    return pw_run(ctx, "icl_pairs_within", true, E, size, n, d, threshold, row_ptr, col, val, cap, total);
}

extern "C" int icl_pairs_between_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_L, const int32_t *l_size,
                                     int64_t n, int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *d_col, float *d_val,
                                     int64_t cap, int64_t *total)
{
    return pb_run(ctx, "icl_pairs_between_dev", false, d_Q, q_size, nq, d_L, l_size, n, d, threshold, exclude, row_ptr, d_col, d_val, cap, total);
}

extern "C" int icl_pairs_between(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *L, const int32_t *l_size, int64_t n,
                                 int32_t d, float threshold, const int64_t *exclude, int64_t *row_ptr, int32_t *col, float *val, int64_t cap,
                                 int64_t *total)
{
    return pb_run(ctx, "icl_pairs_between", true, Q, q_size, nq, L, l_size, n, d, threshold, exclude, row_ptr, col, val, cap, total);
}

extern "C" int icl_pairs_within_from_matrix(const float *D, int64_t n, int64_t ld, float threshold, int64_t *row_ptr, int32_t *col, float *val,
                                            int64_t cap, int64_t *total)
{
    return pairs_within_from_matrix(D, n, ld, threshold, row_ptr, col, val, cap, total) ? ICL_ERR_ARG : ICL_OK;
}

extern "C" int icl_pairs_between_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, float threshold, const int64_t *exclude,
                                             int64_t *row_ptr, int32_t *col, float *val, int64_t cap, int64_t *total)
{
    return pairs_between_from_matrix(D, nq, n, ld, threshold, exclude, row_ptr, col, val, cap, total) ? ICL_ERR_ARG : ICL_OK;
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

static int pairs_stats_out(icl_ctx *ctx, const char *what, const int64_t *stats, int count, int64_t *info)
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "%s: null argument", what);
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < count; ++q) info[q] = stats[q];
    return ICL_OK;
}

extern "C" int icl_last_pairs_stats(icl_ctx *ctx, int64_t info[4]) { return pairs_stats_out(ctx, "icl_last_pairs_stats", ctx ? ctx->pairs_stats : nullptr, 4, info); }

extern "C" int icl_last_pairs_between_stats(icl_ctx *ctx, int64_t info[5])
{
    return pairs_stats_out(ctx, "icl_last_pairs_between_stats", ctx ? ctx->between_stats : nullptr, 5, info);
}
