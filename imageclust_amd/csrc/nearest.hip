// nearest.hip -- icl_nearest: for each query row the k library rows of smallest WardDistance, exact, with no distance matrix.
//
// Values are the reference's (clustering.go:136-157; ward_value.h), from the exact tile ward_dist_exact_kernel (ward.hip) runs, here on
// a rectangle (ward_exact_tile.h): 128 query rows x 128 library rows per tile, k-chunks of both operands staged in LDS, an 8 x 8 block
// of accumulators per thread, each accumulator one strictly sequential chain.  A workgroup owns a BAND of 128 query rows and walks its share of the
// library's column tiles; each row's k best (value, j) stay in LDS from the first tile to the last, a finished tile goes through LDS a
// quarter at a time into them, and nothing of size nq x n is ever written.  With few bands and a large library the column tiles are
// SPLIT over several workgroups per band, each leaves a partial list, and nearest_merge_kernel joins them.  What a list keeps and in
// which order is decided by nearest_select.h alone, on the host (icl_nearest_from_matrix) as on the device.
// Compiled with -ffp-contract=off -fno-slp-vectorize like ward.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"
#include "nearest_select.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile
#include "ward_value.h"

#include <algorithm>
#include <cstring>

#define NR_STAGE (2 * DT_KC * DT_LD) // floats of the two operand chunks; the finished tile's quarters reuse them
#define NR_SUB 64                    // a quarter: 64 rows x 64 columns ...
#define NR_SUB_LD 65                 // ... at an odd pitch (64 * 65 <= NR_STAGE): the selecting lanes, one per row, hit distinct banks
#define NR_MERGE_ROWS 64
#define NR_MAX_SPLITS 1024

static_assert(NR_SUB * NR_SUB_LD <= NR_STAGE, "a quarter tile must fit the operand staging area");
static_assert(NS_KMAX == 64, "the LDS budget below is worked out for k <= 64");

struct nr_args {
    const float *Q, *E;
    const int32_t *qs, *es, *ex; // device copies of q_size, e_size, exclude (any may be null: all 1 / all 1 / none)
    int64_t nq, n;
    int d, k, max_size, vec;
    int64_t ntiles, nbands;
    int splits;
    float *val; // [splits][nq][k]: the result itself when splits == 1, else the partial lists
    int32_t *idx;
};

// floats of dynamic LDS: operand chunks, the band's lists (pitch k | 1: a row per lane, distinct banks), per-row counts, the band's
// row sizes, the tile's column sizes.  k = 64: 84 992 bytes of the 160 KiB.
static inline size_t nr_lds_bytes(int k) { return (size_t)(NR_STAGE + 2 * DT_TILE * (k | 1) + 3 * DT_TILE) * 4; }

__global__ __launch_bounds__(256) void nearest_tile_select_kernel(nr_args a)
{
    extern __shared__ __attribute__((aligned(16))) float nr_smem[];
    float(*As)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(nr_smem);
    float(*Bs)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(nr_smem + DT_KC * DT_LD);
    float *sub = nr_smem;
    const int k = a.k, ks = a.k | 1;
    float *lv = nr_smem + NR_STAGE;
    int32_t *lj = reinterpret_cast<int32_t *>(lv + DT_TILE * ks);
    int32_t *cnt = lj + DT_TILE * ks;
    int32_t *qsz = cnt + DT_TILE;
    int32_t *esz = qsz + DT_TILE;

    // workgroups of one split are neighbours: the bands that run together read the same library tiles at about the same time
    const int64_t band = (int64_t)blockIdx.x % a.nbands, split = (int64_t)blockIdx.x / a.nbands;
    const int64_t t_lo = split * a.ntiles / a.splits, t_hi = (split + 1) * a.ntiles / a.splits;
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    if (tid < DT_TILE) {
        cnt[tid] = 0;
        qsz[tid] = (a.qs && i0 + tid < a.nq) ? a.qs[i0 + tid] : 1;
    }
    __syncthreads();

    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * DT_TILE;
        if (tid < DT_TILE) esz[tid] = (a.es && j0 + tid < a.n) ? a.es[j0 + tid] : 1; // (read after the tile's barriers)

        float acc[8][8];
        ward_exact_tile(a.Q, a.nq, i0, a.E, a.n, j0, a.d, a.vec != 0, As, Bs, acc);

        // The finished tile, a quarter at a time: every thread scales its 4 x 4 values of the quarter (clustering.go:142-144) into the
        // staging area, then one lane per row offers the row's 64 values to the row's list.  The selecting lanes are every fourth
        // thread, so all four waves (SIMDs) take a share; the selection holds a handful of registers while acc stays live.
#pragma unroll
        for (int ah = 0; ah < 2; ++ah)
#pragma unroll
            for (int bh = 0; bh < 2; ++bh) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int sa = qsz[ah * 64 + ty * 4 + r];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        sub[(ty * 4 + r) * NR_SUB_LD + tx * 4 + c] = ward_scale(acc[ah * 4 + r][bh * 4 + c], sa, esz[bh * 64 + tx * 4 + c]);
                }
                __syncthreads();
                if ((tid & 3) == 0) {
                    const int row = ah * 64 + (tid >> 2);
                    const int64_t i = i0 + row;
                    if (i < a.nq) {
                        const int64_t ex = a.ex ? (int64_t)a.ex[i] : -1;
                        const int sq = qsz[row];
                        float *rv = lv + row * ks;
                        int32_t *rj = lj + row * ks;
                        int c = cnt[row];
                        const int64_t jb = j0 + bh * 64;
                        const int ncol = (int)(a.n - jb < NR_SUB ? (a.n - jb > 0 ? a.n - jb : 0) : NR_SUB);
                        for (int col = 0; col < ncol; ++col) {
                            if (ns_left_out(jb + col, ex, sq, esz[bh * 64 + col], a.max_size)) continue;
                            ns_insert(rv, rj, k, c, sub[(tid >> 2) * NR_SUB_LD + col], (int32_t)(jb + col));
                        }
                        cnt[row] = c;
                    }
                }
                __syncthreads();
            }
    }

    // the band's lists, short rows with their tails
    float *ov = a.val + (split * a.nq + i0) * k;
    int32_t *oj = a.idx + (split * a.nq + i0) * k;
    const int rows = (int)(a.nq - i0 < DT_TILE ? a.nq - i0 : DT_TILE);
    for (int e = tid; e < rows * k; e += 256) {
        const int row = e / k, p = e - row * k;
        const bool have = p < cnt[row];
        ov[e] = have ? lv[row * ks + p] : NS_MAXF;
        oj[e] = have ? lj[row * ks + p] : -1;
    }
}

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

// The split count, decided here and nowhere else.  A forced count (icl_set_nearest_options) holds up to one tile per split.  Auto: the
// device has room for about two of these workgroups per CU; with that many bands or more every band walks the whole library, with
// fewer the tiles are dealt over as many workgroups per band as still run in one round.
static int nr_splits(const icl_ctx *ctx, int64_t nbands, int64_t ntiles)
{
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(ntiles, NR_MAX_SPLITS));
    if (ctx->nearest_splits > 0) return (int)std::min<int64_t>(ctx->nearest_splits, cap);
    const int64_t slots = 2 * (int64_t)std::max(1, ctx->prop.multiProcessorCount);
    if (nbands >= slots) return 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(slots / nbands, cap));
}

// For the other unit that walks bands this way (fit.hip): the same split decision, and the merge kernel as it is.
int nearest_splits(const icl_ctx *ctx, int64_t nbands, int64_t ntiles) { return nr_splits(ctx, nbands, ntiles); }

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
    const int64_t nbands = icl_ceil_div(nq, DT_TILE), ntiles = icl_ceil_div(n, DT_TILE);
    const int splits = nr_splits(ctx, nbands, ntiles);
    if (nbands * splits > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_nearest: grid too large (nq=%lld)", (long long)nq);
    // [q_size] [e_size] [exclude] [partial values] [partial indices], each on a 16-byte boundary; the first three go up in one copy
    icl_ws_layout L(16);
    const size_t o_qs = L.take(q_size ? (size_t)nq * 4 : 0), o_es = L.take(e_size ? (size_t)n * 4 : 0), o_ex = L.take(exclude ? (size_t)nq * 4 : 0);
    const size_t b_meta = L.total, b_part = splits > 1 ? (size_t)splits * nq * k * 4 : 0;
    const size_t o_val = L.take(b_part), o_idx = L.take(b_part), need = L.total;
    if (need) ICL_TRY(ctx->nearest.ensure(ctx, need, "icl_nearest: workspace"));
    char *ws = ctx->nearest.as<char>(); // (used only where need > 0)
    if (b_meta) {
        std::vector<int32_t> meta(b_meta / 4, 0);
        if (q_size) std::memcpy(meta.data(), q_size, (size_t)nq * 4);
        if (e_size) std::memcpy(meta.data() + o_es / 4, e_size, (size_t)n * 4);
        for (int64_t i = 0; exclude && i < nq; ++i) meta[o_ex / 4 + i] = (int32_t)exclude[i]; // (n < 2^31)
        // the caller's arrays and this vector may go away at return: a copy that has finished by then, ordered in front of the launch
        ICL_HIP(ctx, hipMemcpyAsync(ws, meta.data(), b_meta, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    nr_args a;
    a.Q = d_Q;
    a.E = d_E;
    a.qs = q_size ? (const int32_t *)(ws + o_qs) : nullptr;
    a.es = e_size ? (const int32_t *)(ws + o_es) : nullptr;
    a.ex = exclude ? (const int32_t *)(ws + o_ex) : nullptr;
    a.nq = nq;
    a.n = n;
    a.d = d;
    a.k = k;
    a.max_size = max_size;
    a.vec = (d & 3) == 0 && (((uintptr_t)d_Q | (uintptr_t)d_E) & 15) == 0;
    a.ntiles = ntiles;
    a.nbands = nbands;
    a.splits = splits;
    a.val = splits > 1 ? (float *)(ws + o_val) : d_val;
    a.idx = splits > 1 ? (int32_t *)(ws + o_idx) : d_idx;
    icl_lds_optin(ctx, (const void *)nearest_tile_select_kernel, (int)nr_lds_bytes(NS_KMAX));
    hipLaunchKernelGGL(nearest_tile_select_kernel, dim3((unsigned)(nbands * splits)), dim3(256), nr_lds_bytes(k), ctx->stream, a);
    ICL_HIP(ctx, hipGetLastError());
    if (splits > 1) ICL_TRY(nearest_merge_launch(ctx, a.val, a.idx, nq, k, splits, d_val, d_idx));
    ctx->nearest_stats[0] = splits;
    ctx->nearest_stats[1] = nbands * ntiles;
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
