// fit.hip -- icl_cluster_fit: how well each clustered row sits in its own cluster, and which other clusters would take it, exact,
// with no distance matrix; icl_ward_values_at: exact values of listed pairs.
//
// Values are the reference's (clustering.go:136-157; ward_value.h).  The band walk is nearest.hip's: a workgroup owns 128 query rows
// and walks its share of the library's 128-column tiles (ward_exact_tile.h), each row's k_alt best alternatives stay in LDS, a finished
// tile goes through LDS a quarter at a time.  One duty more in the epilogue: the lane that selects for row i stores the value of column
// cluster_of[i] to own[i] before it leaves that column out.  A column lies in exactly one tile and a tile belongs to exactly one
// split, so own[i] has ONE writer in the whole launch: a plain store, no atomic, no partial array.  The splits' partial lists are
// joined by nearest.hip's merge kernel.  fit_reduce_kernel then finds each cluster's representative and worst row with integer atomics
// on packed keys (fit_select.h): a minimum and a maximum over a total order, so arrival order cannot show.
// Compiled with -ffp-contract=off -fno-slp-vectorize like nearest.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "icl_common.h"
#include "fit_select.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile
#include "ward_value.h"

#include <algorithm>
#include <cstring>

#define FT_STAGE (2 * DT_KC * DT_LD) // floats of the two operand chunks; the finished tile's quarters reuse them
#define FT_SUB 64                    // a quarter: 64 rows x 64 columns ...
#define FT_SUB_LD 65                 // ... at an odd pitch: the selecting lanes, one per row, hit distinct banks
#define FT_ROWS 256                  // rows per workgroup of the reduction kernels
#define VA_PAIRS 64                  // pairs per wave of ward_values_at_kernel: one per lane
#define VA_KC 128                    // k per chunk: two coalesced 256-byte loads of each row
#define VA_LD (VA_KC + 1)            // odd pitch: lane p walks row p of the chunk's products, distinct banks

static_assert(FT_SUB * FT_SUB_LD <= FT_STAGE, "a quarter tile must fit the operand staging area");
static_assert(FS_KMAX == 64, "the LDS budget below is worked out for k_alt <= 64");

struct ft_args {
    const float *Q, *C;
    const int32_t *qs, *cs, *cof; // device copies of q_size, c_size (either may be null: all 1) and cluster_of
    int64_t nq, K;
    int d, k, max_size, vec;
    int64_t ntiles, nbands;
    int splits;
    float *own;
    float *val; // [splits][nq][k]: the result itself when splits == 1, else the partial lists
    int32_t *idx;
};

// floats of dynamic LDS, as nearest.hip lays them out: operand chunks, the band's lists (pitch k | 1), per-row counts, the band's row
// sizes, the tile's column sizes (signed: a frozen column is negative)
static inline size_t ft_lds_bytes(int k) { return (size_t)(FT_STAGE + 2 * DT_TILE * (k | 1) + 3 * DT_TILE) * 4; }

__global__ __launch_bounds__(256) void fit_tile_select_kernel(ft_args a)
{
    extern __shared__ __attribute__((aligned(16))) float ft_smem[];
    float(*As)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(ft_smem);
    float(*Bs)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(ft_smem + DT_KC * DT_LD);
    float *sub = ft_smem;
    const int k = a.k, ks = a.k | 1;
    float *lv = ft_smem + FT_STAGE;
    int32_t *lj = reinterpret_cast<int32_t *>(lv + DT_TILE * ks);
    int32_t *cnt = lj + DT_TILE * ks;
    int32_t *qsz = cnt + DT_TILE;
    int32_t *csz = qsz + DT_TILE;

    const int64_t band = (int64_t)blockIdx.x % a.nbands, split = (int64_t)blockIdx.x / a.nbands;
    const int64_t t_lo = split * a.ntiles / a.splits, t_hi = (split + 1) * a.ntiles / a.splits;
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    if (tid < DT_TILE) {
        cnt[tid] = 0;
        qsz[tid] = (a.qs && i0 + tid < a.nq) ? a.qs[i0 + tid] : 1;
        // a row of no cluster meets no own column: split 0 is the one writer of its own cost
        if (split == 0 && i0 + tid < a.nq && a.cof[i0 + tid] < 0) a.own[i0 + tid] = NS_MAXF;
    }
    __syncthreads();

    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * DT_TILE;
        if (tid < DT_TILE) csz[tid] = (a.cs && j0 + tid < a.K) ? a.cs[j0 + tid] : 1; // (read after the tile's barriers)

        float acc[8][8];
        ward_exact_tile(a.Q, a.nq, i0, a.C, a.K, j0, a.d, a.vec != 0, As, Bs, acc);

        // The finished tile, a quarter at a time, as in nearest_tile_select_kernel: every thread scales its 4 x 4 values of the quarter
        // (clustering.go:142-144; a frozen column with its item count) into the staging area, then one lane per row takes the row's
        // own cost if its column is here and offers the other columns to the row's list.
#pragma unroll
        for (int ah = 0; ah < 2; ++ah)
#pragma unroll
            for (int bh = 0; bh < 2; ++bh) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int sa = qsz[ah * 64 + ty * 4 + r];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        sub[(ty * 4 + r) * FT_SUB_LD + tx * 4 + c] =
                            ward_scale(acc[ah * 4 + r][bh * 4 + c], sa, (int)fs_items(csz[bh * 64 + tx * 4 + c]));
                }
                __syncthreads();
                if ((tid & 3) == 0) {
                    const int row = ah * 64 + (tid >> 2);
                    const int64_t i = i0 + row;
                    if (i < a.nq) {
                        const int sq = qsz[row];
                        float *rv = lv + row * ks;
                        int32_t *rj = lj + row * ks;
                        int c = cnt[row];
                        const int64_t jb = j0 + bh * 64;
                        const int ncol = (int)(a.K - jb < FT_SUB ? (a.K - jb > 0 ? a.K - jb : 0) : FT_SUB);
                        // the row's own column counted from this quarter's first (K < 2^31; negative for a row of no cluster)
                        const int mine = a.cof[i] < 0 ? -1 : (int)(a.cof[i] - jb);
                        if (mine >= 0 && mine < ncol) a.own[i] = sub[(tid >> 2) * FT_SUB_LD + mine];
                        for (int col = 0; col < ncol; ++col) {
                            if (fs_left_out(col, mine, sq, csz[bh * 64 + col], a.max_size)) continue;
                            ns_insert(rv, rj, k, c, sub[(tid >> 2) * FT_SUB_LD + col], (int32_t)(jb + col));
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

// Exact values of listed pairs: val[p] = WardDistance of row qi[p] of Q and row ej[p] of E.  Each value is one strictly sequential
// chain of d rounded additions, so the parallelism is over pairs: a workgroup is one wave and takes 64 pairs.  For each chunk of 128 k
// the lanes read both rows of every pair side by side (256 contiguous bytes per load) and leave the rounded products
// fl(fl(a - b)^2) in LDS; lane p then adds pair p's products in k order.  qi == null: qi[p] = p.  ej[p] < 0 (internal callers only:
// a row of no cluster): MaxFloat32.
__global__ __launch_bounds__(VA_PAIRS) void ward_values_at_kernel(const float *__restrict__ Q, const int32_t *__restrict__ qs,
                                                                 const float *__restrict__ E, const int32_t *__restrict__ es, int d,
                                                                 const int32_t *__restrict__ qi, const int32_t *__restrict__ ej, int64_t np,
                                                                 float *__restrict__ val)
{
    __shared__ float prod[VA_PAIRS * VA_LD];
    __shared__ int32_t pq[VA_PAIRS], pe[VA_PAIRS];
    const int lane = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * VA_PAIRS, p = p0 + lane;
    const int npw = (int)(np - p0 < VA_PAIRS ? np - p0 : VA_PAIRS);
    const int32_t my_q = p < np ? (qi ? qi[p] : (int32_t)p) : 0, my_e = p < np ? ej[p] : -1;
    pq[lane] = my_q;
    pe[lane] = my_e;
    __syncthreads();

    float s = 0.0f;
    for (int kc = 0; kc < d; kc += VA_KC) {
        const int k0 = kc + lane, k1 = kc + 64 + lane;
#pragma unroll 4
        for (int w = 0; w < npw; ++w) {
            const int32_t e = pe[w];
            if (e < 0) continue; // (the same for every lane)
            const float *x = Q + (int64_t)pq[w] * d, *y = E + (int64_t)e * d;
            if (k0 < d) {
                const float df = x[k0] - y[k0]; // clustering.go:139
                prod[w * VA_LD + lane] = df * df; // :154 product (rounded)
            }
            if (k1 < d) {
                const float df = x[k1] - y[k1];
                prod[w * VA_LD + 64 + lane] = df * df;
            }
        }
        __syncthreads();
        const int kn = d - kc < VA_KC ? d - kc : VA_KC;
        const float *mine = prod + lane * VA_LD;
#pragma unroll 8
        for (int kk = 0; kk < kn; ++kk) s = s + mine[kk]; // :154 sum (rounded), strictly in k order
        __syncthreads();
    }
    if (p < np) val[p] = my_e < 0 ? NS_MAXF : ward_scale(s, qs ? qs[my_q] : 1, es ? (int)fs_items(es[my_e]) : 1);
}

// Each row offers (own cost, row) to its cluster's two keys and counts itself.  Integer atomics over a total order: the result is
// the same whatever order the rows arrive in.
__global__ __launch_bounds__(FT_ROWS) void fit_reduce_kernel(const float *__restrict__ own, const int32_t *__restrict__ cof, int64_t nq,
                                                            unsigned long long *__restrict__ key_rep, unsigned long long *__restrict__ key_worst,
                                                            int32_t *__restrict__ listed)
{
    const int64_t i = (int64_t)blockIdx.x * FT_ROWS + threadIdx.x;
    if (i >= nq) return;
    const int32_t c = cof[i];
    if (c < 0) return;
    const float v = own[i];
    if (key_rep) atomicMin(key_rep + c, (unsigned long long)fs_key_rep(v, i));
    if (key_worst) atomicMax(key_worst + c, (unsigned long long)fs_key_worst(v, i));
    if (listed) atomicAdd(listed + c, 1);
}

// The rows the keys name (-1: nobody named the cluster).
__global__ __launch_bounds__(FT_ROWS) void fit_rows_of_keys_kernel(const unsigned long long *__restrict__ key_rep,
                                                                  const unsigned long long *__restrict__ key_worst, int64_t K,
                                                                  int32_t *__restrict__ rep, int32_t *__restrict__ worst)
{
    const int64_t j = (int64_t)blockIdx.x * FT_ROWS + threadIdx.x;
    if (j >= K) return;
    if (rep) rep[j] = fs_rep_row(key_rep[j]);
    if (worst) worst[j] = fs_worst_row(key_worst[j]);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// Host arrays into one workspace: their int32 copies go up in one transfer that has finished at return (the caller's arrays and the
// staging vector may go away then), ordered in front of the launches.
struct ft_upload {
    icl_ws_layout L{16};
    struct part {
        size_t at, bytes;
        const int32_t *host;
    };
    std::vector<part> parts;
    size_t add(const int32_t *host, int64_t count) // -> the array's offset (a null array takes no room)
    {
        const size_t at = L.take(host ? (size_t)count * 4 : 0);
        if (host && count) parts.push_back({at, (size_t)count * 4, host});
        return at;
    }
    int go(icl_ctx *ctx, char *ws, size_t bytes) // bytes: L.total as it was behind the last add
    {
        if (!bytes) return ICL_OK;
        std::vector<char> meta(bytes, 0);
        for (const part &pt : parts) std::memcpy(meta.data() + pt.at, pt.host, pt.bytes);
        ICL_HIP(ctx, hipMemcpyAsync(ws, meta.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    }
};

static void values_at_launch(icl_ctx *ctx, const float *d_Q, const int32_t *d_qs, const float *d_E, const int32_t *d_es, int d, const int32_t *d_qi,
                             const int32_t *d_ej, int64_t np, float *d_val)
{
    hipLaunchKernelGGL(ward_values_at_kernel, dim3((unsigned)icl_ceil_div(np, VA_PAIRS)), dim3(VA_PAIRS), 0, ctx->stream, d_Q, d_qs, d_E, d_es, d,
                       d_qi, d_ej, np, d_val);
}

// ctx->mu held, the device selected, the arguments checked, nq > 0 or K > 0.
static int cluster_fit_dev_locked(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const float *d_C,
                                  const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, int32_t max_size, float *d_own, int32_t *d_alt_idx,
                                  float *d_alt_val, int32_t *d_listed, int32_t *d_rep, int32_t *d_worst)
{
    const int64_t nbands = icl_ceil_div(nq, DT_TILE), ntiles = icl_ceil_div(K, DT_TILE);
    const bool walk = nq > 0 && k_alt > 0, keys = K > 0 && (d_rep || d_worst);
    const int splits = walk ? nearest_splits(ctx, nbands, ntiles) : 0;
    if (walk && nbands * splits > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_cluster_fit: grid too large (nq=%lld)", (long long)nq);
    // [q_size] [cluster_of] [c_size] [partial values] [partial indices] [rep keys] [worst keys], each on a 16-byte boundary
    ft_upload up;
    const size_t o_qs = up.add(q_size, nq), o_cof = up.add(cluster_of, nq), o_cs = up.add(c_size, K);
    const size_t b_meta = up.L.total, b_part = splits > 1 ? (size_t)splits * nq * k_alt * 4 : 0;
    const size_t o_val = up.L.take(b_part), o_idx = up.L.take(b_part);
    const size_t o_kr = up.L.take(keys ? (size_t)K * 8 : 0), o_kw = up.L.take(keys ? (size_t)K * 8 : 0), need = up.L.total;
    if (need) ICL_TRY(ctx->fit.ensure(ctx, need, "icl_cluster_fit: workspace"));
    char *ws = ctx->fit.as<char>(); // (used only where need > 0)
    ICL_TRY(up.go(ctx, ws, b_meta));
    const int32_t *qs = q_size && nq ? (const int32_t *)(ws + o_qs) : nullptr, *cs = c_size && K ? (const int32_t *)(ws + o_cs) : nullptr;
    const int32_t *cof = (const int32_t *)(ws + o_cof);
    int64_t pairs = 0;
    if (walk) {
        ft_args a;
        a.Q = d_Q;
        a.C = d_C;
        a.qs = qs;
        a.cs = cs;
        a.cof = cof;
        a.nq = nq;
        a.K = K;
        a.d = d;
        a.k = k_alt;
        a.max_size = max_size;
        a.vec = (d & 3) == 0 && (((uintptr_t)d_Q | (uintptr_t)d_C) & 15) == 0;
        a.ntiles = ntiles;
        a.nbands = nbands;
        a.splits = splits;
        a.own = d_own;
        a.val = splits > 1 ? (float *)(ws + o_val) : d_alt_val;
        a.idx = splits > 1 ? (int32_t *)(ws + o_idx) : d_alt_idx;
        icl_lds_optin(ctx, (const void *)fit_tile_select_kernel, (int)ft_lds_bytes(FS_KMAX));
        hipLaunchKernelGGL(fit_tile_select_kernel, dim3((unsigned)(nbands * splits)), dim3(256), ft_lds_bytes(k_alt), ctx->stream, a);
        ICL_HIP(ctx, hipGetLastError());
        if (splits > 1) ICL_TRY(nearest_merge_launch(ctx, a.val, a.idx, nq, k_alt, splits, d_alt_val, d_alt_idx));
        pairs = nq * K;
    } else if (nq > 0) {
        // no list to keep: a band's rows may name up to 128 different column tiles, so the own costs come as listed pairs (i, cluster_of[i])
        values_at_launch(ctx, d_Q, qs, d_C, cs, d, nullptr, cof, nq, d_own);
        ICL_HIP(ctx, hipGetLastError());
        for (int64_t i = 0; i < nq; ++i) pairs += cluster_of[i] >= 0;
    }
    if (K > 0 && (keys || d_listed)) {
        unsigned long long *kr = keys ? (unsigned long long *)(ws + o_kr) : nullptr, *kw = keys ? (unsigned long long *)(ws + o_kw) : nullptr;
        if (keys) {
            ICL_HIP(ctx, hipMemsetAsync(kr, 0xff, (size_t)K * 8, ctx->stream)); // FS_REP_EMPTY
            ICL_HIP(ctx, hipMemsetAsync(kw, 0, (size_t)K * 8, ctx->stream));    // FS_WORST_EMPTY
        }
        if (d_listed) ICL_HIP(ctx, hipMemsetAsync(d_listed, 0, (size_t)K * 4, ctx->stream));
        if (nq > 0) {
            hipLaunchKernelGGL(fit_reduce_kernel, dim3((unsigned)icl_ceil_div(nq, FT_ROWS)), dim3(FT_ROWS), 0, ctx->stream, (const float *)d_own, cof, nq,
                               d_rep ? kr : nullptr, d_worst ? kw : nullptr, d_listed);
            ICL_HIP(ctx, hipGetLastError());
        }
        if (keys) {
            hipLaunchKernelGGL(fit_rows_of_keys_kernel, dim3((unsigned)icl_ceil_div(K, FT_ROWS)), dim3(FT_ROWS), 0, ctx->stream,
                               (const unsigned long long *)kr, (const unsigned long long *)kw, K, d_rep, d_worst);
            ICL_HIP(ctx, hipGetLastError());
        }
    }
    ctx->fit_stats[0] = splits;
    ctx->fit_stats[1] = walk ? nbands * ntiles : 0;
    ctx->fit_stats[2] = pairs;
    ctx->fit_stats[3] = (int64_t)need;
    return ICL_OK;
}

static int fit_check(icl_ctx *ctx, const char *what, const void *Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const void *C,
                     const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, const void *own, const void *alt_idx, const void *alt_val)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = d < 1 ? "d must be at least 1" : fs_bad_arg(nq, K, k_alt, q_size, cluster_of, c_size);
    if (!why && ((nq > 0 && (!Q || !own || (k_alt > 0 && (!alt_idx || !alt_val)))) || (K > 0 && !C))) why = "a null pointer";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

extern "C" int icl_cluster_fit_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const float *d_C,
                                   const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, int32_t max_size, float *d_own, int32_t *d_alt_idx,
                                   float *d_alt_val, int32_t *d_listed, int32_t *d_rep, int32_t *d_worst)
{
    return no_throw(ctx, "icl_cluster_fit_dev", [&]() -> int {
        ICL_TRY(fit_check(ctx, "icl_cluster_fit_dev", d_Q, q_size, cluster_of, nq, d_C, c_size, K, d, k_alt, d_own, d_alt_idx, d_alt_val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->fit_stats) s = 0;
        if (nq == 0 && K == 0) return ICL_OK;
        return cluster_fit_dev_locked(ctx, d_Q, q_size, cluster_of, nq, d_C, c_size, K, d, k_alt, max_size, d_own, d_alt_idx, d_alt_val, d_listed, d_rep,
                                      d_worst);
    });
}

extern "C" int icl_cluster_fit(icl_ctx *ctx, const float *Q, const int32_t *q_size, const int32_t *cluster_of, int64_t nq, const float *C,
                               const int32_t *c_size, int64_t K, int32_t d, int32_t k_alt, int32_t max_size, float *own, int32_t *alt_idx,
                               float *alt_val, int32_t *listed, int32_t *rep, int32_t *worst)
{
    return no_throw(ctx, "icl_cluster_fit", [&]() -> int {
        ICL_TRY(fit_check(ctx, "icl_cluster_fit", Q, q_size, cluster_of, nq, C, c_size, K, d, k_alt, own, alt_idx, alt_val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        for (int64_t &s : ctx->fit_stats) s = 0;
        if (nq == 0 && K == 0) return ICL_OK;
        dev_guard dQ, dC, dO, dI, dV, dL, dR, dW;
        const size_t bo = (size_t)nq * 4, ba = (size_t)nq * k_alt * 4, bk = (size_t)K * 4;
        if (nq) ICL_TRY(icl_dev_upload(ctx, dQ, Q, (size_t)nq * d * 4, "icl_cluster_fit: Q"));
        if (K) ICL_TRY(icl_dev_upload(ctx, dC, C, (size_t)K * d * 4, "icl_cluster_fit: C"));
        if (nq) ICL_TRY(icl_dev_alloc(ctx, dO, bo, "icl_cluster_fit: own"));
        if (ba) ICL_TRY(icl_dev_alloc(ctx, dI, ba, "icl_cluster_fit: alt_idx"));
        if (ba) ICL_TRY(icl_dev_alloc(ctx, dV, ba, "icl_cluster_fit: alt_val"));
        if (K && listed) ICL_TRY(icl_dev_alloc(ctx, dL, bk, "icl_cluster_fit: listed"));
        if (K && rep) ICL_TRY(icl_dev_alloc(ctx, dR, bk, "icl_cluster_fit: rep"));
        if (K && worst) ICL_TRY(icl_dev_alloc(ctx, dW, bk, "icl_cluster_fit: worst"));
        ICL_TRY(cluster_fit_dev_locked(ctx, dQ.as<float>(), q_size, cluster_of, nq, dC.as<float>(), c_size, K, d, k_alt, max_size, dO.as<float>(),
                                       dI.as<int32_t>(), dV.as<float>(), dL.as<int32_t>(), dR.as<int32_t>(), dW.as<int32_t>()));
        if (nq) ICL_HIP(ctx, hipMemcpyAsync(own, dO.p, bo, hipMemcpyDeviceToHost, ctx->stream));
        if (ba) ICL_HIP(ctx, hipMemcpyAsync(alt_idx, dI.p, ba, hipMemcpyDeviceToHost, ctx->stream));
        if (ba) ICL_HIP(ctx, hipMemcpyAsync(alt_val, dV.p, ba, hipMemcpyDeviceToHost, ctx->stream));
        if (dL.p) ICL_HIP(ctx, hipMemcpyAsync(listed, dL.p, bk, hipMemcpyDeviceToHost, ctx->stream));
        if (dR.p) ICL_HIP(ctx, hipMemcpyAsync(rep, dR.p, bk, hipMemcpyDeviceToHost, ctx->stream));
        if (dW.p) ICL_HIP(ctx, hipMemcpyAsync(worst, dW.p, bk, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    });
}

extern "C" int icl_cluster_fit_from_matrix(const float *D, int64_t nq, int64_t K, int64_t ld, const int32_t *q_size, const int32_t *cluster_of,
                                           const int32_t *c_size, int32_t k_alt, int32_t max_size, float *own, int32_t *alt_idx, float *alt_val,
                                           int32_t *listed, int32_t *rep, int32_t *worst)
{
    return fs_fit_from_matrix(D, nq, K, ld, q_size, cluster_of, c_size, k_alt, max_size, own, alt_idx, alt_val, listed, rep, worst) ? ICL_OK
                                                                                                                                     : ICL_ERR_ARG;
}

extern "C" int icl_last_fit_stats(icl_ctx *ctx, int64_t info[4])
{
    if (!ctx || !info) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_fit_stats: null argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int q = 0; q < 4; ++q) info[q] = ctx->fit_stats[q];
    return ICL_OK;
}

// ---- listed pairs ---------------------------------------------------------------------------------------------------------------
static int values_at_check(icl_ctx *ctx, const char *what, const void *Q, const int32_t *q_size, int64_t nq, const void *E, const int32_t *e_size,
                           int64_t n, int32_t d, const int32_t *qi, const int32_t *ej, int64_t np, const void *val)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    const char *why = nullptr;
    if (d < 1) why = "d must be at least 1";
    else if (nq < 0 || n < 0 || np < 0) why = "negative nq, n or np";
    else if (nq >= (1LL << 31) || n >= (1LL << 31)) why = "nq and n must be below 2^31";
    else if (np > 0 && (!Q || !E || !qi || !ej || !val)) why = "a null pointer";
    for (int64_t i = 0; !why && q_size && i < nq; ++i)
        if (q_size[i] <= 0) why = "a q_size entry is not above 0";
    for (int64_t j = 0; !why && e_size && j < n; ++j)
        if (e_size[j] == 0) why = "an e_size entry is 0";
    for (int64_t p = 0; !why && p < np; ++p)
        if (qi[p] < 0 || qi[p] >= nq || ej[p] < 0 || ej[p] >= n) why = "a pair names a row that does not exist";
    if (why) return icl_fail(ctx, ICL_ERR_ARG, "%s: %s", what, why);
    if (ctx->shard) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: not on a replica of a group", what);
    return ICL_OK;
}

// ctx->mu held, the device selected, the arguments checked, np > 0.
static int values_at_dev_locked(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size, int64_t n,
                                int32_t d, const int32_t *qi, const int32_t *ej, int64_t np, float *d_val)
{
    if (icl_ceil_div(np, VA_PAIRS) > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_ward_values_at: grid too large (np=%lld)", (long long)np);
    ft_upload up; // [q_size] [e_size] [qi] [ej]
    const size_t o_qs = up.add(q_size, nq), o_es = up.add(e_size, n), o_qi = up.add(qi, np), o_ej = up.add(ej, np), need = up.L.total;
    ICL_TRY(ctx->fit.ensure(ctx, need, "icl_ward_values_at: workspace"));
    char *ws = ctx->fit.as<char>();
    ICL_TRY(up.go(ctx, ws, need));
    values_at_launch(ctx, d_Q, q_size ? (const int32_t *)(ws + o_qs) : nullptr, d_E, e_size ? (const int32_t *)(ws + o_es) : nullptr, d,
                     (const int32_t *)(ws + o_qi), (const int32_t *)(ws + o_ej), np, d_val);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

extern "C" int icl_ward_values_at_dev(icl_ctx *ctx, const float *d_Q, const int32_t *q_size, int64_t nq, const float *d_E, const int32_t *e_size,
                                      int64_t n, int32_t d, const int32_t *qi, const int32_t *ej, int64_t np, float *d_val)
{
    return no_throw(ctx, "icl_ward_values_at_dev", [&]() -> int {
        ICL_TRY(values_at_check(ctx, "icl_ward_values_at_dev", d_Q, q_size, nq, d_E, e_size, n, d, qi, ej, np, d_val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (np == 0) return ICL_OK;
        return values_at_dev_locked(ctx, d_Q, q_size, nq, d_E, e_size, n, d, qi, ej, np, d_val);
    });
}

extern "C" int icl_ward_values_at(icl_ctx *ctx, const float *Q, const int32_t *q_size, int64_t nq, const float *E, const int32_t *e_size, int64_t n,
                                  int32_t d, const int32_t *qi, const int32_t *ej, int64_t np, float *val)
{
    return no_throw(ctx, "icl_ward_values_at", [&]() -> int {
        ICL_TRY(values_at_check(ctx, "icl_ward_values_at", Q, q_size, nq, E, e_size, n, d, qi, ej, np, val));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (np == 0) return ICL_OK;
        dev_guard dQ, dE, dV;
        ICL_TRY(icl_dev_upload(ctx, dQ, Q, (size_t)nq * d * 4, "icl_ward_values_at: Q"));
        ICL_TRY(icl_dev_upload(ctx, dE, E, (size_t)n * d * 4, "icl_ward_values_at: E"));
        ICL_TRY(icl_dev_alloc(ctx, dV, (size_t)np * 4, "icl_ward_values_at: val"));
        ICL_TRY(values_at_dev_locked(ctx, dQ.as<float>(), q_size, nq, dE.as<float>(), e_size, n, d, qi, ej, np, dV.as<float>()));
        ICL_HIP(ctx, hipMemcpyAsync(val, dV.p, (size_t)np * 4, hipMemcpyDeviceToHost, ctx->stream));
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return ICL_OK;
    });
}
