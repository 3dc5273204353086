// fit.hip -- icl_cluster_fit: how well each clustered row sits in its own cluster, and which other clusters would take it, exact,
// with no distance matrix; icl_ward_values_at: exact values of listed pairs.
//
// Values are the reference's (clustering.go:136-157; ward_value.h).  The band walk is band_select.h's, with this unit's policy: a
// frozen column scales with its item count and is left out, and the lane that selects for row i stores the value of column
// cluster_of[i] to own[i] before it leaves that column out.  A column lies in exactly one tile and a tile belongs to exactly one
// split, so own[i] has ONE writer in the whole launch: a plain store, no atomic, no partial array.  fit_reduce_kernel then finds each
// cluster's representative and worst row with integer atomics on packed keys (fit_select.h): a minimum and a maximum over a total
// order, so arrival order cannot show.
// Compiled with -ffp-contract=off -fno-slp-vectorize like nearest.hip: every difference, product and sum is rounded on its own.
#pragma clang fp contract(off)

#include "band_select.h"
#include "fit_select.h"

#define FT_ROWS 256       // rows per workgroup of the reduction kernels
#define VA_PAIRS 64       // pairs per wave of ward_values_at_kernel: one per lane
#define VA_KC 128         // k per chunk: two coalesced 256-byte loads of each row
#define VA_LD (VA_KC + 1) // odd pitch: lane p walks row p of the chunk's products, distinct banks

struct ft_args : band_args { // E: the clusters' centroids, es: c_size (signed: a frozen column is negative), sel: cluster_of
    float *own;
    float *val;
    int32_t *idx;
};

struct ft_policy {
    using args = ft_args;
    // a row of no cluster meets no own column: split 0 is the one writer of its own cost
    static __device__ __forceinline__ void band_start(const args &a, int64_t split, int64_t i0, int64_t r)
    {
        if (split == 0 && i0 + r < a.nq && a.sel[i0 + r] < 0) a.own[i0 + r] = NS_MAXF;
    }
    static __device__ __forceinline__ int items(int32_t c_size) { return (int)fs_items(c_size); }
    static __device__ __forceinline__ int row_key(const args &, int64_t) { return 0; }
    // the row's own column counted from this quarter's first (K < 2^31; negative for a row of no cluster); its value is the own cost
    // (ncol by reference: by value it is noundef to the optimiser and the two tests below fold into one, which moves the register allocation)
    static __device__ __forceinline__ int quarter_key(const args &a, int64_t i, int, int64_t jb, const int &ncol, const float *sub, int srow)
    {
        const int mine = a.sel[i] < 0 ? -1 : (int)(a.sel[i] - jb);
        if (mine >= 0 && mine < ncol) a.own[i] = sub[srow * BAND_SUB_LD + mine];
        return mine;
    }
    static __device__ __forceinline__ bool left_out(int64_t, int col, int mine, int q_size, int32_t c_size, int32_t max_size)
    {
        return fs_left_out(col, mine, q_size, c_size, max_size);
    }
};

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
    const bool walk = nq > 0 && k_alt > 0, keys = K > 0 && (d_rep || d_worst);
    band_plan plan; // (no walk: no splits, no tiles)
    if (walk) ICL_TRY(plan.decide(ctx, "icl_cluster_fit", nq, K, k_alt));
    // [q_size] [cluster_of] [c_size] [partial values] [partial indices] [rep keys] [worst keys], each on a 16-byte boundary
    icl_ws_upload up;
    const size_t o_qs = up.add(q_size, nq), o_cof = up.add(cluster_of, nq), o_cs = up.add(c_size, K), b_meta = up.L.total;
    const size_t o_val = up.L.take(plan.part_bytes), o_idx = up.L.take(plan.part_bytes);
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
        a.E = d_C;
        a.qs = qs;
        a.es = cs;
        a.sel = cof;
        a.nq = nq;
        a.n = K;
        a.d = d;
        a.k = k_alt;
        a.max_size = max_size;
        a.own = d_own;
        ICL_TRY(plan.run<ft_policy>(ctx, a, (float *)(ws + o_val), (int32_t *)(ws + o_idx), d_alt_val, d_alt_idx));
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
    ctx->fit_stats[0] = plan.splits;
    ctx->fit_stats[1] = plan.nbands * plan.ntiles;
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
    icl_ws_upload up; // [q_size] [e_size] [qi] [ej]
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
