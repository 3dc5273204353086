// ward_many.hip -- many small, independent PerformClusteringWithConstraints calls (clustering.go:198-284) in one call, exact mode:
// icl_cluster_many / icl_cluster_many_dev (include/imageclust.h).  The serving pattern of the reference: every request clusters its
// own few hundred images (d = 1000 + labels), so a loaded server holds many small problems at once.  DESIGN.md "Many small problems".
//
// Device.  Two routes, each an init kernel and a merge kernel with ONE WORKGROUP PER PROBLEM in the merge, largest problems first;
// workgroups share nothing and never wait for each other (no flags, no spins), so a launch is correct whatever the number of
// workgroups resident at a time.
//   * What both merge kernels share is said once: wm_slots (the per-slot LDS arrays: a per-row (min, argmin) cache, sizes, creation
//     ids; wm_slots_bytes, wm_carve), wm_block_min<WAVES>, and the first half of a step -- wm_select_pair: the lexicographic minimum of
//     (value, larger creation id, smaller creation id) over the live, size-compatible pairs, the reference's first strict minimum in
//     row-major order with its MaxFloat32 ban (ward.hip's header); wm_merge_pair: the log entry, the merged centroid
//     (clustering.go:37-40), sizes, ids, keys.
//   * What differs stays apart.  Small route (n <= cap): ward_many_init_kernel writes every problem's exact lower triangle
//     (ComputeInitialDistanceMatrix, clustering.go:61-73), one thread per pair; ward_many_merge_kernel keeps the triangle in LDS when it
//     fits (n <= 281, WM_LDS_MAX), forms the new cluster's row exactly (:76-96), one row per thread, and a thread rescans a row whose
//     cached partner died.  Mid route (cap < n <= WMM_CAP): see "the mid-size route" below.
//   * The four kernels themselves are in ward_many_kernels.h, included three times: as they are for problems that start from singletons,
//     once more for problems that start from SEED clusters (icl_cluster_many_seeded, "seeded clustering" at the end of this file), and
//     a third time for seeded problems with a KEEP-APART relation over their clusters (icl_cluster_many_apart, "constrained seeded
//     clustering" at the end of this file; the host rules are apart_bits.h).
// Host.  Every entry point, seeded or not, is wm_entry (checks, lock, device) around wm_run, which runs the stages wm_classify (k, status,
// wm_route of every problem), wm_make_plan (launch groups -- wm_group: the small route is one, the mid route's are cut under a workspace
// budget -- and the workspace layout), wm_enqueue (uploads, aligned copies, wm_run_group per group, one read-back of the one log slab),
// the large-N problems (ward.hip's icl_ward_cluster_exact: above WMM_CAP rows, a lone small problem, mid-size problems the policy
// leaves there, icl_set_many_options), wm_collect, wm_cout (C_out, seeded calls only: ward_many_cout_kernel), wm_lowest_failure.
// What the two routes' groups do differently on the host is the table wm_kind.
// What a seeded call does differently is in two places: wm_classify takes a problem's k, status and effective sizes from
// ward_seed_admit (ward_seeds.h, icl_cluster_seeded's rule too) and routes by wm_route_seeded, never to the large-N engine.
// What a constrained call does beyond that is in two places as well: wm_make_plan counts every problem's bit rows into its group's data
// region (wm_data_bytes), and wm_run_group expands them (ab_expand) and uploads them behind the head; every problem of such a call runs
// on the constrained kernels, with empty bit rows where it has no constraint.
// Cluster ids and ranks come from the merge log by ward_final_list (ward_seeds.h) whichever route a problem took: rows of one item
// each (through ward.hip's icl_ward_assign_ids), or the seeds with their sizes.
#pragma clang fp contract(off)

#include "apart_bits.h"
#include "icl_common.h"
#include "ward_value.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <numeric>

#define WM_THREADS 256
#define WM_WAVES (WM_THREADS / 64)
#define WM_LDS_MAX 163840 // 160 KiB per workgroup (MI355X)
// Problems with more rows take the large-N engine (DESIGN.md "Many small problems": one problem alone, the one-workgroup loop took 12 ms
// at n = 256 against 5.6 ms for the large-N engine, 151 ms against 10.5 ms at n = 512, where the triangle no longer fits in LDS).
// ICL_MANY_CAP overrides it (read once per process) for A/B runs and tests, up to 8192 (a thread owns at most 32 rows of a problem).
#define WM_CAP_DEFAULT 256
// A batch with fewer candidates for the one-workgroup route than this sends them to the large-N engine too: a lone problem runs faster
// on the whole GPU than on one CU (the same results either way).
#define WM_MIN_BATCH 2

struct wm_prob {
    const float *E; // row 0 of the problem's embeddings (16-byte aligned when d % 4 == 0)
    float *C;       // centroid scratch: n x d, row s = the merged cluster living in slot s
    float *tri;     // packed lower triangle in the global workspace: entry (i, j), i > j, at i (i - 1) / 2 + j (the mid route: the full
                    // n x n square, entry (a, b) at a n + b)
    int32_t n, d, max_size, T; // T: merges CalculateOptimalClusters asks for (clustering.go:220)
    int32_t *log;   // 2 T creation ids: (larger, smaller) per merge
    int32_t *nm;    // merges performed
    int32_t lds_tri; // 1: the merge kernel keeps the triangle in LDS
    int32_t pad;
};

static_assert(sizeof(wm_prob) % 8 == 0, "wm_prob is an array element");

// What a seeded problem (icl_cluster_many_seeded, DESIGN.md "Seeded clustering") has beside its wm_prob, in a table of its own so that
// the unseeded kernels' table keeps its layout: E holds the n seed centroids, and
struct wm_seed {
    const int32_t *size; // n effective sizes >= 1: a seed's item count, or the problem's max_size for a frozen seed (every pair banned)
    int32_t *fin;        // out, n entries: the creation id of the cluster living in slot s when the loop ended, -1 for a dead slot
};

__host__ __device__ static inline int64_t wm_tri_len(int64_t n) { return n * (n - 1) / 2; }

// The per-slot state both merge kernels keep in LDS, in this order; wm_slots_bytes and wm_carve are its only description.
struct wm_slots {
    uint64_t *rkey; // row t's best key (UINT64_MAX: none)
    int32_t *rarg;  // ... and the slot of its partner
    int32_t *sz;    // size of slot s's cluster, 0 when the slot is dead
    int32_t *cid;   // creation id of slot s's cluster: singleton i -> i, t-th merge -> n + t
    uint64_t *red_k; // reduction scratch of wm_block_min, one entry per wave (8-byte aligned: an odd n is padded by one slot)
    int32_t *red_r;
};
#define WM_SLOT_BYTES 20 // rkey + rarg + sz + cid of one slot
__host__ __device__ static inline int64_t wm_slots_bytes(int64_t n, int waves) { return (n + (n & 1)) * WM_SLOT_BYTES + waves * 12; }
__device__ __forceinline__ wm_slots wm_carve(unsigned char *base, int n, int waves)
{
    wm_slots S;
    S.rkey = reinterpret_cast<uint64_t *>(base);
    S.rarg = reinterpret_cast<int32_t *>(S.rkey + n);
    S.sz = S.rarg + n;
    S.cid = S.sz + n;
    S.red_k = reinterpret_cast<uint64_t *>(S.cid + n + (n & 1));
    S.red_r = reinterpret_cast<int32_t *>(S.red_k + waves);
    return S;
}
// LDS bytes of the small merge kernel for a problem of n rows: the slots (the route has always reserved 192 bytes behind the 20 n of
// the arrays; the triangle's place depends on it), then the triangle when it is kept there
#define WM_META_TAIL 192
static_assert(WM_META_TAIL >= WM_SLOT_BYTES + WM_WAVES * 12, "wm_meta_bytes(n) >= wm_slots_bytes(n, WM_WAVES)");
__host__ __device__ static inline int64_t wm_meta_bytes(int64_t n) { return (n * WM_SLOT_BYTES + WM_META_TAIL + 15) / 16 * 16; }
static inline int64_t wm_lds_bytes(int64_t n, bool tri) { return wm_meta_bytes(n) + (tri ? wm_tri_len(n) * 4 : 0); }

// key of an eligible pair: value bits (>= +0, below MaxFloat32), then the larger and the smaller creation id -- unsigned order is the
// reference's scan order (ward.hip's header)
__device__ __forceinline__ uint64_t wm_key(float v, int ca, int cb)
{
    const uint32_t hi = (uint32_t)(ca > cb ? ca : cb), lo = (uint32_t)(ca > cb ? cb : ca);
    return ((uint64_t)__float_as_uint(v) << 32) | (hi << 16) | lo;
}

// block-wide minimum of (key, slot) over WAVES waves; every thread returns it
template <int WAVES>
__device__ __forceinline__ void wm_block_min(uint64_t &k, int &r, uint64_t *sk, int *sr)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint64_t ok = __shfl_xor(k, off);
        const int orr = __shfl_xor(r, off);
        if (ok < k) {
            k = ok;
            r = orr;
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sk[w] = k;
        sr[w] = r;
    }
    __syncthreads();
    k = sk[0];
    r = sr[0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q)
        if (sk[q] < k) {
            k = sk[q];
            r = sr[q];
        }
    __syncthreads(); // the scratch is free for the next reduction
}

// centroid row of the cluster living in slot s: its embedding while it is a singleton, else the merged centroid written into the slot
__device__ __forceinline__ const float *wm_cent(const wm_prob &p, const int32_t *cid, int s)
{
    return (cid[s] >= p.n ? p.C : p.E) + (int64_t)s * p.d;
}

// First half of a merge step, the same on both routes: the reference's selection order and merge rule.
// FindClosestClusters (clustering.go:119-133) over the row caches: the slots of position i (the later cluster, shi) and of j (slo).
// false: (-1, -1), "No more clusters to merge" (:224-227).  Two barriers (wm_block_min's).
template <int THREADS>
__device__ __forceinline__ bool wm_select_pair(const wm_slots S, int n, int &shi, int &slo)
{
    uint64_t bk = ~0ull;
    int br = -1;
    for (int t = threadIdx.x; t < n; t += THREADS)
        if (S.rkey[t] < bk) {
            bk = S.rkey[t];
            br = t;
        }
    wm_block_min<THREADS / 64>(bk, br, S.red_k, S.red_r);
    if (bk == ~0ull) return false;
    const int bu = S.rarg[br];
    shi = S.cid[br] > S.cid[bu] ? br : bu;
    slo = shi == br ? bu : br;
    return true;
}

// The merge itself: log entry, MergeClusters(clusters[i], clusters[j]) (:236, :37-40) into the centroid row of slot slo, where the new
// cluster lives (shi dies), then sizes, ids and keys.  Returns the new cluster's size.  One barrier inside; the caller's next
// barrier publishes the bookkeeping.
template <int THREADS>
__device__ __forceinline__ int wm_merge_pair(const wm_prob &p, const wm_slots S, int step, int shi, int slo)
{
    const int sa = S.sz[shi], sb = S.sz[slo];
    if (threadIdx.x == 0) {
        p.log[2 * step] = S.cid[shi];
        p.log[2 * step + 1] = S.cid[slo];
    }
    {
        const float fa = (float)sa, fb = (float)sb, fs = (float)(sa + sb);
        const float *ca = wm_cent(p, S.cid, shi), *cb = wm_cent(p, S.cid, slo);
        float *out = p.C + (int64_t)slo * p.d;
        for (int k = threadIdx.x; k < p.d; k += THREADS) out[k] = ward_merge_elem(fa, ca[k], fb, cb[k], fs); // (each k read, then written, by one thread)
    }
    __syncthreads(); // every thread has read the old sizes, ids and centroids
    if (threadIdx.x == 0) {
        S.sz[shi] = 0;
        S.rkey[shi] = ~0ull;
        S.sz[slo] = sa + sb;
        S.cid[slo] = p.n + step;
    }
    return sa + sb;
}

// ---- the mid-size route: cap < n <= WMM_CAP rows, one workgroup per problem ----------------------------------------------------------
// The same selection order, ban, merge log and centroid rule as ward_many_merge_kernel; what differs is who does the work:
//   * the matrix is a full n x n square in the global workspace, written symmetrically, so a row rescan reads contiguous memory and
//     is done by one WAVE (coalesced), not one thread;
//   * the new cluster's row: the live, size-compatible rows are compacted into a list; every thread owns one row of the list and
//     keeps its running sum in a register while the workgroup walks k-chunks of WMM_KC floats.  Each chunk of the listed rows and of
//     the new centroid is loaded coalesced into LDS (row stride WMM_KC + 1 floats: 64 lanes reading 64 rows at one k hit 64
//     different banks), double-buffered: the loads of chunk c + 1 are in flight while chunk c is added, strictly in k order.
// Workgroups share nothing and never wait for each other, as in the small route.
#define WMM_CAP 2048
#ifndef WMM_THREADS
#define WMM_THREADS 512 // measured against 1024 threads with WMM_KC 8 (the same LDS): 512 is 5 to 36 % faster (DESIGN.md "Mid-size problems")
#endif
#define WMM_WAVES (WMM_THREADS / 64)
#ifndef WMM_KC
#define WMM_KC 16
#endif
#define WMM_STRIDE (WMM_KC + 1)
#define WMM_BUF (WMM_THREADS * WMM_STRIDE) // floats of one chunk buffer
static_assert(2 * WMM_CAP < 65536, "wm_key packs creation ids (below n + T < 2 n) into 16 bits each; the slot lists are uint16_t");
static_assert(WMM_KC % 4 == 0 && (2 * WMM_BUF * 4) % 16 == 0, "the centroid chunk is read as float4");
// ICL_MANY_MID_AUTO's crossover counts per band of n ([257, 512], [513, 1024], [1025, 2048]): the smallest measured batch at which
// the route beat the large-N engine by more than both spreads, ICL_MANY_MID_OFF and _ON alternating in one process on serving-shape
// problems (profiles/r10_cluster_many_mid_rate.json: it lost at 2, 8 and 24 problems and won at 3, 10 and 32).  0 would keep a band
// off the route.
#define WMM_AUTO_MIN_0 3
#define WMM_AUTO_MIN_1 10
#define WMM_AUTO_MIN_2 32
#define WMI_TILE 64
#define WMI_KC 16

#define WMM_CHUNK_BYTES ((2 * WMM_BUF + 2 * WMM_KC) * 4) // two chunk buffers, two chunks of the new centroid
// LDS bytes of the mid merge kernel: the chunk buffers, the slots, two counters, the list of rows to evaluate and the list of rows to
// rescan (uint16_t each)
__host__ __device__ static inline int64_t wmm_lds_bytes(int64_t n)
{
    return (WMM_CHUNK_BYTES + wm_slots_bytes(n, WMM_WAVES) + 8 + n * 4 + 15) / 16 * 16;
}

// the threads of a wave for which f holds append t to list (order within the list is arbitrary: every use of it is per row)
__device__ __forceinline__ void wmm_append(bool f, int t, int32_t *count, uint16_t *list)
{
    const uint64_t m = __ballot(f);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(count, (int32_t)__popcll(m)); // (LDS, this workgroup only)
    base = __shfl(base, 0);
    if (f) list[base + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)t;
}

// What a constrained seeded problem (icl_cluster_many_apart, DESIGN.md "Constrained seeded clustering") has beside its wm_prob: wm_seed's
// two members under the same names, and the keep-apart relation over the slots as bit rows (apart_bits.h) in the global workspace
struct wm_apart {
    const int32_t *size; // as wm_seed::size
    int32_t *fin;        // as wm_seed::fin
    uint32_t *bits;      // n rows of `words` words: bit u of row t set when the clusters living in slots t and u are apart
    int32_t words, pad;  // ab_words(n)
};
static_assert(sizeof(wm_apart) % 8 == 0, "wm_apart is an array element");

__device__ __forceinline__ bool wm_apart_bit(const uint32_t *row, int u) { return row[u >> 5] >> (u & 31) & 1u; }
// Row t's side of a merge of slots shi and slo into sn = slo: B(new, t) = B(shi, t) or B(slo, t).  When it holds, the bit for sn is set in
// row t (it is already unless only shi's was).  Called by the one thread that owns row t in this step; a slot never comes back to life, so
// nothing is ever cleared.
__device__ __forceinline__ bool wm_apart_inherit(uint32_t *row, int shi, int slo)
{
    const bool hi = wm_apart_bit(row, shi), lo = wm_apart_bit(row, slo);
    if (hi && !lo) row[slo >> 5] |= 1u << (slo & 31);
    return hi || lo;
}
// ... and the new cluster's side: row(sn) |= row(shi), one word per thread
template <int THREADS>
__device__ __forceinline__ void wm_apart_or_row(uint32_t *bits, int words, int sn, int shi)
{
    uint32_t *dst = bits + (int64_t)sn * words;
    const uint32_t *src = bits + (int64_t)shi * words;
    for (int w = threadIdx.x; w < words; w += THREADS) dst[w] |= src[w];
}

// the kernels: from singletons, then from seeds, then from seeds with a keep-apart relation
#define WM_SEEDED 0
#define WM_APART 0
#include "ward_many_kernels.h"
#undef WM_SEEDED
#define WM_SEEDED 1
#include "ward_many_kernels.h"
#undef WM_APART
#define WM_APART 1
#include "ward_many_kernels.h"
#undef WM_APART
#undef WM_SEEDED

// C_out of the seeded calls: block b copies row src[b] (d[b] floats: a final cluster's centroid, from a problem's seed rows or its
// centroid scratch) to out + dst[b], or writes zeros there when src[b] is null
struct wm_crow {
    const float *src;
    int64_t dst;
    int32_t d, pad;
};
__global__ __launch_bounds__(256) void ward_many_cout_kernel(const wm_crow *__restrict__ R, float *__restrict__ out)
{
    const wm_crow r = R[blockIdx.x];
    float *o = out + r.dst;
    for (int k = threadIdx.x; k < r.d; k += 256) o[k] = r.src ? r.src[k] : 0.0f;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int icl_ward_cluster_exact(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int32_t *cluster_id,
                           int32_t *member_rank, int32_t *n_clusters, std::vector<int32_t> *merges); // ward.hip (ctx->mu held)
int icl_ward_assign_ids(icl_ctx *ctx, int64_t n, int32_t min_size, int32_t max_size, const int32_t *pairs, int64_t nmerge, int32_t *cluster_id,
                        int32_t *member_rank, int32_t *n_clusters); // ward.hip

static int64_t wm_cap()
{
    static const int64_t cap = [] {
        const char *s = getenv("ICL_MANY_CAP");
        const long v = s ? strtol(s, nullptr, 10) : WM_CAP_DEFAULT;
        return (int64_t)std::min<long>(std::max<long>(v, 0), 8192);
    }();
    return cap;
}

// The budget a group of mid-route problems stays under with its centroids and square matrices (wm_data_bytes): ICL_MANY_MID_WS_MB
// (read once per process; for A/B runs and tests), else WMM_WS_DEFAULT.
#define WMM_WS_DEFAULT ((size_t)8 << 30)
static size_t wmm_budget()
{
    static const size_t b = [] {
        const char *s = getenv("ICL_MANY_MID_WS_MB");
        const long long v = s ? strtoll(s, nullptr, 10) : 0;
        return v > 0 ? (size_t)v << 20 : WMM_WS_DEFAULT;
    }();
    return b;
}

// ICL_MANY_MID_AUTO: a problem of n rows takes the mid route when the call holds at least wmm_auto_min[band] problems of its band
// that could take it (one workgroup on one CU loses to the whole GPU for a lone problem; the bands and counts: see there)
#define WMM_BANDS 3
static inline int wmm_band(int64_t n) { return n <= 512 ? 0 : n <= 1024 ? 1 : 2; }
static const int64_t wmm_auto_min[WMM_BANDS] = {WMM_AUTO_MIN_0, WMM_AUTO_MIN_1, WMM_AUTO_MIN_2};
static bool wmm_auto_takes(int64_t n, const int64_t *band_count)
{
    const int b = wmm_band(n);
    return wmm_auto_min[b] > 0 && band_count[b] >= wmm_auto_min[b];
}

// what the ARG check of both entry points covers: nothing is written when it fails
static int wm_check_args(icl_ctx *ctx, const char *what, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *n,
                         const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank,
                         int32_t *n_clusters, int32_t *n_merges, int32_t *status)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "%s: null context", what);
    if (nprob < 0 || e_len < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: nprob %d, e_len %lld", what, nprob, (long long)e_len);
    if (nprob == 0) return ICL_OK;
    if (!e_off || !n || !d || !min_size || !max_size || !n_clusters || !n_merges || !status)
        return icl_fail(ctx, ICL_ERR_ARG, "%s: null per-problem array", what);
    int64_t rows = 0;
    bool any_e = false;
    for (int32_t p = 0; p < nprob; ++p) {
        if (n[p] < 0 || d[p] < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: problem %d has n %d, d %d", what, p, n[p], d[p]);
        const int64_t len = (int64_t)n[p] * d[p];
        if (e_off[p] < 0 || e_off[p] > e_len || len > e_len - e_off[p])
            return icl_fail(ctx, ICL_ERR_ARG, "%s: problem %d: rows [%lld, %lld) lie outside E (%lld floats)", what, p, (long long)e_off[p],
                            (long long)(e_off[p] + len), (long long)e_len);
        rows += n[p];
        any_e = any_e || len > 0;
    }
    if (rows >= ((int64_t)1 << 30)) return icl_fail(ctx, ICL_ERR_ARG, "%s: %lld rows in all", what, (long long)rows);
    if (rows && (!cluster_id || !member_rank)) return icl_fail(ctx, ICL_ERR_ARG, "%s: null cluster_id / member_rank", what);
    if (any_e && !E) return icl_fail(ctx, ICL_ERR_ARG, "%s: null E", what);
    return ICL_OK;
}

// the last icl_cluster's reports (icl_ctx::last): a problem on the large-N route must not change them
struct wm_last_guard {
    icl_ctx *c;
    icl_ward_report saved;
    explicit wm_last_guard(icl_ctx *ctx) : c(ctx), saved(std::move(ctx->last)) {}
    ~wm_last_guard() { c->last = std::move(saved); }
};

// WM_NONE: nothing to merge, or the constraints cannot be met; WM_SMALL: n <= cap, the small kernels; WM_LARGE: ward.hip's large-N
// engine, one problem at a time; WM_MID: cap < n <= WMM_CAP, the mid kernels
enum wm_route : int8_t { WM_NONE, WM_SMALL, WM_LARGE, WM_MID };

// What differs between the two one-workgroup routes.  init_blocks lists the init kernel's blocks for table entry g: (g, pair0) per 256
// pairs of the triangle, or (g, ti << 16 | tj) per pair of 64-row tiles, ti >= tj.  Both init kernels take (table, block problems,
// block arguments) and both merge kernels (table, order): pointers only, so one launch call serves either.
struct wm_kind {
    int64_t (*mat_bytes)(int64_t n);
    void (*init_blocks)(int32_t g, int64_t n, std::vector<int32_t> &prob, std::vector<int64_t> &arg);
    int arg_bytes; // of one init-block argument on the device
    bool (*lds_tri)(int64_t n);
    int64_t (*lds_bytes)(int64_t n); // dynamic LDS of the merge kernel
    const void *init_fn, *merge_fn;
    unsigned init_threads, merge_threads;
    bool own_data; // its group has a data region of its own (the small route); else the groups share one, one after the other
    bool apart = false; // the constrained kernels: a wm_apart table, and every problem's bit rows in the group's data region
};
static const wm_kind wm_kind_small = {
    [](int64_t n) { return wm_tri_len(n) * 4; },
    [](int32_t g, int64_t n, std::vector<int32_t> &prob, std::vector<int64_t> &arg) {
        for (int64_t q = 0; q < wm_tri_len(n); q += WM_THREADS) prob.push_back(g), arg.push_back(q);
    },
    8,
    [](int64_t n) { return wm_lds_bytes(n, true) <= WM_LDS_MAX; },
    [](int64_t n) { return wm_lds_bytes(n, wm_lds_bytes(n, true) <= WM_LDS_MAX); },
    (const void *)ward_many_init_kernel, (const void *)ward_many_merge_kernel, WM_THREADS, WM_THREADS, true,
};
static const wm_kind wm_kind_mid = {
    [](int64_t n) { return n * n * 4; },
    [](int32_t g, int64_t n, std::vector<int32_t> &prob, std::vector<int64_t> &arg) {
        const int32_t nt = (int32_t)((n + WMI_TILE - 1) / WMI_TILE);
        for (int32_t ti = 0; ti < nt; ++ti)
            for (int32_t tj = 0; tj <= ti; ++tj) prob.push_back(g), arg.push_back(ti << 16 | tj);
    },
    4,
    [](int64_t) { return false; },
    [](int64_t n) { return wmm_lds_bytes(n); },
    (const void *)ward_many_mid_init_kernel, (const void *)ward_many_mid_merge_kernel, 256, WMM_THREADS, false,
};
// the seeded instantiations: the same shapes, block lists and LDS; their kernels take the wm_seed table as one more argument
static wm_kind wm_seeded_kind(wm_kind k, const void *init_fn, const void *merge_fn)
{
    k.init_fn = init_fn;
    k.merge_fn = merge_fn;
    return k;
}
static const wm_kind wm_kind_small_seeded = wm_seeded_kind(wm_kind_small, (const void *)ward_many_init_seeded_kernel, (const void *)ward_many_merge_seeded_kernel);
static const wm_kind wm_kind_mid_seeded = wm_seeded_kind(wm_kind_mid, (const void *)ward_many_mid_init_seeded_kernel, (const void *)ward_many_mid_merge_seeded_kernel);
// the constrained instantiations: the seeded ones with a wm_apart table in the wm_seed table's place
static wm_kind wm_apart_kind(wm_kind k, const void *init_fn, const void *merge_fn)
{
    k = wm_seeded_kind(k, init_fn, merge_fn);
    k.apart = true;
    return k;
}
static const wm_kind wm_kind_small_apart = wm_apart_kind(wm_kind_small, (const void *)ward_many_init_apart_kernel, (const void *)ward_many_merge_apart_kernel);
static const wm_kind wm_kind_mid_apart = wm_apart_kind(wm_kind_mid, (const void *)ward_many_mid_init_apart_kernel, (const void *)ward_many_mid_merge_apart_kernel);

// centroids + matrix of one problem in a group's data region (256-byte aligned pieces), and its bit rows where the kind has them
static size_t wm_bits_bytes(const wm_kind &k, int64_t n)
{
    icl_ws_layout R(256);
    if (k.apart) R.take(ab_table_bytes(n));
    return R.total;
}
static size_t wm_data_bytes(const wm_kind &k, int64_t n, int64_t d)
{
    icl_ws_layout R(256);
    R.take((size_t)(n * d * 4));
    R.take((size_t)k.mat_bytes(n));
    return R.total + wm_bits_bytes(k, n);
}

// A launch group: problems that run as one init launch and one merge launch, one workgroup each in the merge.  The small route is one
// group with a data region of its own; the mid route's groups use one shared region one after the other (the launches are ordered on
// the stream).
struct wm_group {
    const wm_kind *kind = nullptr;
    std::vector<int32_t> probs; // largest first
    std::vector<int32_t> blk_prob;
    std::vector<int64_t> blk_arg;
    size_t data_bytes = 0;
    size_t o_head = 0, o_data = 0; // in the workspace; the head: [problem table] [init-block arguments] [order] [init-block problems]
    std::vector<unsigned char> head;
    bool seeded = false;  // then the head goes on, 8-byte aligned: [wm_seed or wm_apart table] [effective seed sizes, problem after problem]
    size_t seed_rows = 0; // seeds of all its problems
    // a constrained group: every problem's bit rows (wm_bits_bytes each), one block at the start of its data region, uploaded behind the head
    size_t bit_bytes = 0;
    std::vector<uint32_t> bits;
    size_t seed_elem() const { return kind->apart ? sizeof(wm_apart) : sizeof(wm_seed); }
    size_t plain_bytes() const { return sizeof(wm_prob) * probs.size() + (size_t)kind->arg_bytes * blk_arg.size() + 4 * (probs.size() + blk_prob.size()); }
    size_t o_seed() const { return (plain_bytes() + 7) / 8 * 8; }
    size_t head_bytes() const { return seeded ? o_seed() + seed_elem() * probs.size() + 4 * seed_rows : plain_bytes(); }
};

// the per-problem arguments of every entry point
struct wm_args {
    int32_t nprob;
    const int64_t *e_off;
    const int32_t *n, *d, *min_size, *max_size;
    // the seeded calls (n[p] is the number of seeds m): seed_size as the caller gave it, k_target (may be null), and whether C_out is
    // wanted (then every problem's rows are on the device and a mid-route problem's centroid scratch outlives its group)
    bool seeded = false;
    const int32_t *seed_size = nullptr, *k_target = nullptr;
    bool want_cout = false, cout_host = false;
    // the constrained seeded calls: apart_class (seed layout; may be null), pair_off (nprob + 1 offsets in pairs) and apart_pairs (both may be null)
    bool apart = false;
    const int32_t *apart_class = nullptr;
    const int64_t *pair_off = nullptr;
    const int32_t *apart_pairs = nullptr;
    const char *what() const { return apart ? "icl_cluster_many_apart" : seeded ? "icl_cluster_many_seeded" : "icl_cluster_many"; } // (in front of a failed problem's reason)
};
// ... and the outputs: rank is member_rank or seed_rank; C_out (seeded calls; may be null) on the device for a _dev call, on the host else;
// lowest (may be null): see cluster_many_locked in icl_common.h
struct wm_out {
    int32_t *cluster_id, *rank, *n_clusters, *n_merges, *merges, *status;
    float *C_out = nullptr;
    icl_item_failure *lowest = nullptr;
};

struct wm_plan {
    std::vector<int64_t> img, k; // first image of problem p; clusters CalculateOptimalClusters asks for
    std::vector<int32_t> st;
    std::vector<std::string> why;
    std::vector<wm_route> route;
    bool need_e = false;
    std::vector<wm_group> groups; // the small group (if any), then the mid groups
    std::vector<int64_t> log_at;  // problem p's log in the slab: 2 (n - k) ids, the count at 2 n
    int64_t log_ints = 0;
    std::vector<size_t> o_al; // problems whose rows the float4 loads cannot read in place: a 16-byte aligned copy
    size_t o_e = 0, o_logs = 0, ws_bytes = 0;
    // seeded calls: every seed's effective size (wm_seed::size), first seed of problem p at img[p], and the problem's clamped max_size
    // (a pair of unfrozen clusters never holds more than N items, so the clamp bans none of them); with C_out: the centroid scratch of a
    // mid-route problem outside its group's shared region, every problem's centroid scratch as wm_run_group placed it, the table of
    // ward_many_cout_kernel and, for the host call, the device copy of C_out
    std::vector<int32_t> eff, kmax; // (kmax: the max_size the seeded kernels see, clamped to [1, N] so that a frozen seed's size fits)
    std::vector<size_t> o_c;
    std::vector<const float *> c_dev;
    size_t o_crow = 0, o_cout = 0;
    std::vector<int32_t> finals; // (creation id, rank-0 seed) of every final cluster (ward_final_list), problem p's from fin_at[p] to fin_at[p + 1]
    std::vector<size_t> fin_at;
};

// The routes of the problems that have something to merge.  From singletons: small up to the cap, else the large-N engine, which also takes
// a lone small problem; the mid route takes what icl_set_many_options and the band counts give it.
static void wm_route_plain(const icl_ctx *ctx, const wm_args &A, wm_plan &pl, std::vector<int32_t> &small, std::vector<int32_t> &mid)
{
    const int64_t cap = wm_cap();
    auto mid_size = [&](int32_t p) { return A.n[p] > cap && A.n[p] <= WMM_CAP; };
    int64_t mid_band[WMM_BANDS] = {};
    for (int32_t p = 0; p < A.nprob; ++p) {
        if (pl.st[p] != ICL_OK || A.n[p] - pl.k[p] <= 0) continue;
        pl.route[p] = A.n[p] <= cap ? WM_SMALL : WM_LARGE;
        if (pl.route[p] == WM_SMALL) small.push_back(p);
        if (mid_size(p)) ++mid_band[wmm_band(A.n[p])];
    }
    if ((int64_t)small.size() < WM_MIN_BATCH) {
        for (int32_t p : small) pl.route[p] = WM_LARGE;
        small.clear();
    }
    if (ctx->many_mid != ICL_MANY_MID_OFF)
        for (int32_t p = 0; p < A.nprob; ++p)
            if (pl.route[p] == WM_LARGE && mid_size(p) && (ctx->many_mid == ICL_MANY_MID_ON || wmm_auto_takes(A.n[p], mid_band))) {
                pl.route[p] = WM_MID;
                mid.push_back(p);
            }
}
// From seeds (DESIGN.md "Seeded clustering"), by the number of seeds alone: small up to the cap (a lone problem included), mid up to
// wm_seed_limit whatever icl_set_many_options says, never the large-N engine.
static int64_t wm_seed_limit() { return std::max<int64_t>(wm_cap(), WMM_CAP); }
static void wm_route_seeded(const wm_args &A, wm_plan &pl, std::vector<int32_t> &small, std::vector<int32_t> &mid)
{
    for (int32_t p = 0; p < A.nprob; ++p) {
        if (pl.st[p] != ICL_OK || A.n[p] - pl.k[p] <= 0) continue;
        pl.route[p] = A.n[p] <= wm_cap() ? WM_SMALL : WM_MID;
        (pl.route[p] == WM_SMALL ? small : mid).push_back(p);
    }
}

// k, status and route of every problem; many_stats.  A problem from singletons: k = CalculateOptimalClusters(n) (clustering.go:203-207).  A
// seeded one: ward_seed_admit (N = the seeds' items, k = k_target or CalculateOptimalClusters(N), the sizes the kernels see), and
// ICL_ERR_UNSUPPORTED above wm_seed_limit seeds.
static void wm_classify(icl_ctx *ctx, const wm_args &A, wm_plan &pl, std::vector<int32_t> &small, std::vector<int32_t> &mid)
{
    const int32_t nprob = A.nprob;
    pl.img.assign(nprob + 1, 0);
    pl.k.assign(nprob, 0);
    pl.why.resize(nprob);
    pl.st.assign(nprob, ICL_OK);
    pl.route.assign(nprob, WM_NONE);
    for (int32_t p = 0; p < nprob; ++p) pl.img[p + 1] = pl.img[p] + A.n[p];
    if (A.seeded) {
        pl.eff.assign((size_t)pl.img[nprob], 1);
        pl.c_dev.assign(nprob, nullptr);
        pl.kmax.assign(nprob, 1);
    }
    for (int32_t p = 0; p < nprob; ++p) {
        char b[200];
        if (A.seeded) {
            ward_admission a = ward_seed_admit(A.n[p], A.seed_size + pl.img[p], A.min_size[p], A.max_size[p], A.k_target ? A.k_target[p] : 0,
                                               pl.eff.data() + pl.img[p]);
            if (a.status != ICL_ERR_UNSUPPORTED && A.n[p] > wm_seed_limit()) { // (behind the admission's own refusals, ahead of its constraints)
                a.status = ICL_ERR_UNSUPPORTED;
                snprintf(b, sizeof b, "%lld seeds: a seeded problem holds at most %lld", (long long)A.n[p], (long long)wm_seed_limit());
                a.why = b;
            }
            pl.st[p] = a.status, pl.k[p] = a.k, pl.kmax[p] = a.kmax;
            pl.why[p].swap(a.why);
        } else if (icl_calc_optimal_clusters(A.n[p], A.min_size[p], A.max_size[p], &pl.k[p]) != ICL_OK) {
            pl.st[p] = ICL_ERR_CONSTRAINT;
            snprintf(b, sizeof b, "cannot satisfy cluster size constraints with total items (%d), minSize (%d), and maxSize (%d)", A.n[p],
                     A.min_size[p], A.max_size[p]);
            pl.why[p] = b;
        }
        pl.need_e = pl.need_e || (pl.st[p] == ICL_OK && A.n[p] - pl.k[p] > 0 && (int64_t)A.n[p] * A.d[p] > 0);
    }
    if (A.seeded) wm_route_seeded(A, pl, small, mid);
    else wm_route_plain(ctx, A, pl, small, mid);
    if (A.want_cout && pl.img[nprob] > 0) pl.need_e = true;
    ctx->many_stats[0] = (int64_t)small.size();
    ctx->many_stats[1] = (int64_t)mid.size();
    ctx->many_stats[2] = std::count(pl.route.begin(), pl.route.end(), WM_LARGE);
}

// the launch groups (the mid route's under the budget; a group holds at least one problem) and the workspace:
// [uploaded E] [aligned copies] [logs, counts] [head of every group] [the small group's data] [the mid groups' shared data]
static void wm_make_plan(icl_ctx *ctx, const wm_args &A, bool upload_e, int64_t e_len, std::vector<int32_t> &small, std::vector<int32_t> &mid, wm_plan &pl)
{
    auto larger = [&](int32_t a, int32_t b) { return A.n[a] > A.n[b]; }; // largest first, within and across groups
    std::stable_sort(small.begin(), small.end(), larger);
    std::stable_sort(mid.begin(), mid.end(), larger);
    auto add = [&](const wm_kind &kind, const std::vector<int32_t> &ps, size_t budget) {
        for (int32_t p : ps) {
            const size_t need = wm_data_bytes(kind, A.n[p], A.d[p]);
            if (pl.groups.empty() || pl.groups.back().kind != &kind || pl.groups.back().data_bytes + need > budget) {
                pl.groups.emplace_back();
                pl.groups.back().kind = &kind;
                pl.groups.back().seeded = A.seeded;
            }
            wm_group &g = pl.groups.back();
            kind.init_blocks((int32_t)g.probs.size(), A.n[p], g.blk_prob, g.blk_arg);
            g.probs.push_back(p);
            g.data_bytes += need;
            g.bit_bytes += wm_bits_bytes(kind, A.n[p]);
            g.seed_rows += (size_t)A.n[p];
        }
    };
    add(A.apart ? wm_kind_small_apart : A.seeded ? wm_kind_small_seeded : wm_kind_small, small, SIZE_MAX);
    add(A.apart ? wm_kind_mid_apart : A.seeded ? wm_kind_mid_seeded : wm_kind_mid, mid, wmm_budget());
    ctx->many_stats[3] = (int64_t)pl.groups.size() - (small.empty() ? 0 : 1);
    icl_ws_layout L(256); // 256-byte aligned pieces
    pl.o_e = upload_e && pl.need_e ? L.take((size_t)e_len * 4) : 0;
    pl.o_al.assign(A.nprob, SIZE_MAX);
    pl.log_at.assign(A.nprob, 0);
    for (int32_t p = 0; p < A.nprob; ++p) {
        if (pl.route[p] && A.d[p] % 4 == 0 && A.n[p] && A.e_off[p] % 4 != 0) pl.o_al[p] = L.take((size_t)A.n[p] * A.d[p] * 4);
        if (pl.route[p] == WM_SMALL || pl.route[p] == WM_MID) {
            pl.log_at[p] = pl.log_ints;
            pl.log_ints += 2 * (int64_t)A.n[p] + 1; // 2 (n - k) ids + the count
            if (A.seeded) pl.log_ints += A.n[p];    // ... + the slots' final ids (wm_seed::fin)
        }
    }
    pl.o_c.assign(A.nprob, SIZE_MAX);
    if (A.want_cout) {
        for (int32_t p : mid) pl.o_c[p] = L.take((size_t)A.n[p] * A.d[p] * 4);
        pl.o_crow = L.take(sizeof(wm_crow) * (size_t)std::max<int64_t>(pl.img[A.nprob], 1));
        if (A.cout_host) pl.o_cout = L.take((size_t)std::max<int64_t>(e_len, 1) * 4);
    }
    pl.o_logs = L.take(4 * (size_t)std::max<int64_t>(pl.log_ints, 1));
    size_t shared = 0;
    for (wm_group &g : pl.groups) {
        g.o_head = L.take(g.head_bytes());
        if (g.kind->own_data) g.o_data = L.take(g.data_bytes);
        else shared = std::max(shared, g.data_bytes);
    }
    const size_t o_shared = L.take(shared);
    for (wm_group &g : pl.groups)
        if (!g.kind->own_data) g.o_data = o_shared;
    pl.ws_bytes = L.total;
}

// the group's head (problem table with device addresses, init blocks, order) uploaded, then one init launch and one merge launch
static int wm_run_group(icl_ctx *ctx, const wm_args &A, wm_plan &pl, wm_group &g, char *ws, const std::vector<const float *> &rowsE)
{
    const size_t G = g.probs.size(), o_arg = sizeof(wm_prob) * G, o_ord = o_arg + (size_t)g.kind->arg_bytes * g.blk_arg.size();
    g.head.resize(g.head_bytes());
    wm_prob *tab = reinterpret_cast<wm_prob *>(g.head.data());
    int32_t *ord = reinterpret_cast<int32_t *>(g.head.data() + o_ord);
    unsigned char *stab = g.seeded ? g.head.data() + g.o_seed() : nullptr; // wm_seed or wm_apart entries
    size_t o_eff = g.o_seed() + g.seed_elem() * G; // (of the next problem's effective sizes, in the head)
    icl_ws_layout R(256); // the problems' places in the group's data region
    const size_t o_bits = g.o_data + R.take(g.bit_bytes);
    g.bits.resize(g.bit_bytes / 4);
    size_t bit_at = 0; // (of the next problem's bit rows, in the block)
    int64_t lds = 0;
    for (size_t i = 0; i < G; ++i) {
        const int32_t p = g.probs[i];
        float *C = (float *)(ws + g.o_data + R.take((size_t)A.n[p] * A.d[p] * 4));
        if (pl.o_c[p] != SIZE_MAX) C = (float *)(ws + pl.o_c[p]);
        if (g.seeded) {
            pl.c_dev[p] = C;
            memcpy(g.head.data() + o_eff, pl.eff.data() + pl.img[p], 4 * (size_t)A.n[p]);
            const wm_seed sd{(const int32_t *)(ws + g.o_head + o_eff), (int32_t *)(ws + pl.o_logs) + pl.log_at[p] + 2 * (int64_t)A.n[p] + 1};
            if (g.kind->apart) {
                const int64_t q0 = A.pair_off ? A.pair_off[p] : 0, q1 = A.pair_off ? A.pair_off[p + 1] : 0;
                ab_expand(A.n[p], A.apart_class ? A.apart_class + pl.img[p] : nullptr, q1 > q0 ? A.apart_pairs + 2 * q0 : nullptr, q1 - q0,
                          g.bits.data() + bit_at / 4);
                const wm_apart ap{sd.size, sd.fin, (uint32_t *)(ws + o_bits + bit_at), (int32_t)ab_words(A.n[p]), 0};
                memcpy(stab + sizeof ap * i, &ap, sizeof ap);
                bit_at += wm_bits_bytes(*g.kind, A.n[p]);
            } else {
                memcpy(stab + sizeof sd * i, &sd, sizeof sd);
            }
            o_eff += 4 * (size_t)A.n[p];
        }
        float *mat = (float *)(ws + g.o_data + R.take((size_t)g.kind->mat_bytes(A.n[p])));
        int32_t *log = (int32_t *)(ws + pl.o_logs) + pl.log_at[p];
        tab[i] = wm_prob{rowsE[p], C, mat, A.n[p], A.d[p], g.seeded ? pl.kmax[p] : A.max_size[p], (int32_t)(A.n[p] - pl.k[p]), log, log + 2 * (int64_t)A.n[p],
                         g.kind->lds_tri(A.n[p]) ? 1 : 0, 0};
        ord[i] = (int32_t)i; // (probs is sorted: largest first)
        lds = std::max(lds, g.kind->lds_bytes(A.n[p]));
    }
    for (size_t b = 0; b < g.blk_arg.size(); ++b) // (the low arg_bytes of a little-endian int64_t)
        memcpy(g.head.data() + o_arg + (size_t)g.kind->arg_bytes * b, &g.blk_arg[b], g.kind->arg_bytes);
    if (!g.blk_prob.empty()) memcpy(ord + G, g.blk_prob.data(), 4 * g.blk_prob.size());
    const char *tab_d = ws + g.o_head, *arg_d = tab_d + o_arg, *ord_d = tab_d + o_ord, *blk_d = ord_d + 4 * G;
    ICL_HIP(ctx, hipMemcpyAsync(ws + g.o_head, g.head.data(), g.head.size(), hipMemcpyHostToDevice, ctx->stream));
    if (g.bit_bytes) ICL_HIP(ctx, hipMemcpyAsync(ws + o_bits, g.bits.data(), g.bit_bytes, hipMemcpyHostToDevice, ctx->stream));
    const char *seed_d = tab_d + g.o_seed(); // (the seeded kernels' last argument; the others take three and two)
    void *init_args[] = {&tab_d, &blk_d, &arg_d, &seed_d}, *merge_args[] = {&tab_d, &ord_d, &seed_d};
    if (!g.blk_prob.empty())
        ICL_HIP(ctx, hipLaunchKernel(g.kind->init_fn, dim3((unsigned)g.blk_prob.size()), dim3(g.kind->init_threads), init_args, 0, ctx->stream));
    icl_lds_optin(ctx, g.kind->merge_fn, WM_LDS_MAX);
    ICL_HIP(ctx, hipLaunchKernel(g.kind->merge_fn, dim3((unsigned)G), dim3(g.kind->merge_threads), merge_args, (size_t)lds, ctx->stream));
    return ICL_OK;
}

// uploads, aligned copies, every group's launches, the read-back of the log slab: all on ctx->stream, not waited for
static int wm_enqueue(icl_ctx *ctx, const wm_args &A, wm_plan &pl, const float *d_E, const float *h_E, int64_t e_len, std::vector<const float *> &rowsE,
                      std::vector<int32_t> &slab)
{
    ICL_TRY(ctx->many.ensure(ctx, pl.ws_bytes, "icl_cluster_many: workspace", (size_t)1 << 20));
    char *ws = ctx->many.as<char>();
    if (h_E && pl.need_e) {
        ICL_HIP(ctx, hipMemcpyAsync(ws + pl.o_e, h_E, (size_t)e_len * 4, hipMemcpyHostToDevice, ctx->stream));
        d_E = (const float *)(ws + pl.o_e);
    }
    for (int32_t p = 0; p < A.nprob; ++p) {
        if (!pl.route[p]) continue;
        rowsE[p] = d_E + A.e_off[p];
        if (pl.o_al[p] != SIZE_MAX) {
            ICL_HIP(ctx, hipMemcpyAsync(ws + pl.o_al[p], rowsE[p], (size_t)A.n[p] * A.d[p] * 4, hipMemcpyDeviceToDevice, ctx->stream));
            rowsE[p] = (const float *)(ws + pl.o_al[p]);
        }
    }
    for (wm_group &g : pl.groups) ICL_TRY(wm_run_group(ctx, A, pl, g, ws, rowsE));
    slab.resize((size_t)std::max<int64_t>(pl.log_ints, 1));
    if (pl.log_ints) ICL_HIP(ctx, hipMemcpyAsync(slab.data(), ws + pl.o_logs, 4 * (size_t)pl.log_ints, hipMemcpyDeviceToHost, ctx->stream));
    return ICL_OK;
}

// Every problem's results: ids from its merge log -- the slab's, or the large-N engine's (big_log; that engine has written the ids) -- by
// ward_final_list (clustering.go:265-280; from singletons through icl_ward_assign_ids, which checks the largest cluster too), rows of -1 and
// zero merges for a failed problem, the merge logs, the statuses; a seeded call's final clusters for wm_cout.
static void wm_collect(icl_ctx *ctx, const wm_args &A, wm_plan &pl, const std::vector<int32_t> &slab, const std::vector<std::vector<int32_t>> &big_log,
                       const wm_out &O)
{
    std::vector<int32_t> fin;
    pl.fin_at.assign((size_t)A.nprob + 1, 0);
    for (int32_t p = 0; p < A.nprob; ++p) {
        int32_t *cid = O.cluster_id + pl.img[p], *rank = O.rank + pl.img[p];
        const int32_t *lg = nullptr; // the problem's log, nm pairs
        int64_t nm = 0;
        if (pl.route[p] == WM_LARGE) {
            lg = big_log[p].data();
            nm = (int64_t)big_log[p].size() / 2;
        } else if (pl.route[p] != WM_NONE) {
            lg = slab.data() + pl.log_at[p];
            nm = lg[2 * (int64_t)A.n[p]];
        }
        fin.clear();
        if (pl.st[p] == ICL_OK && pl.route[p] != WM_LARGE) {
            if (A.seeded) {
                const ward_list_result r = ward_final_list(A.n[p], A.seed_size + pl.img[p], A.min_size[p], lg, nm, cid, rank, &O.n_clusters[p], &fin);
                if (r.kind != ward_list_result::OK) { // (the kernel's own log: the sizes were checked with the arguments)
                    pl.st[p] = ICL_ERR_HIP;
                    pl.why[p] = ward_list_text(r);
                }
            } else if (const int rc = icl_ward_assign_ids(ctx, A.n[p], A.min_size[p], A.max_size[p], lg, nm, cid, rank, &O.n_clusters[p])) {
                pl.st[p] = rc;
                pl.why[p] = ctx->err;
            }
        }
        if (pl.st[p] != ICL_OK) {
            std::fill(cid, cid + A.n[p], -1);
            std::fill(rank, rank + A.n[p], -1);
            O.n_clusters[p] = 0;
            nm = 0;
            fin.clear();
        }
        O.n_merges[p] = (int32_t)nm;
        if (O.merges && nm) memcpy(O.merges + 2 * pl.img[p], lg, 8 * (size_t)nm);
        O.status[p] = pl.st[p];
        pl.finals.insert(pl.finals.end(), fin.begin(), fin.end());
        pl.fin_at[(size_t)p + 1] = pl.finals.size();
    }
}

// the lowest failed problem's error, once every problem has its results
static int wm_lowest_failure(icl_ctx *ctx, const wm_args &A, const wm_plan &pl, icl_item_failure *lowest)
{
    for (int32_t p = 0; p < A.nprob; ++p)
        if (pl.st[p] != ICL_OK) {
            if (lowest) *lowest = icl_item_failure{p, pl.st[p], pl.why[p]};
            return icl_fail(ctx, pl.st[p], "%s: problem %d: %s", A.what(), p, pl.why[p].c_str());
        }
    return ICL_OK;
}

// C_out of a seeded call, after wm_collect: one wm_crow per seed of the call -- the centroid of the final cluster whose rank-0 seed it is
// (a surviving seed's own row, or the centroid scratch of the slot the merged cluster lives in, wm_seed::fin), zeros else -- and
// ward_many_cout_kernel.  rowsE: every problem's rows on the device, routed or not.
static int wm_cout(icl_ctx *ctx, const wm_args &A, wm_plan &pl, const std::vector<int32_t> &slab, const std::vector<const float *> &rowsE, int64_t e_len,
                   const wm_out &O)
{
    std::vector<wm_crow> crow((size_t)pl.img[A.nprob]);
    if (crow.empty()) return ICL_OK;
    std::vector<int32_t> slot;
    for (int32_t p = 0; p < A.nprob; ++p) {
        const int64_t m = A.n[p], d = A.d[p], nm = O.n_merges[p];
        for (int64_t i = 0; i < m; ++i) crow[(size_t)(pl.img[p] + i)] = wm_crow{nullptr, A.e_off[p] + i * d, (int32_t)d, 0};
        if (pl.route[p] != WM_NONE) { // the slot a merged cluster lives in
            const int32_t *fin = slab.data() + pl.log_at[p] + 2 * m + 1;
            slot.assign((size_t)(m + nm), -1);
            for (int64_t s = 0; s < m; ++s)
                if (fin[s] >= 0 && fin[s] < m + nm) slot[fin[s]] = (int32_t)s;
        }
        for (size_t f = pl.fin_at[p]; f < pl.fin_at[(size_t)p + 1]; f += 2) {
            const int64_t c = pl.finals[f], first = pl.finals[f + 1];
            const float *src = nullptr;
            if (c < m) src = rowsE[p] + c * d;
            else if (slot[c] >= 0) src = pl.c_dev[p] + (int64_t)slot[c] * d;
            else {
                pl.st[p] = O.status[p] = ICL_ERR_HIP;
                pl.why[p] = "the final state names no slot for a merged cluster";
            }
            crow[(size_t)(pl.img[p] + first)].src = src;
        }
    }
    char *ws = ctx->many.as<char>();
    float *out = A.cout_host ? (float *)(ws + pl.o_cout) : O.C_out;
    ICL_HIP(ctx, hipMemcpyAsync(ws + pl.o_crow, crow.data(), sizeof(wm_crow) * crow.size(), hipMemcpyHostToDevice, ctx->stream));
    if (A.cout_host) ICL_HIP(ctx, hipMemsetAsync(out, 0, (size_t)e_len * 4, ctx->stream)); // (the padding between problems)
    const wm_crow *tab = (const wm_crow *)(ws + pl.o_crow);
    hipLaunchKernelGGL(ward_many_cout_kernel, dim3((unsigned)crow.size()), dim3(256), 0, ctx->stream, tab, out);
    ICL_HIP(ctx, hipGetLastError());
    if (A.cout_host) ICL_HIP(ctx, hipMemcpyAsync(O.C_out, out, (size_t)e_len * 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICL_OK;
}

// Every entry point, after the argument check, with ctx->mu held: the stages of this file's header.  d_E: the rows on the device (e_len
// floats); h_E: the host copy, uploaded into the workspace here, or nullptr.
static int wm_run(icl_ctx *ctx, wm_args A, const float *d_E, const float *h_E, int64_t e_len, const wm_out &O)
{
    A.want_cout = O.C_out != nullptr;
    A.cout_host = O.C_out != nullptr && h_E != nullptr;
    wm_plan pl;
    {
        std::vector<int32_t> small, mid;
        wm_classify(ctx, A, pl, small, mid);
        wm_make_plan(ctx, A, h_E != nullptr, e_len, small, mid, pl);
    }
    std::vector<const float *> rowsE(A.nprob, nullptr);
    std::vector<int32_t> slab;
    ICL_TRY(wm_enqueue(ctx, A, pl, d_E, h_E, e_len, rowsE, slab));
    if (A.want_cout) { // a problem that took no route: its rows where the call's E lies on the device
        const float *base = h_E && pl.need_e ? (const float *)(ctx->many.as<char>() + pl.o_e) : d_E;
        for (int32_t p = 0; p < A.nprob; ++p)
            if (!rowsE[p]) rowsE[p] = base + A.e_off[p];
    }
    // the large-N route, one problem at a time, behind the launches above (its reports of the last icl_cluster are restored)
    std::vector<std::vector<int32_t>> big_log(A.nprob);
    {
        wm_last_guard keep(ctx);
        for (int32_t p = 0; p < A.nprob; ++p) {
            if (pl.route[p] != WM_LARGE) continue;
            int32_t nc = 0;
            const int rc = icl_ward_cluster_exact(ctx, rowsE[p], A.n[p], A.d[p], A.min_size[p], A.max_size[p], O.cluster_id + pl.img[p], O.rank + pl.img[p],
                                                  &nc, &big_log[p]);
            O.n_clusters[p] = nc;
            if (rc != ICL_OK) {
                pl.st[p] = rc;
                pl.why[p] = ctx->err;
            }
        }
    }
    if (!pl.groups.empty()) ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    wm_collect(ctx, A, pl, slab, big_log, O);
    if (A.want_cout) ICL_TRY(wm_cout(ctx, A, pl, slab, rowsE, e_len, O));
    return wm_lowest_failure(ctx, A, pl, O.lowest);
}

// (Declared in icl_common.h: icl_cluster_requests, requests.hip, is the third caller.)
int cluster_many_locked(icl_ctx *ctx, int32_t nprob, const float *d_E, const float *h_E, int64_t e_len, const int64_t *e_off,
                               const int32_t *n, const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id,
                               int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status, icl_item_failure *lowest)
{
    return wm_run(ctx, wm_args{nprob, e_off, n, d, min_size, max_size}, d_E, h_E, e_len,
                  wm_out{cluster_id, member_rank, n_clusters, n_merges, merges, status, nullptr, lowest});
}

extern "C" int icl_set_many_options(icl_ctx *ctx, int mid_mode)
{
    if (!ctx || (mid_mode != ICL_MANY_MID_AUTO && mid_mode != ICL_MANY_MID_OFF && mid_mode != ICL_MANY_MID_ON))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_set_many_options: mid_mode must be ICL_MANY_MID_AUTO, ICL_MANY_MID_OFF or ICL_MANY_MID_ON");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->many_mid = mid_mode;
    return ICL_OK;
}

extern "C" int icl_last_many_stats(icl_ctx *ctx, int64_t *small, int64_t *mid, int64_t *large, int64_t *mid_groups)
{
    if (!ctx) return icl_fail(ctx, ICL_ERR_ARG, "icl_last_many_stats: null context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (small) *small = ctx->many_stats[0];
    if (mid) *mid = ctx->many_stats[1];
    if (large) *large = ctx->many_stats[2];
    if (mid_groups) *mid_groups = ctx->many_stats[3];
    return ICL_OK;
}

// The ARG check of the seeded entry points, beyond wm_check_args': nothing is written when it fails
static int wm_check_seeds(icl_ctx *ctx, const char *what, int32_t nprob, const int32_t *m, const int32_t *seed_size)
{
    int64_t rows = 0;
    for (int32_t p = 0; p < nprob; ++p) rows += m[p];
    if (rows && !seed_size) return icl_fail(ctx, ICL_ERR_ARG, "%s: null seed_size", what);
    for (int64_t i = 0; i < rows; ++i)
        if (!seed_size[i]) return icl_fail(ctx, ICL_ERR_ARG, "%s: seed_size[%lld] is 0", what, (long long)i);
    return ICL_OK;
}

// ... and of the constrained entry points, beyond both (apart_bits.h: ab_bad_arg)
static int wm_check_apart(icl_ctx *ctx, const char *what, const wm_args &A)
{
    if (!A.pair_off && A.apart_pairs) return icl_fail(ctx, ICL_ERR_ARG, "%s: apart_pairs without pair_off", what);
    int64_t rows = 0;
    for (int32_t p = 0; p < A.nprob; ++p) {
        const int64_t q0 = A.pair_off ? A.pair_off[p] : 0, q1 = A.pair_off ? A.pair_off[p + 1] : 0;
        if (q0 < 0 || q1 < q0) return icl_fail(ctx, ICL_ERR_ARG, "%s: problem %d: pair offsets %lld, %lld", what, p, (long long)q0, (long long)q1);
        if (q1 > q0 && !A.apart_pairs) return icl_fail(ctx, ICL_ERR_ARG, "%s: null apart_pairs", what);
        const std::string why = ab_bad_arg(A.n[p], A.apart_class ? A.apart_class + rows : nullptr, q1 > q0 ? A.apart_pairs + 2 * q0 : nullptr, q1 - q0);
        if (!why.empty()) return icl_fail(ctx, ICL_ERR_ARG, "%s: problem %d: %s", what, p, why.c_str());
        rows += A.n[p];
    }
    return ICL_OK;
}

// The entry points: the argument checks, the lock, the device, wm_run.  dev: E (and C_out) are on the device.
static int wm_entry(icl_ctx *ctx, bool dev, const char *what, const wm_args &A, const float *E, int64_t e_len, const wm_out &O)
{
    return no_throw(ctx, what, [&]() -> int {
        ICL_TRY(wm_check_args(ctx, what, A.nprob, E, e_len, A.e_off, A.n, A.d, A.min_size, A.max_size, O.cluster_id, O.rank, O.n_clusters, O.n_merges, O.status));
        if (A.seeded) {
            ICL_TRY(wm_check_seeds(ctx, what, A.nprob, A.n, A.seed_size));
            if (A.apart) ICL_TRY(wm_check_apart(ctx, what, A));
            if (A.nprob == 0) return ICL_OK;
        }
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        return wm_run(ctx, A, dev ? E : nullptr, dev ? nullptr : E, e_len, O);
    });
}

extern "C" int icl_cluster_many_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *n,
                                    const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank,
                                    int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status)
{
    return wm_entry(ctx, true, "icl_cluster_many_dev", wm_args{nprob, e_off, n, d, min_size, max_size}, d_E, e_len,
                    wm_out{cluster_id, member_rank, n_clusters, n_merges, merges, status});
}

extern "C" int icl_cluster_many(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *n, const int32_t *d,
                                const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters,
                                int32_t *n_merges, int32_t *merges, int32_t *status)
{
    return wm_entry(ctx, false, "icl_cluster_many", wm_args{nprob, e_off, n, d, min_size, max_size}, E, e_len,
                    wm_out{cluster_id, member_rank, n_clusters, n_merges, merges, status});
}

// ---- seeded clustering: resume the loop from existing clusters (DESIGN.md "Seeded clustering") ------------------------------------
extern "C" int icl_cluster_many_seeded_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *m,
                                           const int32_t *d, const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size,
                                           const int32_t *k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges,
                                           int32_t *merges, int32_t *status, float *d_C_out)
{
    return wm_entry(ctx, true, "icl_cluster_many_seeded_dev", wm_args{nprob, e_off, m, d, min_size, max_size, true, seed_size, k_target}, d_E, e_len,
                    wm_out{cluster_id, seed_rank, n_clusters, n_merges, merges, status, d_C_out});
}

extern "C" int icl_cluster_many_seeded(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *m,
                                       const int32_t *d, const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size,
                                       const int32_t *k_target, int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges,
                                       int32_t *merges, int32_t *status, float *C_out)
{
    return wm_entry(ctx, false, "icl_cluster_many_seeded", wm_args{nprob, e_off, m, d, min_size, max_size, true, seed_size, k_target}, E, e_len,
                    wm_out{cluster_id, seed_rank, n_clusters, n_merges, merges, status, C_out});
}

// ---- constrained seeded clustering: keep-apart pairs and classes (DESIGN.md "Constrained seeded clustering") ---------------------------
static wm_args wm_apart_args(int32_t nprob, const int64_t *e_off, const int32_t *m, const int32_t *d, const int32_t *seed_size, const int32_t *min_size,
                             const int32_t *max_size, const int32_t *k_target, const int32_t *apart_class, const int64_t *pair_off, const int32_t *apart_pairs)
{
    wm_args A{nprob, e_off, m, d, min_size, max_size, true, seed_size, k_target};
    A.apart = true;
    A.apart_class = apart_class, A.pair_off = pair_off, A.apart_pairs = apart_pairs;
    return A;
}

extern "C" int icl_cluster_many_apart_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *m,
                                          const int32_t *d, const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size,
                                          const int32_t *k_target, const int32_t *apart_class, const int64_t *pair_off, const int32_t *apart_pairs,
                                          int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status,
                                          float *d_C_out)
{
    return wm_entry(ctx, true, "icl_cluster_many_apart_dev",
                    wm_apart_args(nprob, e_off, m, d, seed_size, min_size, max_size, k_target, apart_class, pair_off, apart_pairs), d_E, e_len,
                    wm_out{cluster_id, seed_rank, n_clusters, n_merges, merges, status, d_C_out});
}

extern "C" int icl_cluster_many_apart(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *m, const int32_t *d,
                                      const int32_t *seed_size, const int32_t *min_size, const int32_t *max_size, const int32_t *k_target,
                                      const int32_t *apart_class, const int64_t *pair_off, const int32_t *apart_pairs, int32_t *cluster_id,
                                      int32_t *seed_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status, float *C_out)
{
    return wm_entry(ctx, false, "icl_cluster_many_apart",
                    wm_apart_args(nprob, e_off, m, d, seed_size, min_size, max_size, k_target, apart_class, pair_off, apart_pairs), E, e_len,
                    wm_out{cluster_id, seed_rank, n_clusters, n_merges, merges, status, C_out});
}

// the final-list rule of the seeded calls (ward_final_list) for callers that hold a log of their own
extern "C" int icl_seeded_assign_ids(int32_t m, const int32_t *seed_size, int32_t min_size, const int32_t *merges, int32_t n_merges,
                                     int32_t *cluster_id, int32_t *seed_rank, int32_t *n_clusters)
{
    return no_throw(nullptr, "icl_seeded_assign_ids", [&]() -> int {
        if (m < 0 || n_merges < 0 || !n_clusters || (m && (!seed_size || !cluster_id || !seed_rank)) || (n_merges && !merges))
            return icl_fail(nullptr, ICL_ERR_ARG, "icl_seeded_assign_ids: m %d, n_merges %d or a null array", m, n_merges);
        const ward_list_result r = ward_final_list(m, seed_size, min_size, merges, n_merges, cluster_id, seed_rank, n_clusters, nullptr); // (writes nothing unless OK)
        return r.kind == ward_list_result::OK ? ICL_OK : icl_fail(nullptr, ICL_ERR_ARG, "icl_seeded_assign_ids: %s", ward_list_text(r).c_str());
    });
}
