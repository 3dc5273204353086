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
// Host.  cluster_many_locked runs the stages wm_classify (k, status, wm_route of every problem), wm_make_plan (launch groups --
// wm_group: the small route is one, the mid route's are cut under a workspace budget -- and the workspace layout), wm_enqueue (uploads,
// aligned copies, wm_run_group per group, one read-back of the one log slab), the large-N problems (ward.hip's
// icl_ward_cluster_exact: above WMM_CAP rows, a lone small problem, mid-size problems the policy leaves there, icl_set_many_options),
// wm_collect.  What the two routes' groups do differently on the host is the table wm_kind.
// Cluster ids and member ranks come from the merge log by ward.hip's rule (icl_ward_assign_ids) whichever route a problem took.
#pragma clang fp contract(off)

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

// ComputeInitialDistanceMatrix (clustering.go:61-73) of every problem: block b covers pairs [pair0[b], pair0[b] + 256) of problem prob[b]
__global__ __launch_bounds__(WM_THREADS) void ward_many_init_kernel(const wm_prob *__restrict__ P, const int32_t *__restrict__ blk_prob,
                                                                    const int64_t *__restrict__ blk_pair0)
{
    const wm_prob p = P[blk_prob[blockIdx.x]];
    const int64_t q = blk_pair0[blockIdx.x] + threadIdx.x;
    if (q >= wm_tri_len(p.n)) return;
    int64_t i = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5); // row i holds pairs [i (i - 1) / 2, i (i + 1) / 2)
    while (i * (i - 1) / 2 > q) --i;
    while ((i + 1) * i / 2 <= q) ++i;
    const int64_t j = q - i * (i - 1) / 2;
    float v = ICL_MAXF; // max_size < 2: every pair of singletons is banned (clustering.go:228-234) and never read
    if (p.max_size >= 2) v = ward_pair_value(p.E + i * p.d, p.E + j * p.d, p.d, 1, 1); // WardDistance(clusters[i], clusters[j]) :66
    p.tri[q] = v;
}

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

__global__ __launch_bounds__(WM_THREADS) void ward_many_merge_kernel(const wm_prob *__restrict__ P, const int32_t *__restrict__ order)
{
    extern __shared__ __align__(16) unsigned char wm_lds[];
    const wm_prob p = P[order[blockIdx.x]];
    const int n = p.n, d = p.d, maxs = p.max_size;
    const wm_slots S = wm_carve(wm_lds, n, WM_WAVES);
    uint64_t *const rkey = S.rkey;
    int32_t *const rarg = S.rarg, *const sz = S.sz, *const cid = S.cid;
    float *tri = p.tri;
    if (p.lds_tri) {
        float *lt = reinterpret_cast<float *>(wm_lds + wm_meta_bytes(n));
        const int64_t len = wm_tri_len(n);
        for (int64_t q = threadIdx.x; q < len; q += WM_THREADS) lt[q] = p.tri[q];
        tri = lt;
    }
    for (int t = threadIdx.x; t < n; t += WM_THREADS) {
        sz[t] = 1;
        cid[t] = t;
    }
    __syncthreads();
    auto cent = [&](int s) { return wm_cent(p, cid, s); };
    auto at = [&](int a, int b) -> float & { return a > b ? tri[a * (a - 1) / 2 + b] : tri[b * (b - 1) / 2 + a]; };
    // row t's minimum over every live, size-compatible partner below MaxFloat32 (NaN never is: clustering.go:126)
    auto scan = [&](int t) {
        uint64_t best = ~0ull;
        int arg = -1;
        const int st = sz[t], ct = cid[t];
        for (int u = 0; u < n; ++u) {
            const int su = sz[u];
            if (u == t || su == 0 || st + su > maxs) continue;
            const float v = at(t, u);
            if (!(v < ICL_MAXF)) continue;
            const uint64_t k = wm_key(v, ct, cid[u]);
            if (k < best) {
                best = k;
                arg = u;
            }
        }
        rkey[t] = best;
        rarg[t] = arg;
    };
    for (int t = threadIdx.x; t < n; t += WM_THREADS) scan(t);
    __syncthreads();
    int step = 0;
    for (; step < p.T; ++step) {
        int shi, slo;
        if (!wm_select_pair<WM_THREADS>(S, n, shi, slo)) break;
        const int sn = slo, snew = wm_merge_pair<WM_THREADS>(p, S, step, shi, slo), cnew = n + step;
        __syncthreads();
        // UpdateDistanceMatrix (:76-96): WardDistance(clusters[t], newCluster) for every live t; the owner of row t updates its cache
        const float *cn = p.C + (int64_t)sn * d;
        uint64_t nk = ~0ull;
        int nr = -1;
        uint32_t stale = 0; // rows of this thread whose cached partner just died
        for (int t = threadIdx.x, m = 0; t < n; t += WM_THREADS, ++m) {
            if (t == sn || sz[t] == 0) continue;
            const int st = sz[t];
            float v = ICL_MAXF; // banned: never selected (:228-234), never evaluated
            if (st + snew <= maxs) v = ward_pair_value(cent(t), cn, d, st, snew);
            at(t, sn) = v;
            const uint64_t k = (st + snew <= maxs && v < ICL_MAXF) ? wm_key(v, cid[t], cnew) : ~0ull;
            if (k < nk) {
                nk = k;
                nr = t;
            }
            if (rarg[t] == shi || rarg[t] == slo)
                stale |= 1u << m;
            else if (k < rkey[t]) {
                rkey[t] = k;
                rarg[t] = sn;
            }
        }
        wm_block_min<WM_WAVES>(nk, nr, S.red_k, S.red_r); // (its barriers also publish the new row)
        if (threadIdx.x == 0) {
            rkey[sn] = nk;
            rarg[sn] = nr;
        }
        for (int t = threadIdx.x, m = 0; t < n; t += WM_THREADS, ++m)
            if (stale >> m & 1u) scan(t);
        __syncthreads();
    }
    if (threadIdx.x == 0) *p.nm = step;
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

// ComputeInitialDistanceMatrix (clustering.go:61-73) into the full square: block b computes the 64 x 64 pairs (i, j) of tile
// (ti, tj), ti >= tj, of problem blk_prob[b]; k-chunks of both row sets are staged in LDS, every thread holds 4 x 4 pairs, and every
// pair's sum is s = s + fl(fl(x_k - y_k)^2) strictly in k order -- the value ward_pair_value(E_i, E_j, d, 1, 1) returns.
__global__ __launch_bounds__(256) void ward_many_mid_init_kernel(const wm_prob *__restrict__ P, const int32_t *__restrict__ blk_prob,
                                                                 const int32_t *__restrict__ blk_tile)
{
    __shared__ float A[WMI_TILE * (WMI_KC + 1)], B[WMI_TILE * (WMI_KC + 1)];
    const wm_prob p = P[blk_prob[blockIdx.x]];
    const int n = p.n, d = p.d, tid = threadIdx.x;
    const int i0 = (blk_tile[blockIdx.x] >> 16) * WMI_TILE, j0 = (blk_tile[blockIdx.x] & 0xffff) * WMI_TILE;
    const int tx = tid & 15, ty = tid >> 4;
    float s[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = 0.0f;
    if (p.max_size >= 2) {
        const bool vec = (d & 3) == 0;
        for (int k0 = 0; k0 < d; k0 += WMI_KC) {
            const int kc = min(WMI_KC, d - k0);
            __syncthreads(); // the previous chunk has been added
            if (vec) { // thread -> (row tid / 4, floats 4 (tid % 4) ...) of both row sets: 16-byte loads, 64 B per row
                const int r = tid >> 2, kk = (tid & 3) * 4;
                float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
                if (kk < kc) {
                    if (i0 + r < n) a = *reinterpret_cast<const float4 *>(p.E + (int64_t)(i0 + r) * d + k0 + kk);
                    if (j0 + r < n) b = *reinterpret_cast<const float4 *>(p.E + (int64_t)(j0 + r) * d + k0 + kk);
                }
                float *pa = A + r * (WMI_KC + 1) + kk, *pb = B + r * (WMI_KC + 1) + kk;
                pa[0] = a.x, pa[1] = a.y, pa[2] = a.z, pa[3] = a.w;
                pb[0] = b.x, pb[1] = b.y, pb[2] = b.z, pb[3] = b.w;
            } else {
#pragma unroll
                for (int q = 0; q < WMI_TILE * WMI_KC / 256; ++q) {
                    const int idx = tid + q * 256, r = idx / WMI_KC, kk = idx % WMI_KC;
                    float a = 0.f, b = 0.f;
                    if (kk < kc) {
                        if (i0 + r < n) a = p.E[(int64_t)(i0 + r) * d + k0 + kk];
                        if (j0 + r < n) b = p.E[(int64_t)(j0 + r) * d + k0 + kk];
                    }
                    A[r * (WMI_KC + 1) + kk] = a;
                    B[r * (WMI_KC + 1) + kk] = b;
                }
            }
            __syncthreads();
            for (int k = 0; k < kc; ++k) {
                float x[4], y[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) x[a] = A[(ty + 16 * a) * (WMI_KC + 1) + k];
#pragma unroll
                for (int b = 0; b < 4; ++b) y[b] = B[(tx + 16 * b) * (WMI_KC + 1) + k];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const float df = x[a] - y[b]; // clustering.go:139
                        const float pr = df * df;     // :154 product (rounded)
                        s[a][b] = s[a][b] + pr;       // :154 sum (rounded), strictly in k order
                    }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i >= n || j >= n || i < j) continue;
            // max_size < 2: every pair of singletons is banned (clustering.go:228-234) and never read; the diagonal is never read
            const float v = (p.max_size >= 2 && i != j) ? ward_scale(s[a][b], 1, 1) : ICL_MAXF;
            p.tri[(int64_t)i * n + j] = v;
            p.tri[(int64_t)j * n + i] = v;
        }
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

__global__ __launch_bounds__(WMM_THREADS) void ward_many_mid_merge_kernel(const wm_prob *__restrict__ P, const int32_t *__restrict__ order)
{
    extern __shared__ __align__(16) unsigned char wm_lds[];
    const wm_prob p = P[order[blockIdx.x]];
    const int n = p.n, d = p.d, maxs = p.max_size, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *buf = reinterpret_cast<float *>(wm_lds);                     // two chunk buffers: row r of the pass at r * WMM_STRIDE
    float *cbuf = buf + 2 * WMM_BUF;                                    // two chunks of the new centroid
    const wm_slots S = wm_carve(wm_lds + WMM_CHUNK_BYTES, n, WMM_WAVES);
    uint64_t *const rkey = S.rkey;
    int32_t *const rarg = S.rarg, *const sz = S.sz, *const cid = S.cid;
    int32_t *cnt = reinterpret_cast<int32_t *>(wm_lds + WMM_CHUNK_BYTES + wm_slots_bytes(n, WMM_WAVES));                               // [0] rows to evaluate, [1] rows to rescan
    uint16_t *ev = reinterpret_cast<uint16_t *>(cnt + 2);
    uint16_t *stl = ev + n;
    float *M = p.tri; // entry (a, b) at a n + b, both orders written
    for (int t = tid; t < n; t += WMM_THREADS) {
        sz[t] = 1;
        cid[t] = t;
    }
    __syncthreads();
    auto cent = [&](int s) { return wm_cent(p, cid, s); };
    // row t's minimum over every live, size-compatible partner below MaxFloat32 (NaN never is: clustering.go:126), by one wave
    auto scan = [&](int t) {
        uint64_t best = ~0ull;
        int arg = -1;
        const int st = sz[t], ct = cid[t];
        const float *row = M + (int64_t)t * n;
        for (int u = lane; u < n; u += 64) {
            const int su = sz[u];
            if (u == t || su == 0 || st + su > maxs) continue;
            const float v = row[u];
            if (!(v < ICL_MAXF)) continue;
            const uint64_t k = wm_key(v, ct, cid[u]);
            if (k < best) {
                best = k;
                arg = u;
            }
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            const uint64_t ok = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            if (ok < best) {
                best = ok;
                arg = oa;
            }
        }
        if (lane == 0) {
            rkey[t] = best;
            rarg[t] = arg;
        }
    };
    for (int t = wave; t < n; t += WMM_WAVES) scan(t);
    __syncthreads();
    const bool vec = (d & 3) == 0; // rows are 16-byte aligned then (the host copies a problem whose rows are not)
    const int nch = (d + WMM_KC - 1) / WMM_KC;
    int step = 0;
    for (; step < p.T; ++step) {
        int shi, slo;
        if (!wm_select_pair<WMM_THREADS>(S, n, shi, slo)) break;
        const int sn = slo, snew = wm_merge_pair<WMM_THREADS>(p, S, step, shi, slo), cnew = n + step;
        if (tid == 0) cnt[0] = cnt[1] = 0;
        __syncthreads();
        // UpdateDistanceMatrix (:76-96).  Every live row t: banned pairs get MaxFloat32 and are never evaluated (:228-234); the
        // others go on the list of rows to evaluate; rows whose cached partner just died go on the list of rows to rescan.
        const float *cn = p.C + (int64_t)sn * d;
        float *Mn = M + (int64_t)sn * n;
        for (int t0 = 0; t0 < n; t0 += WMM_THREADS) {
            const int t = t0 + tid;
            const bool live = t < n && t != sn && sz[t] != 0;
            const bool evalp = live && sz[t] + snew <= maxs;
            if (live && !evalp) {
                M[(int64_t)t * n + sn] = ICL_MAXF;
                Mn[t] = ICL_MAXF;
            }
            wmm_append(evalp, t, &cnt[0], ev);
            wmm_append(live && (rarg[t] == shi || rarg[t] == slo), t, &cnt[1], stl);
        }
        __syncthreads();
        const int ne = cnt[0], ns = cnt[1];
        uint64_t nk = ~0ull;
        int nr = -1;
        for (int r0 = 0; r0 < ne; r0 += WMM_THREADS) { // a pass: WMM_THREADS listed rows, one per thread
            const int nrows = min(WMM_THREADS, ne - r0);
            const int my = tid < nrows ? ev[r0 + tid] : -1;
            float s = 0.0f;
            // the loads of this thread, the same rows in every chunk: vec, float4 q covers floats 4 (idx % (KC / 4)) ... of row
            // idx / (KC / 4), idx = tid + q WMM_THREADS; else float q is element idx % KC of row idx / KC
            const float *src[WMM_KC]; // (vec: the first KC / 4)
            if (vec) {
#pragma unroll
                for (int q = 0; q < WMM_KC / 4; ++q) {
                    const int idx = tid + q * WMM_THREADS, r = idx / (WMM_KC / 4);
                    src[q] = r < nrows ? cent(ev[r0 + r]) + (idx % (WMM_KC / 4)) * 4 : nullptr;
                }
            } else {
#pragma unroll
                for (int q = 0; q < WMM_KC; ++q) {
                    const int idx = tid + q * WMM_THREADS, r = idx / WMM_KC;
                    src[q] = r < nrows ? cent(ev[r0 + r]) + idx % WMM_KC : nullptr;
                }
            }
            float g[WMM_KC];
            float gc = 0.0f; // threads 0 .. KC - 1: the new centroid's element
            auto fetch = [&](int c) {
                const int k0 = c * WMM_KC;
                if (vec) {
#pragma unroll
                    for (int q = 0; q < WMM_KC / 4; ++q) {
                        const int kk = ((tid + q * WMM_THREADS) % (WMM_KC / 4)) * 4;
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (src[q] && k0 + kk < d) v = *reinterpret_cast<const float4 *>(src[q] + k0);
                        g[4 * q] = v.x, g[4 * q + 1] = v.y, g[4 * q + 2] = v.z, g[4 * q + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < WMM_KC; ++q) {
                        const int kk = (tid + q * WMM_THREADS) % WMM_KC;
                        g[q] = 0.0f;
                        if (src[q] && k0 + kk < d) g[q] = src[q][k0];
                    }
                }
                if (tid < WMM_KC) gc = k0 + tid < d ? cn[k0 + tid] : 0.0f;
            };
            auto stash = [&](int c) {
                float *b = buf + (c & 1) * WMM_BUF;
                if (vec) {
#pragma unroll
                    for (int q = 0; q < WMM_KC / 4; ++q) {
                        const int idx = tid + q * WMM_THREADS;
                        float *o = b + (idx / (WMM_KC / 4)) * WMM_STRIDE + (idx % (WMM_KC / 4)) * 4;
                        o[0] = g[4 * q], o[1] = g[4 * q + 1], o[2] = g[4 * q + 2], o[3] = g[4 * q + 3];
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < WMM_KC; ++q) {
                        const int idx = tid + q * WMM_THREADS;
                        b[(idx / WMM_KC) * WMM_STRIDE + idx % WMM_KC] = g[q];
                    }
                }
                if (tid < WMM_KC) cbuf[(c & 1) * WMM_KC + tid] = gc;
            };
            fetch(0);
            stash(0);
            __syncthreads();
            for (int c = 0; c < nch; ++c) {
                if (c + 1 < nch) fetch(c + 1); // in flight while chunk c is added
                if (my >= 0) {
                    const float *rb = buf + (c & 1) * WMM_BUF + tid * WMM_STRIDE;
                    const float4 *cb4 = reinterpret_cast<const float4 *>(cbuf + (c & 1) * WMM_KC);
                    const int kc = min(WMM_KC, d - c * WMM_KC);
                    if (kc == WMM_KC) {
#pragma unroll
                        for (int q = 0; q < WMM_KC / 4; ++q) {
                            const float4 y = cb4[q];
                            float df = rb[4 * q] - y.x; // clustering.go:139
                            float pr = df * df;         // :154 product (rounded)
                            s = s + pr;                 // :154 sum (rounded), strictly in k order
                            df = rb[4 * q + 1] - y.y;
                            pr = df * df;
                            s = s + pr;
                            df = rb[4 * q + 2] - y.z;
                            pr = df * df;
                            s = s + pr;
                            df = rb[4 * q + 3] - y.w;
                            pr = df * df;
                            s = s + pr;
                        }
                    } else {
                        const float *cb = cbuf + (c & 1) * WMM_KC;
                        for (int q = 0; q < kc; ++q) {
                            const float df = rb[q] - cb[q];
                            const float pr = df * df;
                            s = s + pr;
                        }
                    }
                }
                if (c + 1 < nch) stash(c + 1); // (that buffer was last read before the previous barrier)
                __syncthreads();
            }
            if (my >= 0) { // WardDistance(clusters[my], newCluster); the owner of the row updates its cache
                const float v = ward_scale(s, sz[my], snew);
                M[(int64_t)my * n + sn] = v;
                Mn[my] = v;
                const uint64_t k = v < ICL_MAXF ? wm_key(v, cid[my], cnew) : ~0ull;
                if (k < nk) {
                    nk = k;
                    nr = my;
                }
                if (rarg[my] != shi && rarg[my] != slo && k < rkey[my]) {
                    rkey[my] = k;
                    rarg[my] = sn;
                }
            }
        }
        wm_block_min<WMM_WAVES>(nk, nr, S.red_k, S.red_r); // (its barriers also publish the new row and column)
        if (tid == 0) {
            rkey[sn] = nk;
            rarg[sn] = nr;
        }
        for (int q = wave; q < ns; q += WMM_WAVES) scan(stl[q]);
        __syncthreads();
    }
    if (tid == 0) *p.nm = step;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int icl_ward_cluster_exact(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, int32_t min_size, int32_t max_size, int32_t *cluster_id,
                           int32_t *member_rank, int32_t *n_clusters, std::vector<int32_t> *merges); // ward.hip (ctx->mu held)
int icl_ward_assign_ids(icl_ctx *ctx, int64_t n, int32_t min_size, int32_t max_size, const std::vector<int32_t> &pairs, int64_t nmerge,
                        int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters); // ward.hip

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

struct icl_many_ws {
    void *buf = nullptr;
    size_t bytes = 0;
};

void icl_many_free(icl_ctx *ctx)
{
    if (!ctx || !ctx->many) return;
    if (ctx->many->buf) (void)hipFree(ctx->many->buf);
    delete ctx->many;
    ctx->many = nullptr;
}

static int wm_ensure(icl_ctx *ctx, size_t bytes, char **out)
{
    if (!ctx->many) ctx->many = new icl_many_ws;
    icl_many_ws *w = ctx->many;
    if (w->bytes < bytes) {
        if (w->buf) {
            ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
            (void)hipFree(w->buf);
            w->buf = nullptr;
            w->bytes = 0;
        }
        const size_t b = std::max(bytes, (size_t)1 << 20);
        if (hipMalloc(&w->buf, b) != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "icl_cluster_many: workspace of %zu bytes", b);
        w->bytes = b;
    }
    *out = (char *)w->buf;
    return ICL_OK;
}

// bump allocation inside the workspace: 256-byte aligned pieces
struct wm_layout {
    size_t off = 0;
    size_t take(size_t bytes)
    {
        const size_t o = off;
        off += (bytes + 255) / 256 * 256;
        return o;
    }
};

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
};
static const wm_kind wm_kind_small = {
    [](int64_t n) { return wm_tri_len(n) * 4; },
    [](int32_t g, int64_t n, std::vector<int32_t> &prob, std::vector<int64_t> &arg) {
        for (int64_t q = 0; q < wm_tri_len(n); q += WM_THREADS) prob.push_back(g), arg.push_back(q);
    },
    8,
    [](int64_t n) { return wm_lds_bytes(n, true) <= WM_LDS_MAX; },
    [](int64_t n) { return wm_lds_bytes(n, wm_lds_bytes(n, true) <= WM_LDS_MAX); },
    (const void *)ward_many_init_kernel, (const void *)ward_many_merge_kernel, WM_THREADS, WM_THREADS,
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
    (const void *)ward_many_mid_init_kernel, (const void *)ward_many_mid_merge_kernel, 256, WMM_THREADS,
};

// centroids + matrix of one problem in a group's data region (256-byte aligned pieces)
static size_t wm_data_bytes(const wm_kind &k, int64_t n, int64_t d)
{
    wm_layout R;
    R.take((size_t)(n * d * 4));
    R.take((size_t)k.mat_bytes(n));
    return R.off;
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
    size_t head_bytes() const { return sizeof(wm_prob) * probs.size() + (size_t)kind->arg_bytes * blk_arg.size() + 4 * (probs.size() + blk_prob.size()); }
};

// the per-problem arguments of both entry points
struct wm_args {
    int32_t nprob;
    const int64_t *e_off;
    const int32_t *n, *d, *min_size, *max_size;
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
};

// k, status and route of every problem; many_stats
static void wm_classify(icl_ctx *ctx, const wm_args &A, wm_plan &pl, std::vector<int32_t> &small, std::vector<int32_t> &mid)
{
    const int64_t cap = wm_cap();
    const int32_t nprob = A.nprob;
    pl.img.assign(nprob + 1, 0);
    pl.k.assign(nprob, 0);
    pl.why.resize(nprob);
    pl.st.assign(nprob, ICL_OK);
    pl.route.assign(nprob, WM_NONE);
    for (int32_t p = 0; p < nprob; ++p) {
        pl.img[p + 1] = pl.img[p] + A.n[p];
        if (icl_calc_optimal_clusters(A.n[p], A.min_size[p], A.max_size[p], &pl.k[p]) != ICL_OK) { // clustering.go:203-207
            pl.st[p] = ICL_ERR_CONSTRAINT;
            char b[200];
            snprintf(b, sizeof b, "cannot satisfy cluster size constraints with total items (%d), minSize (%d), and maxSize (%d)", A.n[p],
                     A.min_size[p], A.max_size[p]);
            pl.why[p] = b;
        }
    }
    auto mid_size = [&](int32_t p) { return A.n[p] > cap && A.n[p] <= WMM_CAP; };
    int64_t mid_band[WMM_BANDS] = {};
    for (int32_t p = 0; p < nprob; ++p) {
        if (pl.st[p] != ICL_OK || A.n[p] - pl.k[p] <= 0) continue;
        pl.route[p] = A.n[p] <= cap ? WM_SMALL : WM_LARGE;
        if (pl.route[p] == WM_SMALL) small.push_back(p);
        if (mid_size(p)) ++mid_band[wmm_band(A.n[p])];
        pl.need_e = pl.need_e || (int64_t)A.n[p] * A.d[p] > 0;
    }
    if ((int64_t)small.size() < WM_MIN_BATCH) {
        for (int32_t p : small) pl.route[p] = WM_LARGE;
        small.clear();
    }
    if (ctx->many_mid != ICL_MANY_MID_OFF)
        for (int32_t p = 0; p < nprob; ++p)
            if (pl.route[p] == WM_LARGE && mid_size(p) && (ctx->many_mid == ICL_MANY_MID_ON || wmm_auto_takes(A.n[p], mid_band))) {
                pl.route[p] = WM_MID;
                mid.push_back(p);
            }
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
            }
            wm_group &g = pl.groups.back();
            kind.init_blocks((int32_t)g.probs.size(), A.n[p], g.blk_prob, g.blk_arg);
            g.probs.push_back(p);
            g.data_bytes += need;
        }
    };
    add(wm_kind_small, small, SIZE_MAX);
    add(wm_kind_mid, mid, wmm_budget());
    ctx->many_stats[3] = (int64_t)pl.groups.size() - (small.empty() ? 0 : 1);
    wm_layout L;
    pl.o_e = upload_e && pl.need_e ? L.take((size_t)e_len * 4) : 0;
    pl.o_al.assign(A.nprob, SIZE_MAX);
    pl.log_at.assign(A.nprob, 0);
    for (int32_t p = 0; p < A.nprob; ++p) {
        if (pl.route[p] && A.d[p] % 4 == 0 && A.n[p] && A.e_off[p] % 4 != 0) pl.o_al[p] = L.take((size_t)A.n[p] * A.d[p] * 4);
        if (pl.route[p] == WM_SMALL || pl.route[p] == WM_MID) {
            pl.log_at[p] = pl.log_ints;
            pl.log_ints += 2 * (int64_t)A.n[p] + 1; // 2 (n - k) ids + the count
        }
    }
    pl.o_logs = L.take(4 * (size_t)std::max<int64_t>(pl.log_ints, 1));
    size_t shared = 0;
    for (wm_group &g : pl.groups) {
        g.o_head = L.take(g.head_bytes());
        if (g.kind == &wm_kind_small) g.o_data = L.take(g.data_bytes);
        else shared = std::max(shared, g.data_bytes);
    }
    const size_t o_shared = L.take(shared);
    for (wm_group &g : pl.groups)
        if (g.kind != &wm_kind_small) g.o_data = o_shared;
    pl.ws_bytes = L.off;
}

// the group's head (problem table with device addresses, init blocks, order) uploaded, then one init launch and one merge launch
static int wm_run_group(icl_ctx *ctx, const wm_args &A, const wm_plan &pl, wm_group &g, char *ws, const std::vector<const float *> &rowsE)
{
    const size_t G = g.probs.size(), o_arg = sizeof(wm_prob) * G, o_ord = o_arg + (size_t)g.kind->arg_bytes * g.blk_arg.size();
    g.head.resize(g.head_bytes());
    wm_prob *tab = reinterpret_cast<wm_prob *>(g.head.data());
    int32_t *ord = reinterpret_cast<int32_t *>(g.head.data() + o_ord);
    wm_layout R; // the problems' places in the group's data region
    int64_t lds = 0;
    for (size_t i = 0; i < G; ++i) {
        const int32_t p = g.probs[i];
        float *C = (float *)(ws + g.o_data + R.take((size_t)A.n[p] * A.d[p] * 4));
        float *mat = (float *)(ws + g.o_data + R.take((size_t)g.kind->mat_bytes(A.n[p])));
        int32_t *log = (int32_t *)(ws + pl.o_logs) + pl.log_at[p];
        tab[i] = wm_prob{rowsE[p], C, mat, A.n[p], A.d[p], A.max_size[p], (int32_t)(A.n[p] - pl.k[p]), log, log + 2 * (int64_t)A.n[p],
                         g.kind->lds_tri(A.n[p]) ? 1 : 0, 0};
        ord[i] = (int32_t)i; // (probs is sorted: largest first)
        lds = std::max(lds, g.kind->lds_bytes(A.n[p]));
    }
    for (size_t b = 0; b < g.blk_arg.size(); ++b) // (the low arg_bytes of a little-endian int64_t)
        memcpy(g.head.data() + o_arg + (size_t)g.kind->arg_bytes * b, &g.blk_arg[b], g.kind->arg_bytes);
    if (!g.blk_prob.empty()) memcpy(ord + G, g.blk_prob.data(), 4 * g.blk_prob.size());
    const char *tab_d = ws + g.o_head, *arg_d = tab_d + o_arg, *ord_d = tab_d + o_ord, *blk_d = ord_d + 4 * G;
    ICL_HIP(ctx, hipMemcpyAsync(ws + g.o_head, g.head.data(), g.head.size(), hipMemcpyHostToDevice, ctx->stream));
    void *init_args[] = {&tab_d, &blk_d, &arg_d}, *merge_args[] = {&tab_d, &ord_d};
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
    char *ws = nullptr;
    ICL_TRY(wm_ensure(ctx, pl.ws_bytes, &ws));
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

// ids from the merge logs (clustering.go:265-280, ward.hip's rule), merge logs, statuses; the lowest failed problem's error
static int wm_collect(icl_ctx *ctx, const wm_args &A, wm_plan &pl, const std::vector<int32_t> &slab, std::vector<std::vector<int32_t>> &big_log,
                      int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status,
                      icl_item_failure *lowest)
{
    std::vector<int32_t> pairs;
    for (int32_t p = 0; p < A.nprob; ++p) {
        int32_t *cid = cluster_id + pl.img[p], *rank = member_rank + pl.img[p];
        int64_t nm = 0;
        if (pl.route[p] == WM_LARGE) {
            pairs.swap(big_log[p]);
            nm = (int64_t)pairs.size() / 2;
        } else if (pl.route[p] != WM_NONE) {
            const int32_t *lg = slab.data() + pl.log_at[p];
            nm = lg[2 * (int64_t)A.n[p]];
            pairs.assign(lg, lg + 2 * nm);
        } else
            pairs.clear();
        if (pl.st[p] == ICL_OK && pl.route[p] != WM_LARGE) {
            const int rc = icl_ward_assign_ids(ctx, A.n[p], A.min_size[p], A.max_size[p], pairs, nm, cid, rank, &n_clusters[p]);
            if (rc != ICL_OK) {
                pl.st[p] = rc;
                pl.why[p] = ctx->err;
            }
        }
        if (pl.st[p] != ICL_OK) {
            std::fill(cid, cid + A.n[p], -1);
            std::fill(rank, rank + A.n[p], -1);
            n_clusters[p] = 0;
            nm = 0;
        }
        n_merges[p] = (int32_t)nm;
        if (merges && nm) memcpy(merges + 2 * pl.img[p], pairs.data(), 8 * (size_t)nm);
        status[p] = pl.st[p];
    }
    for (int32_t p = 0; p < A.nprob; ++p)
        if (pl.st[p] != ICL_OK) {
            if (lowest) *lowest = icl_item_failure{p, pl.st[p], pl.why[p]};
            return icl_fail(ctx, pl.st[p], "icl_cluster_many: problem %d: %s", p, pl.why[p].c_str());
        }
    return ICL_OK;
}

// Both entry points, after the argument check, with ctx->mu held.  d_E: the embeddings on the device (e_len floats); h_E: the host copy
// (icl_cluster_many), uploaded into the workspace here, or nullptr.  (Declared in icl_common.h: icl_cluster_requests, requests.hip, is the
// third caller.)
int cluster_many_locked(icl_ctx *ctx, int32_t nprob, const float *d_E, const float *h_E, int64_t e_len, const int64_t *e_off,
                               const int32_t *n, const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id,
                               int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status, icl_item_failure *lowest)
{
    const wm_args A = {nprob, e_off, n, d, min_size, max_size};
    wm_plan pl;
    {
        std::vector<int32_t> small, mid;
        wm_classify(ctx, A, pl, small, mid);
        wm_make_plan(ctx, A, h_E != nullptr, e_len, small, mid, pl);
    }
    std::vector<const float *> rowsE(nprob, nullptr);
    std::vector<int32_t> slab;
    ICL_TRY(wm_enqueue(ctx, A, pl, d_E, h_E, e_len, rowsE, slab));
    // the large-N route, one problem at a time, behind the launches above (its reports of the last icl_cluster are restored)
    std::vector<std::vector<int32_t>> big_log(nprob);
    {
        wm_last_guard keep(ctx);
        for (int32_t p = 0; p < nprob; ++p) {
            if (pl.route[p] != WM_LARGE) continue;
            int32_t nc = 0;
            const int rc = icl_ward_cluster_exact(ctx, rowsE[p], n[p], d[p], min_size[p], max_size[p], cluster_id + pl.img[p], member_rank + pl.img[p],
                                                  &nc, &big_log[p]);
            n_clusters[p] = nc;
            if (rc != ICL_OK) {
                pl.st[p] = rc;
                pl.why[p] = ctx->err;
            }
        }
    }
    if (!pl.groups.empty()) ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return wm_collect(ctx, A, pl, slab, big_log, cluster_id, member_rank, n_clusters, n_merges, merges, status, lowest);
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

extern "C" int icl_cluster_many_dev(icl_ctx *ctx, int32_t nprob, const float *d_E, int64_t e_len, const int64_t *e_off, const int32_t *n,
                                    const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank,
                                    int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status)
{
    return no_throw(ctx, "icl_cluster_many_dev", [&]() -> int {
        ICL_TRY(wm_check_args(ctx, "icl_cluster_many_dev", nprob, d_E, e_len, e_off, n, d, min_size, max_size, cluster_id, member_rank, n_clusters,
                              n_merges, status));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        return cluster_many_locked(ctx, nprob, d_E, nullptr, e_len, e_off, n, d, min_size, max_size, cluster_id, member_rank, n_clusters, n_merges,
                                   merges, status);
    });
}

extern "C" int icl_cluster_many(icl_ctx *ctx, int32_t nprob, const float *E, int64_t e_len, const int64_t *e_off, const int32_t *n, const int32_t *d,
                                const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id, int32_t *member_rank, int32_t *n_clusters,
                                int32_t *n_merges, int32_t *merges, int32_t *status)
{
    return no_throw(ctx, "icl_cluster_many", [&]() -> int {
        ICL_TRY(wm_check_args(ctx, "icl_cluster_many", nprob, E, e_len, e_off, n, d, min_size, max_size, cluster_id, member_rank, n_clusters, n_merges,
                              status));
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        return cluster_many_locked(ctx, nprob, nullptr, E, e_len, e_off, n, d, min_size, max_size, cluster_id, member_rank, n_clusters, n_merges, merges,
                                   status);
    });
}
