// ward_many.hip -- many small, independent PerformClusteringWithConstraints calls (clustering.go:198-284) in one call, exact mode:
// icl_cluster_many / icl_cluster_many_dev (include/imageclust.h).  The serving pattern of the reference: every request clusters its
// own few hundred images (d = 1000 + labels), so a loaded server holds many small problems at once.  DESIGN.md "Many small problems".
//
//   * ward_many_init_kernel: one launch over (problem, 256-pair tile) writes every problem's exact lower triangle
//     (ComputeInitialDistanceMatrix, clustering.go:61-73) into one workspace, one thread per pair.
//   * ward_many_merge_kernel: ONE WORKGROUP PER PROBLEM, largest problems first.  The workgroup keeps its triangle in LDS when it
//     fits (n <= 281 with the per-slot arrays, WM_LDS_MAX; the launch's dynamic LDS is that of the largest such problem of the batch),
//     else in the global workspace, plus a per-row (min, argmin) cache, the sizes and the creation ids.  Each step selects the
//     lexicographic minimum of (value, larger creation id, smaller creation id) over the live, size-compatible pairs -- the
//     reference's first strict minimum in row-major order with its MaxFloat32 ban (ward.hip's header) -- forms the
//     merged centroid (clustering.go:37-40) and the new cluster's row exactly (:76-96), and rescans a row only when its cached
//     partner died.  Workgroups share nothing and never wait for each other: no flags, no spins, so the launch is correct
//     whatever the number of workgroups resident at a time.
//   * ward_many_mid_init_kernel / ward_many_mid_merge_kernel: the mid-size route, cap < n <= WMM_CAP rows, again one workgroup per
//     problem with nothing shared between workgroups (see there); the host runs these problems in groups under a workspace budget.
//   * Problems above WMM_CAP rows, a lone small problem, and mid-size problems the policy leaves there (icl_set_many_options) go
//     through ward.hip's large-N engine (icl_ward_cluster_exact) inside the same call, one at a time.
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
// LDS bytes of the merge kernel for a problem of n rows: per-slot arrays, reduction scratch, the triangle when it is kept there
__host__ __device__ static inline int64_t wm_meta_bytes(int64_t n) { return (n * 20 + 64 * 3 + 15) / 16 * 16; }
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

// block-wide minimum of (key, slot); every thread returns it
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
    for (int q = 1; q < WM_WAVES; ++q)
        if (sk[q] < k) {
            k = sk[q];
            r = sr[q];
        }
    __syncthreads(); // the scratch is free for the next reduction
}

__global__ __launch_bounds__(WM_THREADS) void ward_many_merge_kernel(const wm_prob *__restrict__ P, const int32_t *__restrict__ order)
{
    extern __shared__ __align__(16) unsigned char wm_lds[];
    const wm_prob p = P[order[blockIdx.x]];
    const int n = p.n, d = p.d, maxs = p.max_size;
    uint64_t *rkey = reinterpret_cast<uint64_t *>(wm_lds); // row t's best key (UINT64_MAX: none)
    int32_t *rarg = reinterpret_cast<int32_t *>(rkey + n); // ... and the slot of its partner
    int32_t *sz = rarg + n;                                 // size of slot s's cluster, 0 when the slot is dead
    int32_t *cid = sz + n;                                  // creation id of slot s's cluster: singleton i -> i, t-th merge -> n + t
    uint64_t *red_k = reinterpret_cast<uint64_t *>(cid + n + (n & 1)); // (8-byte aligned)
    int32_t *red_r = reinterpret_cast<int32_t *>(red_k + WM_WAVES);
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
    const float *E = p.E;
    float *Cw = p.C;
    auto cent = [&](int s) -> const float * { return (cid[s] >= n ? Cw : E) + (int64_t)s * d; };
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
        // FindClosestClusters (clustering.go:119-133) over the row caches
        uint64_t bk = ~0ull;
        int br = -1;
        for (int t = threadIdx.x; t < n; t += WM_THREADS)
            if (rkey[t] < bk) {
                bk = rkey[t];
                br = t;
            }
        wm_block_min(bk, br, red_k, red_r);
        if (bk == ~0ull) break; // (-1, -1): "No more clusters to merge" (:224-227)
        const int bu = rarg[br];
        const int shi = cid[br] > cid[bu] ? br : bu, slo = shi == br ? bu : br; // position i (the later cluster) and j
        const int sa = sz[shi], sb = sz[slo];
        const int sn = slo; // the new cluster lives in the slot of the earlier one; shi dies
        if (threadIdx.x == 0) {
            p.log[2 * step] = cid[shi];
            p.log[2 * step + 1] = cid[slo];
        }
        // MergeClusters(clusters[i], clusters[j]) (:236, :37-40) into slot sn's centroid row (each k read, then written, by one thread)
        {
            const float fa = (float)sa, fb = (float)sb, fs = (float)(sa + sb);
            const float *ca = cent(shi), *cb = cent(slo);
            float *out = Cw + (int64_t)sn * d;
            for (int k = threadIdx.x; k < d; k += WM_THREADS) out[k] = ward_merge_elem(fa, ca[k], fb, cb[k], fs);
        }
        __syncthreads(); // every thread has read the old sizes, ids and centroids
        if (threadIdx.x == 0) {
            sz[shi] = 0;
            rkey[shi] = ~0ull;
            sz[sn] = sa + sb;
            cid[sn] = n + step;
        }
        __syncthreads();
        // UpdateDistanceMatrix (:76-96): WardDistance(clusters[t], newCluster) for every live t; the owner of row t updates its cache
        const int snew = sa + sb, cnew = n + step;
        const float *cn = Cw + (int64_t)sn * d;
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
        wm_block_min(nk, nr, red_k, red_r); // (its barriers also publish the new row)
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

// LDS bytes of the mid merge kernel: two chunk buffers, two centroid chunks, the per-slot arrays (20 B per row), reduction scratch,
// two counters, the list of rows to evaluate and the list of rows to rescan
__host__ __device__ static inline int64_t wmm_lds_bytes(int64_t n)
{
    return ((2 * WMM_BUF + 2 * WMM_KC) * 4 + (n + (n & 1)) * 20 + WMM_WAVES * 12 + 8 + n * 4 + 15) / 16 * 16;
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

// block-wide minimum of (key, slot) over WMM_THREADS threads; every thread returns it
__device__ __forceinline__ void wmm_block_min(uint64_t &k, int &r, uint64_t *sk, int *sr)
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
    for (int q = 1; q < WMM_WAVES; ++q)
        if (sk[q] < k) {
            k = sk[q];
            r = sr[q];
        }
    __syncthreads(); // the scratch is free for the next reduction
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
    uint64_t *rkey = reinterpret_cast<uint64_t *>(cbuf + 2 * WMM_KC);   // row t's best key (UINT64_MAX: none)
    int32_t *rarg = reinterpret_cast<int32_t *>(rkey + n);              // ... and the slot of its partner
    int32_t *sz = rarg + n;                                             // size of slot s's cluster, 0 when the slot is dead
    int32_t *cid = sz + n;                                              // creation id of slot s's cluster
    uint64_t *red_k = reinterpret_cast<uint64_t *>(cid + n + (n & 1)); // (8-byte aligned)
    int32_t *red_r = reinterpret_cast<int32_t *>(red_k + WMM_WAVES);
    int32_t *cnt = red_r + WMM_WAVES;                                   // [0] rows to evaluate, [1] rows to rescan
    uint16_t *ev = reinterpret_cast<uint16_t *>(cnt + 2);
    uint16_t *stl = ev + n;
    float *M = p.tri; // entry (a, b) at a n + b, both orders written
    for (int t = tid; t < n; t += WMM_THREADS) {
        sz[t] = 1;
        cid[t] = t;
    }
    __syncthreads();
    const float *E = p.E;
    float *Cw = p.C;
    auto cent = [&](int s) -> const float * { return (cid[s] >= n ? Cw : E) + (int64_t)s * d; };
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
        // FindClosestClusters (clustering.go:119-133) over the row caches
        uint64_t bk = ~0ull;
        int br = -1;
        for (int t = tid; t < n; t += WMM_THREADS)
            if (rkey[t] < bk) {
                bk = rkey[t];
                br = t;
            }
        wmm_block_min(bk, br, red_k, red_r);
        if (bk == ~0ull) break; // (-1, -1): "No more clusters to merge" (:224-227)
        const int bu = rarg[br];
        const int shi = cid[br] > cid[bu] ? br : bu, slo = shi == br ? bu : br; // position i (the later cluster) and j
        const int sa = sz[shi], sb = sz[slo];
        const int sn = slo; // the new cluster lives in the slot of the earlier one; shi dies
        if (tid == 0) {
            p.log[2 * step] = cid[shi];
            p.log[2 * step + 1] = cid[slo];
        }
        // MergeClusters(clusters[i], clusters[j]) (:236, :37-40) into slot sn's centroid row (each k read, then written, by one thread)
        {
            const float fa = (float)sa, fb = (float)sb, fs = (float)(sa + sb);
            const float *ca = cent(shi), *cb = cent(slo);
            float *out = Cw + (int64_t)sn * d;
            for (int k = tid; k < d; k += WMM_THREADS) out[k] = ward_merge_elem(fa, ca[k], fb, cb[k], fs);
        }
        __syncthreads(); // every thread has read the old sizes, ids and centroids
        if (tid == 0) {
            sz[shi] = 0;
            rkey[shi] = ~0ull;
            sz[sn] = sa + sb;
            cid[sn] = n + step;
            cnt[0] = 0;
            cnt[1] = 0;
        }
        __syncthreads();
        // UpdateDistanceMatrix (:76-96).  Every live row t: banned pairs get MaxFloat32 and are never evaluated (:228-234); the
        // others go on the list of rows to evaluate; rows whose cached partner just died go on the list of rows to rescan.
        const int snew = sa + sb, cnew = n + step;
        const float *cn = Cw + (int64_t)sn * d;
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
        wmm_block_min(nk, nr, red_k, red_r); // (its barriers also publish the new row and column)
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

// The mid route's workspace per problem (centroids + the square matrix, 256-byte aligned pieces) and the budget a group of them
// stays under: ICL_MANY_MID_WS_MB (read once per process; for A/B runs and tests), else WMM_WS_DEFAULT.
#define WMM_WS_DEFAULT ((size_t)8 << 30)
static size_t wmm_ws_bytes(int64_t n, int64_t d) { return ((size_t)(n * d * 4) + 255) / 256 * 256 + ((size_t)(n * n * 4) + 255) / 256 * 256; }
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

// the last icl_cluster's reports (icl_last_merges, icl_last_merge_values, icl_last_ward_*): a problem on the large-N route must not change them
struct wm_last_guard {
    icl_ctx *c;
    std::vector<int32_t> merges;
    std::vector<float> vals;
    int64_t viol, layout[3], stats[4];
    int32_t mode[2];
    double dist_ms, merge_ms;
    explicit wm_last_guard(icl_ctx *ctx) : c(ctx), merges(ctx->last_merges), vals(ctx->last_merge_vals), viol(ctx->ward_bound_viol),
                                           dist_ms(ctx->last_dist_ms), merge_ms(ctx->last_merge_ms)
    {
        memcpy(layout, ctx->ward_layout, sizeof layout);
        memcpy(stats, ctx->ward_stats, sizeof stats);
        memcpy(mode, ctx->ward_mode, sizeof mode);
    }
    ~wm_last_guard()
    {
        c->last_merges.swap(merges);
        c->last_merge_vals.swap(vals);
        c->ward_bound_viol = viol;
        memcpy(c->ward_layout, layout, sizeof layout);
        memcpy(c->ward_stats, stats, sizeof stats);
        memcpy(c->ward_mode, mode, sizeof mode);
        c->last_dist_ms = dist_ms;
        c->last_merge_ms = merge_ms;
    }
};

// Both entry points, after the argument check, with ctx->mu held.  d_E: the embeddings on the device (e_len floats); h_E: the host copy
// (icl_cluster_many), uploaded into the workspace here, or nullptr.
static int cluster_many_locked(icl_ctx *ctx, int32_t nprob, const float *d_E, const float *h_E, int64_t e_len, const int64_t *e_off,
                               const int32_t *n, const int32_t *d, const int32_t *min_size, const int32_t *max_size, int32_t *cluster_id,
                               int32_t *member_rank, int32_t *n_clusters, int32_t *n_merges, int32_t *merges, int32_t *status)
{
    const int64_t cap = wm_cap();
    std::vector<int64_t> img(nprob + 1, 0), k(nprob, 0);
    std::vector<std::string> why(nprob);
    std::vector<int32_t> st(nprob, ICL_OK);
    for (int32_t p = 0; p < nprob; ++p) {
        img[p + 1] = img[p] + n[p];
        if (icl_calc_optimal_clusters(n[p], min_size[p], max_size[p], &k[p]) != ICL_OK) { // clustering.go:203-207
            st[p] = ICL_ERR_CONSTRAINT;
            char b[200];
            snprintf(b, sizeof b, "cannot satisfy cluster size constraints with total items (%d), minSize (%d), and maxSize (%d)", n[p], min_size[p],
                     max_size[p]);
            why[p] = b;
        }
    }
    // routes: 0 nothing to merge (or failed), 1 the small kernels, 2 the large-N engine, 3 the mid-size kernels
    std::vector<int8_t> route(nprob, 0);
    std::vector<int32_t> gpu; // problems of route 1
    std::vector<int32_t> mid; // problems of route 3
    bool need_e = false;
    int64_t mid_band[WMM_BANDS] = {};
    for (int32_t p = 0; p < nprob; ++p) {
        if (st[p] != ICL_OK || n[p] - k[p] <= 0) continue;
        route[p] = n[p] <= cap ? 1 : 2;
        if (route[p] == 1) gpu.push_back(p);
        if (n[p] > cap && n[p] <= WMM_CAP) ++mid_band[wmm_band(n[p])];
        need_e = need_e || (int64_t)n[p] * d[p] > 0;
    }
    if ((int64_t)gpu.size() < WM_MIN_BATCH) {
        for (int32_t p : gpu) route[p] = 2;
        gpu.clear();
    }
    if (ctx->many_mid != ICL_MANY_MID_OFF)
        for (int32_t p = 0; p < nprob; ++p)
            if (route[p] == 2 && n[p] > cap && n[p] <= WMM_CAP && (ctx->many_mid == ICL_MANY_MID_ON || wmm_auto_takes(n[p], mid_band))) {
                route[p] = 3;
                mid.push_back(p);
            }
    std::stable_sort(mid.begin(), mid.end(), [&](int32_t a, int32_t b) { return n[a] > n[b]; }); // largest first, within and across groups
    // groups of mid problems whose centroids and matrices fit the budget together (a group holds at least one problem)
    const int32_t NM = (int32_t)mid.size();
    std::vector<int32_t> grp_at(1, 0); // group q: mid[grp_at[q] .. grp_at[q + 1])
    size_t mid_ws = 0;
    {
        size_t cur = 0;
        for (int32_t g = 0; g < NM; ++g) {
            const size_t need = wmm_ws_bytes(n[mid[g]], d[mid[g]]);
            if (g > grp_at.back() && cur + need > wmm_budget()) {
                grp_at.push_back(g);
                cur = 0;
            }
            cur += need;
            mid_ws = std::max(mid_ws, cur);
        }
        if (NM) grp_at.push_back(NM);
    }
    const int32_t NG = (int32_t)grp_at.size() - 1;
    ctx->many_stats[0] = (int64_t)gpu.size();
    ctx->many_stats[1] = NM;
    ctx->many_stats[2] = 0;
    for (int32_t p = 0; p < nprob; ++p) ctx->many_stats[2] += route[p] == 2;
    ctx->many_stats[3] = NG;
    // workspace: [uploaded E] [aligned copies] [problem table] [order] [init blocks] [logs, counts] [centroids] [triangles]
    wm_layout L;
    const size_t o_e = h_E && need_e ? L.take((size_t)e_len * 4) : 0;
    std::vector<size_t> o_al(nprob, SIZE_MAX); // problems whose rows the float4 loads cannot read in place: a 16-byte aligned copy
    for (int32_t p = 0; p < nprob; ++p)
        if (route[p] && d[p] % 4 == 0 && n[p] && e_off[p] % 4 != 0) o_al[p] = L.take((size_t)n[p] * d[p] * 4);
    const int32_t G = (int32_t)gpu.size();
    std::vector<int32_t> blk_prob;
    std::vector<int64_t> blk_pair0;
    for (int32_t g = 0; g < G; ++g)
        for (int64_t q = 0; q < wm_tri_len(n[gpu[g]]); q += WM_THREADS) {
            blk_prob.push_back(g);
            blk_pair0.push_back(q);
        }
    const size_t o_tab = L.take(sizeof(wm_prob) * std::max(G, 1)), o_ord = L.take(4 * (size_t)std::max(G, 1));
    const size_t o_bp = L.take(4 * std::max<size_t>(blk_prob.size(), 1)), o_bq = L.take(8 * std::max<size_t>(blk_pair0.size(), 1));
    std::vector<size_t> o_log(G), o_c(G), o_t(G);
    int64_t log_ints = 0;
    for (int32_t g = 0; g < G; ++g) log_ints += 2 * (int64_t)n[gpu[g]] + 1; // 2 (n - k) ids + the count
    const size_t o_logs = L.take(4 * (size_t)std::max<int64_t>(log_ints, 1));
    for (int32_t g = 0; g < G; ++g) {
        const int32_t p = gpu[g];
        o_c[g] = L.take((size_t)n[p] * d[p] * 4);
        o_t[g] = L.take((size_t)wm_tri_len(n[p]) * 4);
    }
    // the mid route: [problem table] [order] [init blocks] [logs, counts] of every group, then one region of centroids and matrices
    // that the groups use one after the other (the launches are ordered on the stream)
    std::vector<int32_t> mblk_prob, mblk_tile;
    std::vector<size_t> mblk_at(NG + 1, 0);
    for (int32_t q = 0; q < NG; ++q) {
        for (int32_t g = grp_at[q]; g < grp_at[q + 1]; ++g) {
            const int32_t nt = (n[mid[g]] + WMI_TILE - 1) / WMI_TILE;
            for (int32_t ti = 0; ti < nt; ++ti)
                for (int32_t tj = 0; tj <= ti; ++tj) {
                    mblk_prob.push_back(g);
                    mblk_tile.push_back(ti << 16 | tj);
                }
        }
        mblk_at[q + 1] = mblk_prob.size();
    }
    const size_t o_mtab = L.take(sizeof(wm_prob) * std::max(NM, 1)), o_mord = L.take(4 * (size_t)std::max(NM, 1));
    const size_t o_mbp = L.take(4 * std::max<size_t>(mblk_prob.size(), 1)), o_mbt = L.take(4 * std::max<size_t>(mblk_tile.size(), 1));
    int64_t mlog_ints = 0;
    for (int32_t g = 0; g < NM; ++g) mlog_ints += 2 * (int64_t)n[mid[g]] + 1;
    const size_t o_mlogs = L.take(4 * (size_t)std::max<int64_t>(mlog_ints, 1));
    const size_t o_mws = L.take(mid_ws);
    char *ws = nullptr;
    ICL_TRY(wm_ensure(ctx, L.off, &ws));
    if (h_E && need_e) {
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_e, h_E, (size_t)e_len * 4, hipMemcpyHostToDevice, ctx->stream));
        d_E = (const float *)(ws + o_e);
    }
    std::vector<const float *> rowsE(nprob, nullptr);
    for (int32_t p = 0; p < nprob; ++p) {
        if (!route[p]) continue;
        rowsE[p] = d_E + e_off[p];
        if (o_al[p] != SIZE_MAX) {
            ICL_HIP(ctx, hipMemcpyAsync(ws + o_al[p], rowsE[p], (size_t)n[p] * d[p] * 4, hipMemcpyDeviceToDevice, ctx->stream));
            rowsE[p] = (const float *)(ws + o_al[p]);
        }
    }
    std::vector<int32_t> hlog((size_t)std::max<int64_t>(log_ints, 1));
    std::vector<int64_t> log_at(G);
    if (G) {
        std::vector<wm_prob> tab(G);
        int64_t at = 0, lds = 0;
        for (int32_t g = 0; g < G; ++g) {
            const int32_t p = gpu[g];
            wm_prob &w = tab[g];
            w.E = rowsE[p];
            w.C = (float *)(ws + o_c[g]);
            w.tri = (float *)(ws + o_t[g]);
            w.n = n[p];
            w.d = d[p];
            w.max_size = max_size[p];
            w.T = (int32_t)(n[p] - k[p]);
            log_at[g] = at;
            w.log = (int32_t *)(ws + o_logs) + at;
            w.nm = w.log + 2 * (int64_t)n[p];
            at += 2 * (int64_t)n[p] + 1;
            w.lds_tri = wm_lds_bytes(n[p], true) <= WM_LDS_MAX ? 1 : 0;
            w.pad = 0;
            lds = std::max(lds, wm_lds_bytes(n[p], w.lds_tri != 0));
        }
        std::vector<int32_t> ord(G);
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return n[gpu[a]] > n[gpu[b]]; }); // largest problems first
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_tab, tab.data(), sizeof(wm_prob) * G, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_ord, ord.data(), 4 * (size_t)G, hipMemcpyHostToDevice, ctx->stream));
        if (!blk_prob.empty()) {
            ICL_HIP(ctx, hipMemcpyAsync(ws + o_bp, blk_prob.data(), 4 * blk_prob.size(), hipMemcpyHostToDevice, ctx->stream));
            ICL_HIP(ctx, hipMemcpyAsync(ws + o_bq, blk_pair0.data(), 8 * blk_pair0.size(), hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(ward_many_init_kernel, dim3((unsigned)blk_prob.size()), dim3(WM_THREADS), 0, ctx->stream, (const wm_prob *)(ws + o_tab),
                               (const int32_t *)(ws + o_bp), (const int64_t *)(ws + o_bq));
            ICL_HIP(ctx, hipGetLastError());
        }
        icl_lds_optin(ctx, (const void *)ward_many_merge_kernel, WM_LDS_MAX);
        hipLaunchKernelGGL(ward_many_merge_kernel, dim3((unsigned)G), dim3(WM_THREADS), (unsigned)lds, ctx->stream, (const wm_prob *)(ws + o_tab),
                           (const int32_t *)(ws + o_ord));
        ICL_HIP(ctx, hipGetLastError());
        ICL_HIP(ctx, hipMemcpyAsync(hlog.data(), ws + o_logs, 4 * (size_t)log_ints, hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<int32_t> hmlog((size_t)std::max<int64_t>(mlog_ints, 1));
    std::vector<int64_t> mlog_at(NM);
    std::vector<wm_prob> mtab(NM);
    std::vector<int32_t> mord(NM);
    if (NM) {
        int64_t at = 0;
        for (int32_t q = 0; q < NG; ++q) {
            wm_layout R; // this group's share of the reused region
            for (int32_t g = grp_at[q]; g < grp_at[q + 1]; ++g) {
                const int32_t p = mid[g];
                wm_prob &w = mtab[g];
                w.E = rowsE[p];
                w.C = (float *)(ws + o_mws + R.take((size_t)n[p] * d[p] * 4));
                w.tri = (float *)(ws + o_mws + R.take((size_t)n[p] * n[p] * 4));
                w.n = n[p];
                w.d = d[p];
                w.max_size = max_size[p];
                w.T = (int32_t)(n[p] - k[p]);
                mlog_at[g] = at;
                w.log = (int32_t *)(ws + o_mlogs) + at;
                w.nm = w.log + 2 * (int64_t)n[p];
                at += 2 * (int64_t)n[p] + 1;
                w.lds_tri = 0;
                w.pad = 0;
                mord[g] = g; // (mid is sorted: largest first)
            }
        }
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_mtab, mtab.data(), sizeof(wm_prob) * NM, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_mord, mord.data(), 4 * (size_t)NM, hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_mbp, mblk_prob.data(), 4 * mblk_prob.size(), hipMemcpyHostToDevice, ctx->stream));
        ICL_HIP(ctx, hipMemcpyAsync(ws + o_mbt, mblk_tile.data(), 4 * mblk_tile.size(), hipMemcpyHostToDevice, ctx->stream));
        icl_lds_optin(ctx, (const void *)ward_many_mid_merge_kernel, WM_LDS_MAX);
        for (int32_t q = 0; q < NG; ++q) { // one init launch and one merge launch per group
            const size_t nb = mblk_at[q + 1] - mblk_at[q];
            hipLaunchKernelGGL(ward_many_mid_init_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (const wm_prob *)(ws + o_mtab),
                               (const int32_t *)(ws + o_mbp) + mblk_at[q], (const int32_t *)(ws + o_mbt) + mblk_at[q]);
            ICL_HIP(ctx, hipGetLastError());
            const int64_t lds = wmm_lds_bytes(n[mid[grp_at[q]]]); // the group's largest problem
            hipLaunchKernelGGL(ward_many_mid_merge_kernel, dim3((unsigned)(grp_at[q + 1] - grp_at[q])), dim3(WMM_THREADS), (unsigned)lds, ctx->stream,
                               (const wm_prob *)(ws + o_mtab), (const int32_t *)(ws + o_mord) + grp_at[q]);
            ICL_HIP(ctx, hipGetLastError());
        }
        ICL_HIP(ctx, hipMemcpyAsync(hmlog.data(), ws + o_mlogs, 4 * (size_t)mlog_ints, hipMemcpyDeviceToHost, ctx->stream));
    }
    // the large-N route, one problem at a time, behind the launches above (its reports of the last icl_cluster are restored)
    std::vector<std::vector<int32_t>> big_log(nprob);
    {
        wm_last_guard keep(ctx);
        for (int32_t p = 0; p < nprob; ++p) {
            if (route[p] != 2) continue;
            int32_t nc = 0;
            const int rc = icl_ward_cluster_exact(ctx, rowsE[p], n[p], d[p], min_size[p], max_size[p], cluster_id + img[p], member_rank + img[p], &nc,
                                                  &big_log[p]);
            n_clusters[p] = nc;
            if (rc != ICL_OK) {
                st[p] = rc;
                why[p] = ctx->err;
            }
        }
    }
    if (G || NM) ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<int32_t> mid_of(NM ? nprob : 0, -1); // problem -> its place in mid
    for (int32_t g = 0; g < NM; ++g) mid_of[mid[g]] = g;
    // ids from the merge logs (clustering.go:265-280, ward.hip's rule), merge logs, statuses
    std::vector<int32_t> pairs;
    for (int32_t p = 0, g = 0; p < nprob; ++p) {
        int32_t *cid = cluster_id + img[p], *rank = member_rank + img[p];
        int64_t nm = 0;
        if (route[p] == 1) {
            const int32_t *lg = hlog.data() + log_at[g++];
            nm = lg[2 * (int64_t)n[p]];
            pairs.assign(lg, lg + 2 * nm);
        } else if (route[p] == 3) {
            const int32_t *lg = hmlog.data() + mlog_at[mid_of[p]];
            nm = lg[2 * (int64_t)n[p]];
            pairs.assign(lg, lg + 2 * nm);
        } else if (route[p] == 2) {
            pairs.swap(big_log[p]);
            nm = (int64_t)pairs.size() / 2;
        } else
            pairs.clear();
        if (st[p] == ICL_OK && route[p] != 2) {
            const int rc = icl_ward_assign_ids(ctx, n[p], min_size[p], max_size[p], pairs, nm, cid, rank, &n_clusters[p]);
            if (rc != ICL_OK) {
                st[p] = rc;
                why[p] = ctx->err;
            }
        }
        if (st[p] != ICL_OK) {
            std::fill(cid, cid + n[p], -1);
            std::fill(rank, rank + n[p], -1);
            n_clusters[p] = 0;
            nm = 0;
        }
        n_merges[p] = (int32_t)nm;
        if (merges && nm) memcpy(merges + 2 * img[p], pairs.data(), 8 * (size_t)nm);
        status[p] = st[p];
    }
    for (int32_t p = 0; p < nprob; ++p)
        if (st[p] != ICL_OK) return icl_fail(ctx, st[p], "icl_cluster_many: problem %d: %s", p, why[p].c_str());
    return ICL_OK;
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
