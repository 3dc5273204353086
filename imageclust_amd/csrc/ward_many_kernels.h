// ward_many_kernels.h -- the four kernels of ward_many.hip's one-workgroup routes.  Not a header of its own: ward_many.hip includes it
// three times, after everything the kernels share.  WM_SEEDED 0: the kernels behind icl_cluster_many[_dev] and icl_cluster_requests[_mem], every
// problem starting from singletons (ward_many_init_kernel, ...).  WM_SEEDED 1: the same text with the start state taken from a wm_seed
// table, the kernels' last argument (ward_many_init_seeded_kernel, ...): slot t starts as seed t -- size SD[g].size[t], creation id t,
// centroid row t of E -- a pair whose sizes exceed max_size is banned from the start, and the merge kernels leave the slots' final
// creation ids in SD[g].fin.  The first inclusion compiles to the code it was before there were seeds (scratch/isa_compare.py).
// WM_SEEDED 1 with WM_APART 1: the seeded text with a KEEP-APART relation over the live clusters (ward_many_init_apart_kernel, ...,
// icl_cluster_many_apart; DESIGN.md "Constrained seeded clustering").  The table is wm_apart: sizes and fin as in wm_seed, and the
// problem's bit rows in the global workspace -- bit u of row t (W words a row) set when the clusters in slots t and u are apart.  A pair
// whose bit is set holds MaxFloat32 from the start and is never evaluated; a merged cluster inherits the bans of both parents (wm_apart_
// inherit below).  The first two inclusions compile to the code they were before there was a relation.
#if WM_APART
#define WM_KERNEL(name) name##_apart_kernel
#define WM_SEED_PARAM , const wm_apart *__restrict__ SD
#elif WM_SEEDED
#define WM_KERNEL(name) name##_seeded_kernel
#define WM_SEED_PARAM , const wm_seed *__restrict__ SD
#else
#define WM_KERNEL(name) name##_kernel
#define WM_SEED_PARAM
#endif

// ComputeInitialDistanceMatrix (clustering.go:61-73) of every problem: block b covers pairs [pair0[b], pair0[b] + 256) of problem prob[b]
__global__ __launch_bounds__(WM_THREADS) void WM_KERNEL(ward_many_init)(const wm_prob *__restrict__ P, const int32_t *__restrict__ blk_prob,
                                                                    const int64_t *__restrict__ blk_pair0 WM_SEED_PARAM)
{
    const wm_prob p = P[blk_prob[blockIdx.x]];
    const int64_t q = blk_pair0[blockIdx.x] + threadIdx.x;
    if (q >= wm_tri_len(p.n)) return;
    int64_t i = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5); // row i holds pairs [i (i - 1) / 2, i (i + 1) / 2)
    while (i * (i - 1) / 2 > q) --i;
    while ((i + 1) * i / 2 <= q) ++i;
    const int64_t j = q - i * (i - 1) / 2;
#if WM_SEEDED
    const int32_t *ssz = SD[blk_prob[blockIdx.x]].size;
    const int si = ssz[i], sj = ssz[j];
    float v = ICL_MAXF; // a pair whose sizes exceed max_size is banned from the start (clustering.go:228-234) and never evaluated
#if WM_APART
    if (si + sj <= p.max_size && !wm_apart_bit(SD[blk_prob[blockIdx.x]].bits + i * SD[blk_prob[blockIdx.x]].words, (int)j)) // (nor a pair kept apart)
#else
    if (si + sj <= p.max_size)
#endif
        v = ward_pair_value(p.E + i * p.d, p.E + j * p.d, p.d, si, sj);
#else
    float v = ICL_MAXF; // max_size < 2: every pair of singletons is banned (clustering.go:228-234) and never read
    if (p.max_size >= 2) v = ward_pair_value(p.E + i * p.d, p.E + j * p.d, p.d, 1, 1); // WardDistance(clusters[i], clusters[j]) :66
#endif
    p.tri[q] = v;
}

__global__ __launch_bounds__(WM_THREADS) void WM_KERNEL(ward_many_merge)(const wm_prob *__restrict__ P, const int32_t *__restrict__ order WM_SEED_PARAM)
{
    extern __shared__ __align__(16) unsigned char wm_lds[];
    const wm_prob p = P[order[blockIdx.x]];
    const int n = p.n, d = p.d, maxs = p.max_size;
    const wm_slots S = wm_carve(wm_lds, n, WM_WAVES);
    uint64_t *const rkey = S.rkey;
    int32_t *const rarg = S.rarg, *const sz = S.sz, *const cid = S.cid;
#if WM_APART
    uint32_t *const abits = SD[order[blockIdx.x]].bits;
    const int aw = SD[order[blockIdx.x]].words;
#endif
    float *tri = p.tri;
    if (p.lds_tri) {
        float *lt = reinterpret_cast<float *>(wm_lds + wm_meta_bytes(n));
        const int64_t len = wm_tri_len(n);
        for (int64_t q = threadIdx.x; q < len; q += WM_THREADS) lt[q] = p.tri[q];
        tri = lt;
    }
    for (int t = threadIdx.x; t < n; t += WM_THREADS) {
#if WM_SEEDED
        sz[t] = SD[order[blockIdx.x]].size[t];
#else
        sz[t] = 1;
#endif
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
#if WM_APART
        wm_apart_or_row<WM_THREADS>(abits, aw, sn, shi); // (row shi is dead: nobody writes it; the step's closing barrier publishes row sn)
#endif
        uint64_t nk = ~0ull;
        int nr = -1;
        uint32_t stale = 0; // rows of this thread whose cached partner just died
        for (int t = threadIdx.x, m = 0; t < n; t += WM_THREADS, ++m) {
            if (t == sn || sz[t] == 0) continue;
            const int st = sz[t];
            float v = ICL_MAXF; // banned: never selected (:228-234), never evaluated
#if WM_APART
            const bool okp = !wm_apart_inherit(abits + (int64_t)t * aw, shi, slo) && st + snew <= maxs; // (the owner of row t: its bit for sn)
            if (okp) v = ward_pair_value(cent(t), cn, d, st, snew);
            at(t, sn) = v;
            const uint64_t k = (okp && v < ICL_MAXF) ? wm_key(v, cid[t], cnew) : ~0ull;
#else
            if (st + snew <= maxs) v = ward_pair_value(cent(t), cn, d, st, snew);
            at(t, sn) = v;
            const uint64_t k = (st + snew <= maxs && v < ICL_MAXF) ? wm_key(v, cid[t], cnew) : ~0ull;
#endif
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
#if WM_SEEDED
    int32_t *fin = SD[order[blockIdx.x]].fin; // (every step, and the set-up, ended with a barrier)
    for (int t = threadIdx.x; t < n; t += WM_THREADS) fin[t] = sz[t] ? cid[t] : -1;
#endif
}

// ComputeInitialDistanceMatrix (clustering.go:61-73) into the full square: block b computes the 64 x 64 pairs (i, j) of tile
// (ti, tj), ti >= tj, of problem blk_prob[b]; k-chunks of both row sets are staged in LDS, every thread holds 4 x 4 pairs, and every
// pair's sum is s = s + fl(fl(x_k - y_k)^2) strictly in k order -- the value ward_pair_value(E_i, E_j, d, 1, 1) returns.
__global__ __launch_bounds__(256) void WM_KERNEL(ward_many_mid_init)(const wm_prob *__restrict__ P, const int32_t *__restrict__ blk_prob,
                                                                 const int32_t *__restrict__ blk_tile WM_SEED_PARAM)
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
    if (WM_SEEDED || p.max_size >= 2) {
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
#if WM_SEEDED
            const int32_t *ssz = SD[blk_prob[blockIdx.x]].size; // a pair whose sizes exceed max_size is banned from the start
            const int si = ssz[i], sj = ssz[j];
#if WM_APART
            const bool okp = i != j && si + sj <= p.max_size && !wm_apart_bit(SD[blk_prob[blockIdx.x]].bits + (int64_t)i * SD[blk_prob[blockIdx.x]].words, j);
#else
            const bool okp = i != j && si + sj <= p.max_size;
#endif
            const float v = okp ? ward_scale(s[a][b], si, sj) : ICL_MAXF;
#else
            const float v = (p.max_size >= 2 && i != j) ? ward_scale(s[a][b], 1, 1) : ICL_MAXF;
#endif
            p.tri[(int64_t)i * n + j] = v;
            p.tri[(int64_t)j * n + i] = v;
        }
}

__global__ __launch_bounds__(WMM_THREADS) void WM_KERNEL(ward_many_mid_merge)(const wm_prob *__restrict__ P, const int32_t *__restrict__ order WM_SEED_PARAM)
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
#if WM_APART
    uint32_t *const abits = SD[order[blockIdx.x]].bits;
    const int aw = SD[order[blockIdx.x]].words;
#endif
    for (int t = tid; t < n; t += WMM_THREADS) {
#if WM_SEEDED
        sz[t] = SD[order[blockIdx.x]].size[t];
#else
        sz[t] = 1;
#endif
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
#if WM_APART
        wm_apart_or_row<WMM_THREADS>(abits, aw, sn, shi); // (row shi is dead: nobody writes it; the step's closing barrier publishes row sn)
#endif
        for (int t0 = 0; t0 < n; t0 += WMM_THREADS) {
            const int t = t0 + tid;
            const bool live = t < n && t != sn && sz[t] != 0;
#if WM_APART
            const bool evalp = live && !wm_apart_inherit(abits + (int64_t)t * aw, shi, slo) && sz[t] + snew <= maxs; // (the owner of row t: its bit for sn)
#else
            const bool evalp = live && sz[t] + snew <= maxs;
#endif
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
#if WM_SEEDED
    int32_t *fin = SD[order[blockIdx.x]].fin; // (every step, and the set-up, ended with a barrier)
    for (int t = tid; t < n; t += WMM_THREADS) fin[t] = sz[t] ? cid[t] : -1;
#endif
}

#undef WM_KERNEL
#undef WM_SEED_PARAM
