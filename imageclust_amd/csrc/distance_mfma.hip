// distance_mfma.hip -- K6: the pairwise Ward (half squared Euclidean) matrix in GEMM form on the matrix cores,
//     D~[i][j] = 0.5*(|e_i|^2 + |e_j|^2) - e_i . e_j          (north_star: "-2 E E^T on MFMA plus broadcast row-norms")
// for the FAST clustering mode (ICL_UPDATE_LW) and as a stand-alone entry point (icl_distance_mfma_dev).
//
// It replaces the arithmetic of ComputeInitialDistanceMatrix (/root/reference/internal/clustering/clustering.go:61-73)
// only approximately: the GEMM form sums in a different order and cancels, so its low bits differ from the reference's
// sequential sum (clustering.go:137-141,152-155).  The bit-exact tile is ward_dist_exact_kernel (ward.hip); cluster
// ids produced from D~ are reported, never asserted, against the reference.  Entries are stored clamped to >= +0 (NaN kept).
//
// Precision: fp32 operands are split e = hi + lo with hi = bf16(e), lo = bf16(e - hi) and the dot product is
// hi.hi + hi.lo + lo.hi (the lo.lo term is below fp32 resolution): the three products are ONE bf16 GEMM over the
// concatenated K axis  A' = [hi | hi | lo],  B' = [hi | lo | hi]  (K' = 3*D), fp32 accumulate -> ~2^-16 relative to
// |e_i||e_j| per term.  Tiles, LDS image, LDS-DMA staging and the MFMA sweep are the convolution kernel's
// (mfma_tile.h): 128x128 outputs per workgroup, lower-triangle tiles only.
#include "icl_common.h"
#include "distance.h"
#include "mfma_tile.h"

#include <algorithm>

// E [n][d] fp32 -> A' / B' [n][3*dp] bf16 (dp = d rounded up to 64, zero padded) and norms[n] = sum e^2 (fp32).
__global__ __launch_bounds__(256) void dist_split_kernel(const float *__restrict__ E, int64_t n, int d, int dp,
                                                        uint16_t *__restrict__ A, uint16_t *__restrict__ B, float *__restrict__ norms)
{
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    float acc = 0.0f;
    for (int k = threadIdx.x; k < dp; k += 256) {
        const float e = k < d ? E[r * d + k] : 0.0f;
        const uint16_t hi = BF16::from_f(e);
        const uint16_t lo = BF16::from_f(e - BF16::to_f(hi));
        acc += e * e;
        uint16_t *a = A + r * 3 * dp, *b = B + r * 3 * dp;
        a[k] = hi; a[dp + k] = hi; a[2 * dp + k] = lo;
        b[k] = hi; b[dp + k] = lo; b[2 * dp + k] = hi;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) norms[r] = red[0] + red[1] + red[2] + red[3];
}

struct dist_args {
    const uint16_t *A, *B; // [n][K]
    const float *norms;
    const void *zero;
    float *out;
    const int64_t *rowoff; // packed lower triangle (MODE 0) or nullptr
    int64_t n, ld;
    int K;
};

// ---- the GEMM tile both kernels below run (the convolution kernel's tile machinery, mfma_tile.h) -------------------------------
#define DG_BN 128                              /* tile columns (rows are CV_BM = 128) */
#define DG_STAGE ((DG_BN + CV_BM) * CV_ROWB)   /* bytes of one k-step of both operands; two stages are in flight */
#define DG_EP_LD (DG_BN + 4)                   /* pitch of the finished fp32 tile, which reuses the stages */

// c[i][j] = sum_k X[i0 + i][k] * W[j0 + j][k] for the 128 x 128 pairs of a tile, left as fp32 at smem[i * DG_EP_LD + j] behind a
// barrier.  X, W: [n][K] elements of T (K a multiple of T::BK); rows past n read the zero page.  All 256 threads of the workgroup.
template <typename T>
__device__ __forceinline__ void dist_gemm_tile(const typename T::elem *X, const typename T::elem *W, int64_t n, int K, const void *zero, int64_t i0,
                                               int64_t j0, unsigned char *smem)
{
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    // staging roles: one LDS-DMA piece = 8 rows x 128 B; "x" rows = i (lane of the MFMA result), "w" rows = j
    const int prow = lane >> 3, ps = lane & 7;
    const typename T::elem *xsrc[4], *wsrc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = wid * 32 + q * 8 + prow;
        const int64_t ri = i0 + row, rj = j0 + row;
        xsrc[q] = ri < n ? X + ri * K + lds_swz(row, ps) * T::KE : nullptr;
        wsrc[q] = rj < n ? W + rj * K + lds_swz(row, ps) * T::KE : nullptr;
    }
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const unsigned wave_off = __builtin_amdgcn_readfirstlane(wid * 32 * CV_ROWB);
    int k0 = 0;
    auto stage = [&](int buf) {
        const unsigned wdst = smem_base + buf * DG_STAGE + wave_off, xdst = wdst + DG_BN * CV_ROWB;
#pragma unroll
        for (int q = 0; q < 4; ++q) glds16_asm(wsrc[q] ? (const void *)(wsrc[q] + k0) : zero, wdst + q * 8 * CV_ROWB);
#pragma unroll
        for (int q = 0; q < 4; ++q) glds16_asm(xsrc[q] ? (const void *)(xsrc[q] + k0) : zero, xdst + q * 8 * CV_ROWB);
        k0 += T::BK;
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    const int nk = K / T::BK;
    stage(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    for (int ks = 0; ks < nk; ++ks) {
        const int cur = ks & 1;
        if (ks + 1 < nk) stage(cur ^ 1);
        const unsigned char *wsm = smem + cur * DG_STAGE;
        conv_mma_kstep<T, DG_BN>(wsm, wsm + DG_BN * CV_ROWB, wm, wn, fr, fh, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // accumulators (lane = i, register quads = 4 consecutive j) -> fp32 LDS tile [i][j]
    float *ep = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int ml = wm * 64 + b * 32 + fr;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int nl = wn * 64 + a * 32 + 8 * g + 4 * fh;
                *reinterpret_cast<float4 *>(ep + ml * DG_EP_LD + nl) =
                    make_float4(acc[a][b][4 * g + 0], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
            }
    }
    __syncthreads();
}

// The finished tile as coalesced rows: entry (i, j) = value(nrm[i], nrm[j], c[i][j]).  32 lanes x 4 floats = one 128-wide tile row, 8
// rows per pass.  MODE 0: packed lower triangle, j < i at out[rowoff[i] + j];  MODE 1: dense rows, j <= i at out[i * ld + j], 0 at j == i.
template <int MODE, typename F>
__device__ __forceinline__ void dist_store_rows(const unsigned char *smem, const float *nrm, int64_t n, int64_t i0, int64_t j0, float *out,
                                                const int64_t *rowoff, int64_t ld, F value)
{
    const float *ep = reinterpret_cast<const float *>(smem);
    const int tid = threadIdx.x, nl = (tid & 31) * 4;
    float nj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) nj[q] = (j0 + nl + q) < n ? nrm[j0 + nl + q] : 0.0f;
    for (int ml = tid >> 5; ml < CV_BM; ml += 8) {
        const int64_t i = i0 + ml;
        if (i >= n) break;
        const float ni = nrm[i];
        const float4 t = *reinterpret_cast<const float4 *>(ep + ml * DG_EP_LD + nl);
        const float v[4] = {value(ni, nj[0], t.x), value(ni, nj[1], t.y), value(ni, nj[2], t.z), value(ni, nj[3], t.w)};
        const int64_t jb = j0 + nl;
        const int64_t lim = MODE == 0 ? i : i + 1; // columns j < lim are written
        float *row = MODE == 0 ? out + rowoff[i] : out + i * ld;
        if (jb + 3 < i && ((MODE == 0) || ((ld & 3) == 0))) { // strictly below the diagonal: one 16-byte store
            *reinterpret_cast<float4 *>(row + jb) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (jb + q < lim) row[jb + q] = (MODE == 1 && jb + q == i) ? 0.0f : v[q];
        }
    }
}

// D~ of the whole triangle in row-major tile order (MODE: dist_store_rows).
template <int MODE>
__global__ __launch_bounds__(256) void dist_mfma_kernel(const dist_args p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ti, tj;
    tri_decode32(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * CV_BM, j0 = (int64_t)tj * DG_BN;
    dist_gemm_tile<BF16>(p.A, p.B, p.n, p.K, p.zero, i0, j0, smem);
    // the true value is >= 0; the estimate of (near-)duplicate rows is rounding noise of either sign.  Negative and -0 are stored as +0, a NaN stays
    // a NaN: the merge loop's (value bits, id) keys then order every entry of the matrix as its value does (ward.hip, ward_lw_value)
    dist_store_rows<MODE>(smem, p.norms, p.n, i0, j0, p.out, p.rowoff, p.ld, [](float ni, float nj, float c) {
        const float v = 0.5f * (ni + nj) - c;
        return v > 0.0f ? v : (v == v ? 0.0f : v);
    });
}

static size_t dist_lds_bytes()
{
    const size_t stages = 2 * (size_t)DG_STAGE, ep = (size_t)CV_BM * DG_EP_LD * 4;
    return std::max(stages, ep);
}

// (the sized tile, at the end of this file)
static void dist_sized_enqueue(icl_ctx *ctx, const dist_args &a, const int32_t *d_items, unsigned nblocks);

// Shared by icl_distance_mfma_dev and the LW clustering mode (ward.hip).  Scratch: A', B', norms, the zero page.  d_items (may be null): the
// rows are clusters of that many items and the sized tile runs (icl_dist_mfma_sized_launch).
static int dist_mfma_run(icl_ctx *ctx, const float *d_E, int64_t n, int d, const int32_t *d_items, float *d_out, const int64_t *d_rowoff, int64_t ld)
{
    if (n <= 0) return ICL_OK;
    const int dp = (d + 63) / 64 * 64;
    const int K = 3 * std::max(dp, 64);
    const int dpe = K / 3;
    dev_guard gA, gB, g_norms, g_zero; // (the caller holds ctx->mu and has the device selected)
    ICL_TRY(icl_dev_alloc(ctx, gA, (size_t)n * K * 2, "distance GEMM: A' (%lld x %d)", (long long)n, K));
    ICL_TRY(icl_dev_alloc(ctx, gB, (size_t)n * K * 2, "distance GEMM: B' (%lld x %d)", (long long)n, K));
    ICL_TRY(icl_dev_alloc(ctx, g_norms, (size_t)n * 4, "distance GEMM: norms"));
    ICL_TRY(icl_dev_alloc(ctx, g_zero, 256, "distance GEMM: zero page"));
    uint16_t *A = gA.as<uint16_t>(), *B = gB.as<uint16_t>();
    float *norms = g_norms.as<float>();
    void *zero = g_zero.p;
    ICL_HIP(ctx, hipMemsetAsync(zero, 0, 256, ctx->stream));
    hipLaunchKernelGGL(dist_split_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, d_E, n, d, dpe, A, B, norms);
    icl_lds_optin(ctx, (const void *)dist_mfma_kernel<0>, (int)dist_lds_bytes());
    icl_lds_optin(ctx, (const void *)dist_mfma_kernel<1>, (int)dist_lds_bytes());
    dist_args a{A, B, norms, zero, d_out, d_rowoff, n, ld, K};
    int64_t nblocks;
    ICL_TRY(icl_dist_grid(ctx, 0, icl_ceil_div(n, CV_BM), &nblocks));
    {
        const double pairs = (double)n * (double)(n + 1) * 0.5;
        icl_prof_scope ps(ctx, ICL_K_DIST_MFMA, 2.0 * pairs * d, 4.0 * pairs + 4.0 * (double)n * d);
        if (d_items)
            dist_sized_enqueue(ctx, a, d_items, (unsigned)nblocks);
        else if (d_rowoff)
            hipLaunchKernelGGL(dist_mfma_kernel<0>, dim3((unsigned)nblocks), dim3(256), dist_lds_bytes(), ctx->stream, a);
        else
            hipLaunchKernelGGL(dist_mfma_kernel<1>, dim3((unsigned)nblocks), dim3(256), dist_lds_bytes(), ctx->stream, a);
    }
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icl_prof_collect(ctx);
    return ICL_OK;
}
int icl_dist_mfma_launch(icl_ctx *ctx, const float *d_E, int64_t n, int d, float *d_out, const int64_t *d_rowoff, int64_t ld)
{
    return dist_mfma_run(ctx, d_E, n, d, nullptr, d_out, d_rowoff, ld);
}
int icl_dist_mfma_sized_launch(icl_ctx *ctx, const float *d_C, int64_t m, int d, const int32_t *d_items, float *d_out, const int64_t *d_rowoff, int64_t ld)
{
    return dist_mfma_run(ctx, d_C, m, d, d_items, d_out, d_rowoff, ld);
}

// ------------------------------------------------------------------------------------------------------------
// Distance BOUNDS for the exact mode (round 3): ComputeInitialDistanceMatrix (clustering.go:61-73) costs 3 D unfused fp32 ops
// per pair on the vector ALUs (ward_dist_exact_kernel: 0.49 s at N = 100 000, D = 2048).  Only the few entries near a row's
// minimum ever decide anything, so the matrix is first filled with PROVEN LOWER BOUNDS from a GEMM on the matrix cores and an
// entry is evaluated exactly -- sequential unfused fp32, the reference's own expression -- only when a row scan finds its
// bound inside the band that could hold the row's minimum (ward.hip, scan_row_refine).  Nothing the reference compares is
// ever taken from the GEMM.
//
// The GEMM runs on f32 operands with v_mfma_f32_32x32x2_f32, whose result is, bit for bit, a k-ordered chain of fp32 fmaf
// (MI355X_MICROARCH.md "Matrix cores": one rounding per product, no wider accumulation) -- an operation with a textbook error
// bound, unlike the bf16 forms' unspecified internal accumulation.  Operands are the rows of E minus a common vector mu (the
// column means; any mu is valid, a good one shrinks the norms and with them the bound):  a' = fl(a - mu).
//
// Bound (u = 2^-24, D' = D rounded up to 32, S = sum_k (a_k - b_k)^2 in exact arithmetic):
//   reference value R = fl(0.5 * s^) with s^ the sequential fp32 sum of fl(fl(a_k - b_k)^2): every term is non-negative, so
//       s^ = sum (a_k - b_k)^2 (1 + eta_k),  |eta_k| <= (1 + u)^(D + 2) - 1 =: g'      =>  R in [S/2 (1 - g'), S/2 (1 + g')]
//       (the scaling by 0.5 is exact; gradual underflow of tiny products adds at most D 2^-149, absorbed by the floor below).
//   estimate  T = 0.5 (n_a + n_b) - c,  n_a = computed |a'|^2,  c = fmaf chain of a'.b':
//       |c - a'.b'| <= gD sum |a'_k b'_k| <= gD (|a'|^2 + |b'|^2) / 2,  gD = D' u / (1 - D' u)        (fma chain, any order)
//       |n_a - |a'|^2| <= 20 u |a'|^2                      (dist_center_kernel: <= 20 roundings on any path of its summation tree)
//       the three fp32 operations that form T from n_a, n_b, c add <= 3 u (|a'|^2 + |b'|^2) (1 + 20 u)
//       centring: a' - b' = (a - b) + da + db, |da_k| <= u |a_k - mu_k| = u |a'_k| / (1 - u):
//           | |a' - b'|^2 / 2 - S / 2 | <= u (|a'| + |b'|)^2 (1 + 2u) <= 2 u (|a'|^2 + |b'|^2) (1 + 2u)
//   together   | T - S/2 | <= E_ab := (gD / 2 + 16 u)(1 + 64 u)(n_a + n_b)      (n_a, n_b: the COMPUTED norms, hence the slack factor)
//   stored     L = max(0, (T - E_ab)(1 - g')) rounded toward zero, with the sign bit set as the "bound, not value" flag (-0.0: L = 0)
//   scan side  U(L) = (L (1 + 3 g') + 2 E_ab)(1 + g') >= R     (T <= L / ((1 - g')(1 - 2u)) + E_ab  and  R <= (T + E_ab)(1 + g'))
// ------------------------------------------------------------------------------------------------------------
// column sums of E (double accumulators: accuracy is irrelevant for correctness, any mu is valid -- but every GPU of a job must derive the SAME mu
// from the same E, bit for bit: the rows one GPU computes for another's matrix mean there what they mean here.  Fixed partition, fixed order: each of
// DIST_CS_PARTS row ranges leaves its partial sums in part[y][k], one thread per column then adds them in ascending y.  Until round 5 the partial
// sums were atomicAdd'ed: the order of the additions, and with it mu's last bits, changed from run to run.)
#define DIST_CS_PARTS 256
__global__ __launch_bounds__(256) void dist_colsum_kernel(const float *__restrict__ E, int64_t n, int d, double *__restrict__ part)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= d) return;
    const int64_t per = (n + gridDim.y - 1) / gridDim.y, lo = (int64_t)blockIdx.y * per, hi = lo + per < n ? lo + per : n;
    double acc = 0.0;
    for (int64_t r = lo; r < hi; ++r) acc += (double)E[r * d + k];
    part[(int64_t)blockIdx.y * d + k] = acc;
}
__global__ __launch_bounds__(256) void dist_colsum_join_kernel(const double *__restrict__ part, int parts, int d, double *__restrict__ sum)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= d) return;
    double acc = 0.0;
    for (int y = 0; y < parts; ++y) acc += part[(int64_t)y * d + k];
    sum[k] = acc;
}
// Ec[r][k] = fl(E[r][k] - mu[k]) (zero beyond d), nrm[r] = |Ec[r]|^2 by a balanced tree: thread t squares its elements k = t,
// t + 256, ... and sums them pairwise (a binary counter of partial sums by level), then the wave's shuffle tree, then the four
// wave totals.  Roundings on any path: 1 (square) + at most 2 log2(ceil(D'/256)) (pairwise + the final collapse of the levels)
// + 6 + 2 -- at most 19 for D' <= 8192, inside the 20 u of the bound above (icl_dist_bound_usable: larger D take the exact kernel).
__global__ __launch_bounds__(256) void dist_center_kernel(const float *__restrict__ E, int64_t n, int d, int dp, const double *__restrict__ sum,
                                                         float *__restrict__ Ec, float *__restrict__ nrm)
{
    __shared__ float red[4];
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    // pairwise (balanced) summation of this thread's squares: element index stride 256; a stack of partial sums by level
    float lvl[12];
    unsigned have = 0;
    const double inv_n = 1.0 / (double)n;
    for (int k = threadIdx.x; k < dp; k += 256) {
        float e = 0.0f;
        if (k < d) {
            const float mu = (float)(sum[k] * inv_n);
            e = E[r * d + k] - mu;
        }
        Ec[r * dp + k] = e;
        float v = e * e;
        int l = 0;
        while (have & (1u << l)) { // carry: two partial sums of the same level merge into the next one
            v = lvl[l] + v;
            have &= ~(1u << l);
            ++l;
        }
        lvl[l] = v;
        have |= 1u << l;
    }
    float acc = 0.0f;
    bool any = false;
    for (int l = 0; l < 12; ++l)
        if (have & (1u << l)) {
            acc = any ? acc + lvl[l] : lvl[l];
            any = true;
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) nrm[r] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct dbound_args {
    const float *Ec; // [n][K] centred rows, K = D rounded up to 32
    const float *nrm;
    const void *zero;
    float *out;
    const int64_t *rowoff;
    int64_t n, tr_lo, tr_hi;
    int K;
    float ceps, gam; // E_ab = ceps (n_a + n_b); gam = g'
};

// 128 x 128 pairs per workgroup on v_mfma_f32_32x32x2_f32 (the f32 form of the tile above), tiles in dist_tile.h's band order;
// out[rowoff[i] + j] = flagged lower bound of the Ward value of singletons i > j.
__global__ __launch_bounds__(256) void dist_bound_kernel(const dbound_args p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ti, tj;
    tri_band_decode(xcd_remap((int)blockIdx.x, (int)gridDim.x), p.tr_lo, p.tr_hi, ti, tj);
    const int64_t i0 = (int64_t)ti * CV_BM, j0 = (int64_t)tj * DG_BN;
    dist_gemm_tile<F32>(p.Ec, p.Ec, p.n, p.K, p.zero, i0, j0, smem);
    const float ceps = p.ceps, gam = p.gam;
    dist_store_rows<0>(smem, p.nrm, p.n, i0, j0, p.out, p.rowoff, 0, [=](float ni, float nj, float c) {
        const float ns = ni + nj;
        const float T = 0.5f * ns - c;
        // (T - E_ab)(1 - g'), pushed DOWN by 4 u against the three roundings of this expression itself
        // (ceps is E_ab's constant rounded UP on the host, so the computed product is no smaller than E_ab)
        float L = (T - ceps * ns) * (1.0f - gam);
        L = L * (1.0f - 2.4e-7f);
        L = (L > 1e-30f && ns < 1e37f) ? L : 0.0f; // subnormal range / overflowing norms (also NaN): no claim, the entry is evaluated exactly when it matters
        return __uint_as_float(__float_as_uint(L) | 0x80000000u); // sign bit = "lower bound, not a value" (-0.0: bound 0)
    });
}

// (distance.h says what each launcher takes)
size_t icl_dist_colsum_doubles(int d) { return (size_t)(1 + DIST_CS_PARTS) * (size_t)std::max(d, 1); }
int icl_dist_center_launch(icl_ctx *ctx, const float *d_E, int64_t n, int d, int K, double *d_colsum, float *d_Ec, float *d_nrm, hipStream_t strm)
{
    // d_colsum: (1 + DIST_CS_PARTS) x d doubles -- the sums, then the partial sums (icl_dist_colsum_doubles)
    const unsigned ys = (unsigned)std::max<int64_t>(1, std::min<int64_t>(DIST_CS_PARTS, n / 256));
    hipLaunchKernelGGL(dist_colsum_kernel, dim3((unsigned)icl_ceil_div(d, 256), ys), dim3(256), 0, strm, d_E, n, d, d_colsum + d);
    hipLaunchKernelGGL(dist_colsum_join_kernel, dim3((unsigned)icl_ceil_div(d, 256)), dim3(256), 0, strm, d_colsum + d, (int)ys, d, d_colsum);
    hipLaunchKernelGGL(dist_center_kernel, dim3((unsigned)n), dim3(256), 0, strm, d_E, n, d, K, d_colsum, d_Ec, d_nrm);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

int icl_dist_bound_launch(icl_ctx *ctx, const float *d_Ec, const float *d_nrm, const void *d_zero, int64_t n, int K, float ceps, float gam, float *d_out,
                          const int64_t *d_rowoff, int64_t tr_lo, int64_t tr_hi, hipStream_t strm)
{
    if (tr_hi <= tr_lo) return ICL_OK;
    int64_t nblocks;
    ICL_TRY(icl_dist_grid(ctx, tr_lo, tr_hi, &nblocks));
    icl_lds_optin(ctx, (const void *)dist_bound_kernel, (int)dist_lds_bytes());
    dbound_args a{d_Ec, d_nrm, d_zero, d_out, d_rowoff, n, tr_lo, tr_hi, K, ceps, gam};
    const int64_t r_lo = tr_lo * CV_BM, r_hi = std::min<int64_t>(tr_hi * CV_BM, n);
    const double pairs = 0.5 * ((double)r_hi * (double)(r_hi - 1) - (double)r_lo * (double)(r_lo - 1));
    icl_prof_scope ps(ctx, ICL_K_DIST_MFMA, 2.0 * pairs * K, 4.0 * pairs + 4.0 * (double)r_hi * K);
    hipLaunchKernelGGL(dist_bound_kernel, dim3((unsigned)nblocks), dim3(256), dist_lds_bytes(), strm, a);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

extern "C" int icl_distance_mfma_dev(icl_ctx *ctx, const float *d_E, int64_t n, int32_t d, float *d_D, int64_t ld)
{
    if (!ctx || n < 0 || d < 0 || ld < n || (n && (!d_E || !d_D))) return icl_fail(ctx, ICL_ERR_ARG, "icl_distance_mfma_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return icl_dist_mfma_launch(ctx, d_E, n, d, d_D, nullptr, ld);
}

// ------------------------------------------------------------------------------------------------------------
// The SIZED tile (FAST mode from seeds: icl_cluster_seeded_fast, icl_distance_mfma_seeded_dev).  Row i is a cluster of items[i] >= 1 items
// with centroid E[i]; the entry of i > j is WardDistance's scaling (ward_value.h, ward_scale: fl(f32(s_i s_j) / f32(s_i + s_j)) on the real
// item counts) of the squared distance 2 D~(i, j), D~ the entry dist_mfma_kernel stores for the same two rows:
//     V0(i, j) = clamp0( fl( ward_scale(s_i, s_j) * fl(2 * D~(i, j)) ) ).
// The scale is positive, so the clamp commutes with it; with s_i = s_j = 1 the entry is D~(i, j) itself (num / den = 1/2 and the factor 2 are
// exact below 2^127).  Same split operands, GEMM tile and store geometry as dist_mfma_kernel; defined behind every other kernel of the unit.
// ------------------------------------------------------------------------------------------------------------
// D~'s entry, the expression of dist_mfma_kernel's lambda under the unit's own contraction rule (in front of ward_value.h's pragma)
__device__ __forceinline__ float dist_mfma_entry(float ni, float nj, float c)
{
    const float v = 0.5f * (ni + nj) - c;
    return v > 0.0f ? v : (v == v ? 0.0f : v);
}
#include "ward_value.h"

struct dist_sized_args {
    dist_args g;          // operands, norms, output and its layout: dist_mfma_kernel's
    const int32_t *items; // [n] item counts, >= 1
};

// dist_store_rows with the two rows' item counts beside their norms (MODE: as there)
template <int MODE>
__device__ __forceinline__ void dist_store_rows_sized(const unsigned char *smem, const float *nrm, const int32_t *items, int64_t n, int64_t i0, int64_t j0,
                                                      float *out, const int64_t *rowoff, int64_t ld)
{
    const float *ep = reinterpret_cast<const float *>(smem);
    const int tid = threadIdx.x, nl = (tid & 31) * 4;
    float nj[4];
    int sj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool in = (j0 + nl + q) < n;
        nj[q] = in ? nrm[j0 + nl + q] : 0.0f;
        sj[q] = in ? items[j0 + nl + q] : 1;
    }
    for (int ml = tid >> 5; ml < CV_BM; ml += 8) {
        const int64_t i = i0 + ml;
        if (i >= n) break;
        const float ni = nrm[i];
        const int si = items[i];
        const float4 t = *reinterpret_cast<const float4 *>(ep + ml * DG_EP_LD + nl);
        const float c[4] = {t.x, t.y, t.z, t.w};
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float w = ward_scale(2.0f * dist_mfma_entry(ni, nj[q], c[q]), si, sj[q]);
            v[q] = w > 0.0f ? w : (w == w ? 0.0f : w);
        }
        const int64_t jb = j0 + nl;
        const int64_t lim = MODE == 0 ? i : i + 1; // columns j < lim are written
        float *row = MODE == 0 ? out + rowoff[i] : out + i * ld;
        if (jb + 3 < i && ((MODE == 0) || ((ld & 3) == 0))) { // strictly below the diagonal: one 16-byte store
            *reinterpret_cast<float4 *>(row + jb) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (jb + q < lim) row[jb + q] = (MODE == 1 && jb + q == i) ? 0.0f : v[q];
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void dist_mfma_sized_kernel(const dist_sized_args p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int ti, tj;
    tri_decode32(blockIdx.x, ti, tj);
    const int64_t i0 = (int64_t)ti * CV_BM, j0 = (int64_t)tj * DG_BN;
    dist_gemm_tile<BF16>(p.g.A, p.g.B, p.g.n, p.g.K, p.g.zero, i0, j0, smem);
    dist_store_rows_sized<MODE>(smem, p.g.norms, p.items, p.g.n, i0, j0, p.g.out, p.g.rowoff, p.g.ld);
}

static void dist_sized_enqueue(icl_ctx *ctx, const dist_args &a, const int32_t *d_items, unsigned nblocks)
{
    icl_lds_optin(ctx, (const void *)dist_mfma_sized_kernel<0>, (int)dist_lds_bytes());
    icl_lds_optin(ctx, (const void *)dist_mfma_sized_kernel<1>, (int)dist_lds_bytes());
    const dist_sized_args s{a, d_items};
    if (a.rowoff)
        hipLaunchKernelGGL(dist_mfma_sized_kernel<0>, dim3(nblocks), dim3(256), dist_lds_bytes(), ctx->stream, s);
    else
        hipLaunchKernelGGL(dist_mfma_sized_kernel<1>, dim3(nblocks), dim3(256), dist_lds_bytes(), ctx->stream, s);
}

extern "C" int icl_distance_mfma_seeded_dev(icl_ctx *ctx, const float *d_C, int64_t m, int32_t d, const int32_t *seed_size, float *d_D, int64_t ld)
{
    if (!ctx || m < 0 || d < 0 || ld < m || (m && (!d_C || !d_D || !seed_size))) return icl_fail(ctx, ICL_ERR_ARG, "icl_distance_mfma_seeded_dev: bad argument");
    std::vector<int32_t> items((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t s = seed_size[i] < 0 ? -(int64_t)seed_size[i] : seed_size[i];
        if (s < 1 || s >= ((int64_t)1 << 30)) // (two counts must add up inside an int: ward_scale)
            return icl_fail(ctx, ICL_ERR_ARG, "icl_distance_mfma_seeded_dev: seed_size[%lld] is %d", (long long)i, seed_size[i]);
        items[(size_t)i] = (int32_t)s;
    }
    if (!m) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    dev_guard g_items;
    ICL_TRY(icl_dev_upload(ctx, g_items, items.data(), (size_t)m * 4, "icl_distance_mfma_seeded_dev: item counts"));
    return icl_dist_mfma_sized_launch(ctx, d_C, m, d, g_items.as<int32_t>(), d_D, nullptr, ld); // (synchronised: items may go)
}
