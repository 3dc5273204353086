// distance_i8.hip -- distance BOUNDS of ComputeInitialDistanceMatrix (/root/reference/internal/clustering/clustering.go:61-73) from an INTEGER
// GEMM on the matrix cores (round 5).  Same contract as dist_bound_kernel (distance_mfma.hip, "Distance BOUNDS for the exact mode"): the
// initial matrix is filled with PROVEN lower bounds of the reference's values (sign bit set), the row scans evaluate an entry exactly -- the
// reference's own sequential fp32 expression -- only where a bound reaches a row's minimum, nothing a comparison sees is ever a bound.
//
// Why integers.  The f32 matrix-core form (v_mfma_f32_32x32x2_f32) is an fmaf chain with a textbook error bound, but it runs at 1/16 of the
// bf16 rate: 153 ms of the 100 000-image step at 85 % of ITS peak.  The bf16 forms are 16x faster, but their internal accumulation is
// unspecified, so nothing can be proven about their rounding.  v_mfma_i32_16x16x64_i8 has no rounding at all: 8-bit products, 32-bit sums,
// exact by the ISA's definition whatever the order inside the instruction -- and it runs at twice the bf16 rate.  So the dot product is taken
// on a FIXED-POINT image of the centred rows, and every error of the bound is one this file introduces itself and can account for:
//
//   a' = fl(a - mu) (dist_center_kernel, as before).  Row a gets the scale s_a = 2^e_a with max_k |a'_k| < 2^e_a and the 21-bit integers
//       A_k = rint(a'_k 2^(20 - e_a)),  |A_k| <= 2^20,  |a'_k - s_a 2^-20 A_k| <= s_a 2^-21                 (exact in double; zero row: A = 0)
//   in three balanced base-128 digits  A = q1 2^14 + q2 2^7 + q3,  q2, q3 in [-64, 63], |q1| <= 64  (int8).  With S_st = sum_k q_s^a q_t^b:
//       sum_k A_k B_k = 2^28 S11 + 2^21 (S12 + S21) + 2^14 (S13 + S31 + S22) + 2^7 (S23 + S32) + S33
//   The kernel computes the first three classes EXACTLY: one int8 GEMM over the concatenated K axis
//       P_a = [q1 | q1 | q2 | q1 | q3 | q2],   Q_b = [q1 | q2 | q1 | q3 | q1 | q2]           (6 D bytes of K)
//   -- both read out of ONE digit array [q1 | q2 | q3] per row (3 D bytes: a K-tile's staging offset picks the digit) -- whose 32-bit accumulator is multiplied by 128 after the first D bytes -- hi = 128 S11 + (S12 + S21) <= 2^30 + 2^24 for D <= 2048 -- parked
//   in the output tile itself after 3 D bytes, and restarted for lo = S13 + S31 + S22 <= 3 * 2^23; the epilogue forms I = 128 hi + lo in
//   double (exact: < 2^38) and c = 2^(e_a + e_b - 26) I (a power-of-two scaling: exact).  Then, with L1_a >= sum_k |a'_k|,
//       | a'.b' - c | <= 2^-21 ( s_a (L1_b + D s_b 2^-21) + s_b L1_a )        (the two roundings to 21 bits, first and second order)
//                       + s_a s_b 2^-40 D (2^20 + 2^12)                        (the classes left out: |q| <= 64)              =: m_ab
//   and the rest of the bound is distance_mfma.hip's: T = (n_a + n_b) / 2 - c in double,
//       | T - S/2 | <= E_ab := m_ab + 16 u (1 + 64 u)(n_a + n_b)      (computed norms, centring, the conversions; u = 2^-24)
//       stored  L = max(0, (T - E_ab)(1 - g')) rounded toward zero, sign bit set;   scan side  U(L) = (L (1 + 3 g') + 2 E_ab)(1 + 2 g') >= R
//   The epilogue evaluates E_ab in separable form (dist_i8_bound.h): s_a (2^-21 L1_b) + s_b (2^-21 L1_a) + s_a s_b C_D + kappa n_a + kappa n_b with
//   C_D = D 2^-42 + D (2^20 + 2^12) 2^-40 and kappa = 16 u (1 + 64 u) -- the same real number term by term; the scalings by s and 2^-21 and C_D
//   itself are exact in double, kappa n and the sums round at most six times, all terms are non-negative, so the computed value is within
//   7 * 2^-53 relative of E_ab and the factor (1 + 1e-12) it is multiplied with keeps it an upper bound, as it did for the nested form.
//   (ward.hip wupper recomputes E_ab from the rows' s, L1 and n).  For unit-variance Gaussian rows at D = 2048, E_ab ~ 0.03 against 0.25 for
//   the fmaf-chain bound (whose worst case grows with D u): the integer bound is the TIGHTER one as well as the faster one.
//
// Main loop: the 256 x 256 x (128 bytes) 8-phase loop of conv_p8.h / scratch/gemm8p_bench.hip unchanged -- LDS-DMA kept in flight across raw
// barriers, counted vmcnt, staggered wave groups; the int8 instruction takes the same 16 bytes per lane as the bf16 one, and a dot product does
// not care in which order an instruction walks K as long as both operands are staged alike.  Lower-triangle tiles only.
#include "icl_common.h"
#include "distance.h"
#include "dist_i8_bound.h"
#include "mfma_tile.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

typedef int di8_i32x4 __attribute__((ext_vector_type(4)));

#define DI8_OOB 0x80000000u
#define DI8_SLOT 16384
#define DI8_BUF 65536
#define DI8_WA 0
#define DI8_XA 1
#define DI8_WB 2
#define DI8_XB 3

__device__ __forceinline__ di8_i32x4 di8_srd(const void *base, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)base;
    di8_i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)a); // (wave-uniform by construction; the tile decode runs on the vector ALU)
    r.y = __builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    r.z = __builtin_amdgcn_readfirstlane((int)bytes);
    r.w = 0x00020000;
    return r;
}
// two LDS-DMA pieces (64 lanes x 16 B -> 1 KiB each) of one half-tile (conv_p8.h p8_dma: one scalar per LDS destination, M0 restored)
__device__ __forceinline__ void di8_dma2(const di8_i32x4 &srd, unsigned voff0, unsigned voff1, unsigned soff, unsigned lds0)
{
    unsigned keep;
    const unsigned lds1 = lds0 + 0x2000u;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %5\n\t"
                 "s_nop 4\n\t"
                 "buffer_load_dwordx4 %1, %3, %4 offen lds\n\t"
                 "s_mov_b32 m0, %6\n\t"
                 "s_nop 0\n\t"
                 "buffer_load_dwordx4 %2, %3, %4 offen lds\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff0), "v"(voff1), "s"(srd), "s"(soff), "s"(lds0), "s"(lds1)
                 : "memory");
}
__device__ __forceinline__ di8_i32x4 di8_mfma(const uint4 &a, const uint4 &b, const di8_i32x4 &c)
{
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(di8_i32x4, a), __builtin_bit_cast(di8_i32x4, b), c, 0, 0, 0);
}

// ---- fixed-point image of the centred rows ------------------------------------------------------------------------------------
// Ec [n][K] (K = D rounded up to 32, zero beyond D) -> Q [n][3 Kp] int8 = [q1 | q2 | q3] (Kp = D rounded up to 256), ex[n] (e_a; INT_MIN: the row is all
// zeros or not finite -- its digits are zero and s_a counts as 0), l1[n] >= sum_k |a'_k|.
__global__ __launch_bounds__(256) void dist_quant_kernel(const float *__restrict__ Ec, int64_t n, int K, int Kp, int8_t *__restrict__ Q,
                                                        int32_t *__restrict__ ex, float *__restrict__ l1)
{
    __shared__ float red[2][4];
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const float *row = Ec + r * K;
    float mx = 0.0f, sum = 0.0f;
    bool bad = false;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float a = fabsf(row[k]);
        bad |= !(a < 3.0e38f); // inf / NaN
        mx = fmaxf(mx, a);
        sum += a;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        sum += __shfl_down(sum, off, 64);
    }
    const bool anybad = __syncthreads_or(bad ? 1 : 0) != 0;
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = mx;
        red[1][threadIdx.x >> 6] = sum;
    }
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    sum = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    int e = 0;
    const bool zero = anybad || !(mx > 0.0f);
    if (!zero) (void)frexpf(mx, &e); // mx = f 2^e, f in [0.5, 1): every |a'_k| < 2^e
    if (threadIdx.x == 0) {
        ex[r] = zero ? INT32_MIN : e;
        // any summation order of K non-negative terms: computed >= exact (1 - K u)  =>  exact <= computed (1 + 2 K u)
        l1[r] = zero ? 0.0f : sum * (1.0f + 2.0f * (float)K * 5.9604645e-8f) * 1.000001f;
    }
    int8_t *q = Q + r * 3 * (int64_t)Kp;
    for (int k = threadIdx.x; k < Kp; k += 256) {
        int q1 = 0, q2 = 0, q3 = 0;
        if (!zero && k < K) {
            const int A = (int)rint(ldexp((double)row[k], 20 - e)); // exact scaling, |.| < 2^20: the rounding to an integer is the only error
            q3 = ((A + 64) & 127) - 64;
            const int A1 = (A - q3) >> 7; // exact: A - q3 is a multiple of 128
            q2 = ((A1 + 64) & 127) - 64;
            q1 = (A1 - q2) >> 7;
        }
        q[k] = (int8_t)q1;
        q[Kp + k] = (int8_t)q2;
        q[2 * Kp + k] = (int8_t)q3;
    }
}

struct di8_args {
    const int8_t *Q; // [n][3 Kp]: the digit strings q1 | q2 | q3 of every row
    const float *nrm, *l1;
    const int32_t *ex;
    float *out;
    const int64_t *rowoff;
    int64_t n;
    int T;      // tile rows (256 pairs each)
    int Kp, d;  // bytes per product; the embedding dimension D of the bound's constants
    float gam;  // g'
    unsigned int *rowub; // [n] (may be null) per row i: the smallest UPPER bound U(L) over its pairs j < i, as float bits (atomicMin): the threshold the
                         // initial row minima start from -- their first pass over the row is this epilogue (one pass instead of two)
};

__global__ __launch_bounds__(512) void dist_bound_i8_kernel(const di8_args p)
{
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * DI8_BUF];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 2, wc = wid & 3;
    int ti, tj;
    // tile order: dist_tile.h, over all tile rows -- the workgroups an XCD runs at the same time share their operand blocks in its L2
    tri_band_decode(xcd_remap((int)blockIdx.x, (int)gridDim.x), 0, p.T, ti, tj);
    ti = __builtin_amdgcn_readfirstlane(ti);
    tj = __builtin_amdgcn_readfirstlane(tj);
    const int64_t m0 = (int64_t)ti * 256, n0 = (int64_t)tj * 256; // X rows = output rows i (P strings), W rows = output columns j (Q strings)
    const unsigned rowb = 3u * (unsigned)p.Kp;
    // one buffer descriptor per operand block (256 rows x 3 Kp bytes <= 1.5 MB): the byte offsets stay small whatever n is
    const int64_t xrows = p.n - m0 < 256 ? p.n - m0 : 256, wrows = p.n - n0 < 256 ? p.n - n0 : 256;
    const di8_i32x4 asrd = di8_srd(p.Q + m0 * (int64_t)rowb, (unsigned)xrows * rowb), bsrd = di8_srd(p.Q + n0 * (int64_t)rowb, (unsigned)wrows * rowb);
    unsigned vx[2][2], vw[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int sr = (j * 8 + wid) * 8 + (lane >> 3);
        const int ls = (lane & 7) ^ ((sr >> 1) & 7);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int xr = (sr >> 6) * 128 + h * 64 + (sr & 63);   // X slot row sr = wr * 64 + r: tile row wr * 128 + h * 64 + r
            const int wrow = (sr >> 5) * 64 + h * 32 + (sr & 31);  // W slot row sr = wc * 32 + r: tile row wc * 64 + h * 32 + r
            vx[h][j] = xr < xrows ? (unsigned)xr * rowb + ls * 16u : DI8_OOB;
            vw[h][j] = wrow < wrows ? (unsigned)wrow * rowb + ls * 16u : DI8_OOB;
        }
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + wid * 1024);
    const int l15 = lane & 15, q = lane >> 4, f = (l15 >> 1) & 7;
    const unsigned char *xrd[2], *wrd[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ph = ((4 * s + q) ^ f) << 4;
        xrd[s] = smem + (wr * 64 + l15) * 128 + ph;
        wrd[s] = smem + (wc * 32 + l15) * 128 + ph;
    }
    di8_i32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = di8_i32x4{0, 0, 0, 0};

    const int nt = 6 * p.Kp / 128, b1 = p.Kp / 128, b2 = 3 * p.Kp / 128; // K-tiles; class boundaries (even: Kp % 256 == 0)
    // K-tile t lies in digit product pr = t / b1 of the six: X (rows i) takes digit {1,1,2,1,3,2}[pr], W (columns j) digit {1,2,1,3,1,2}[pr]
    auto stage = [&](int slot, int buf, int t) {
        const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + buf * DI8_BUF + slot * DI8_SLOT);
        const int pr = (t >= b1) + (t >= 2 * b1) + (t >= 3 * b1) + (t >= 4 * b1) + (t >= 5 * b1);
        const bool isx = slot == DI8_XA || slot == DI8_XB;
        const unsigned dig = ((isx ? 0x120100u : 0x102010u) >> (4 * pr)) & 15u;
        const unsigned soff = __builtin_amdgcn_readfirstlane(dig * (unsigned)p.Kp + (unsigned)(t - pr * b1) * 128u);
        if (slot == DI8_WA) di8_dma2(bsrd, vw[0][0], vw[0][1], soff, dst);
        else if (slot == DI8_WB) di8_dma2(bsrd, vw[1][0], vw[1][1], soff, dst);
        else if (slot == DI8_XA) di8_dma2(asrd, vx[0][0], vx[0][1], soff, dst);
        else di8_dma2(asrd, vx[1][0], vx[1][1], soff, dst);
    };
    uint4 xf[4][2], w0[2][2], w1[2][2];
    auto mma = [&](int hx, int hw, uint4 (&wf)[2][2]) {
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[hx * 4 + m][hw * 2 + n] = di8_mfma(wf[n][s], xf[m][s], acc[hx * 4 + m][hw * 2 + n]);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
    };
    auto ktile = [&](auto bufc, auto modec, int t) {
        constexpr int BUF = decltype(bufc)::value, MODE = decltype(modec)::value;
        const size_t bo = (size_t)BUF * DI8_BUF;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int s = 0; s < 2; ++s) w0[n][s] = *reinterpret_cast<const uint4 *>(wrd[s] + bo + DI8_WA * DI8_SLOT + n * 2048);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[m][s] = *reinterpret_cast<const uint4 *>(xrd[s] + bo + DI8_XA * DI8_SLOT + m * 2048);
        if (MODE <= 1) stage(DI8_XB, BUF ^ 1, t + 1);
        asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
        mma(0, 0, w0);
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int s = 0; s < 2; ++s) w1[n][s] = *reinterpret_cast<const uint4 *>(wrd[s] + bo + DI8_WB * DI8_SLOT + n * 2048);
        if (MODE == 0) stage(DI8_WA, BUF, t + 2);
        mma(0, 1, w1);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[m][s] = *reinterpret_cast<const uint4 *>(xrd[s] + bo + DI8_XB * DI8_SLOT + m * 2048);
        if (MODE == 0) stage(DI8_XA, BUF, t + 2);
        mma(1, 1, w1);
        if (MODE == 0) {
            stage(DI8_WB, BUF, t + 2);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else if (MODE == 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        mma(1, 0, w0);
    };
    // where this lane's accumulators live in the output: acc[mt][ntl][e] = pair (row i, column j + e)
    auto out_ptr = [&](int mt, int ntl, int64_t &i, int64_t &j) -> float * {
        i = m0 + wr * 128 + (mt >> 2) * 64 + (mt & 3) * 16 + l15;
        j = n0 + wc * 64 + (ntl >> 1) * 32 + (ntl & 1) * 16 + 4 * q;
        return i < p.n ? p.out + p.rowoff[i] + j : nullptr;
    };
    stage(DI8_WA, 0, 0);
    stage(DI8_XA, 0, 0);
    stage(DI8_WB, 0, 0);
    stage(DI8_XB, 0, 0);
    stage(DI8_WA, 1, 1);
    stage(DI8_XA, 1, 1);
    stage(DI8_WB, 1, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();
    int t = 0;
    for (; t + 4 <= nt; t += 2) {
        if (t == b1) { // S11 complete: hi = 128 S11 + (S12 + S21) from here on
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = acc[i][j] * 128;
        }
        if (t == b2) {
            // hi complete: parked in the output tile (this lane reads its own words back in the epilogue), the accumulator restarts for lo.
            // The stores share the VM counter with the LDS-DMA in flight, and loads and stores may retire out of order with respect to each
            // other, so the counted waits of the loop would no longer mean what they say: drain everything once (one bubble per tile).
#pragma unroll
            for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                for (int ntl = 0; ntl < 4; ++ntl) {
                    int64_t i, j;
                    float *o = out_ptr(mt, ntl, i, j);
                    if (o && j < i) { // (j is a multiple of 4 and so is the row's 16-byte alignment: a straddling group is stored whole inside the pitch)
                        *reinterpret_cast<di8_i32x4 *>(o) = acc[mt][ntl];
                    }
                    acc[mt][ntl] = di8_i32x4{0, 0, 0, 0};
                }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        ktile(std::integral_constant<int, 0>(), std::integral_constant<int, 0>(), t);
        ktile(std::integral_constant<int, 1>(), std::integral_constant<int, 0>(), t + 1);
    }
    ktile(std::integral_constant<int, 0>(), std::integral_constant<int, 1>(), t);
    ktile(std::integral_constant<int, 1>(), std::integral_constant<int, 2>(), t + 1);
    if (wr == 0) __builtin_amdgcn_s_barrier();
    // ---- epilogue: I = 128 hi + lo (exact in double), T, E_ab, the flagged bound (dist_i8_bound.h).
    // INTERIOR: the tile lies strictly below the diagonal and inside n (all but the diagonal tiles and the last, ragged tile row: 782 of 76 636
    // tiles at n = 100 000) -- every row i < n, every column j + e < i: no predicate on any element, float4 stores only.  The other tiles keep
    // the predicates.  Either way a lane forms the pointers of its 8 rows once, the column constants once per column group, and requests the
    // parked hi words and the row constants of four row groups together (they do not depend on one another): eight round trips per tile and
    // one for the row offsets, where each of the 32 (row group, column group) pairs used to wait for two in turn.
    // The asm statements are fences for the compiler only (no instruction): without them it schedules the whole tile's arithmetic as one block,
    // converts a column group's integers up front, defers the upper bounds to the end, and spills hundreds of registers.
    const double cd = di8_cd(p.d), gam = (double)p.gam;
    auto epilogue = [&](auto interiorc) {
        constexpr bool INTERIOR = decltype(interiorc)::value;
        float *rptr[8];
        float um[8]; // smallest upper bound of this lane's entries in row (mt, l15)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int64_t i = m0 + wr * 128 + (mt >> 2) * 64 + (mt & 3) * 16 + l15;
            rptr[mt] = (INTERIOR || i < p.n) ? p.out + p.rowoff[i] : nullptr;
            um[mt] = ICL_MAXF;
        }
#pragma unroll
        for (int ntl = 0; ntl < 4; ++ntl) {
            const int64_t j = n0 + wc * 64 + (ntl >> 1) * 32 + (ntl & 1) * 16 + 4 * q;
            di8_side cb[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = INTERIOR || j + e < p.n;
                cb[e] = di8_side_of(in ? p.ex[j + e] : DI8B_NOEXP, in ? p.l1[j + e] : 0.0f, in ? p.nrm[j + e] : 0.0f);
            }
#pragma unroll
            for (int hx = 0; hx < 2; ++hx) {
                di8_i32x4 hi[4]; // this lane's own words, parked at K-tile b2
                int rex[4];
                float rl1[4], rnr[4];
                asm volatile("" ::: "memory");
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int64_t i = m0 + wr * 128 + hx * 64 + m * 16 + l15;
                    const bool live = INTERIOR || (i < p.n && j < i);
                    hi[m] = live ? *reinterpret_cast<const di8_i32x4 *>(rptr[hx * 4 + m] + j) : di8_i32x4{0, 0, 0, 0};
                    rex[m] = live ? p.ex[i] : DI8B_NOEXP;
                    rl1[m] = live ? p.l1[i] : 0.0f;
                    rnr[m] = live ? p.nrm[i] : 0.0f;
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int mt = hx * 4 + m;
                    const int64_t i = m0 + wr * 128 + hx * 64 + m * 16 + l15;
                    if (!INTERIOR && (i >= p.n || j >= i)) continue;
                    di8_i32x4 lo = acc[mt][ntl], hw = hi[m];
                    asm volatile("" : "+v"(rex[m]), "+v"(rl1[m]), "+v"(rnr[m]), "+v"(lo), "+v"(hw)::"memory");
                    const di8_side ra = di8_side_of(rex[m], rl1[m], rnr[m]);
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double I = 128.0 * (double)hw[e] + (double)lo[e];
                        const double Eab = di8_eab(ra, cb[e], cd);
                        const float L = di8_lower(di8_T(ra, cb[e], I), Eab, ra.n + cb[e].n, gam);
                        v[e] = __uint_as_float(__float_as_uint(L) | 0x80000000u);
                        if (INTERIOR || j + e < i) um[mt] = fminf(um[mt], di8_upper(L, Eab, gam));
                    }
                    asm volatile("" : "+v"(um[mt]));
                    if (INTERIOR || j + 3 < i) {
                        *reinterpret_cast<float4 *>(rptr[mt] + j) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (j + e < i) rptr[mt][j + e] = v[e];
                    }
                    // (complete rows, ward.hip: writing the second copy of the pair from here -- row j + e at column i, 64 contiguous bytes per quarter
                    // wave and store -- cost this kernel 12 ms at n = 100 000; ward_symmetrize_kernel's tile transposes take 7.8 ms for the same bytes)
                }
            }
        }
        if (p.rowub) { // the four quarter waves of a wave hold the same 16 rows: join them, one atomic per row and wave
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                um[mt] = fminf(um[mt], __shfl_xor(um[mt], 16, 64));
                um[mt] = fminf(um[mt], __shfl_xor(um[mt], 32, 64));
            }
            if (q == 0) {
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    const int64_t i = m0 + wr * 128 + (mt >> 2) * 64 + (mt & 3) * 16 + l15;
                    // (upper bounds are >= +0: their bits order like the values; INTERIOR: every row has entries, and ICL_MAXF would change nothing)
                    if (INTERIOR || (i < p.n && um[mt] < ICL_MAXF)) atomicMin(&p.rowub[i], __float_as_uint(um[mt]));
                }
            }
        }
    };
    if (tj < ti && m0 + 256 <= p.n) epilogue(std::true_type());
    else epilogue(std::false_type());
}

// Usable for this shape?  D <= 2048 keeps hi = 128 S11 + S12 + S21 inside 32 bits.
bool icl_dist_i8_usable(int64_t n, int d) { return d >= 1 && d <= 2048 && n < (1LL << 29); }
size_t icl_dist_i8_pq_bytes(int64_t n, int d)
{
    const int64_t Kp = (d + 255) / 256 * 256;
    return (size_t)(n * 3 * Kp) + 256;
}

// (distance.h says what each argument is)
int icl_dist_bound_i8_launch(icl_ctx *ctx, const float *d_Ec, const float *d_nrm, int64_t n, int d, int K, float gam, void *d_pq, float *d_l1, int32_t *d_ex,
                             float *d_out, const int64_t *d_rowoff, hipStream_t strm, unsigned int *d_rowub)
{
    const int Kp = (d + 255) / 256 * 256;
    int8_t *Q = reinterpret_cast<int8_t *>(d_pq);
    if (n <= 0) return ICL_OK;
    hipLaunchKernelGGL(dist_quant_kernel, dim3((unsigned)n), dim3(256), 0, strm, d_Ec, n, K, Kp, Q, d_ex, d_l1);
    const int64_t T = icl_ceil_div(n, 256);
    int64_t nblocks;
    ICL_TRY(icl_dist_grid(ctx, 0, T, &nblocks));
    if (d_rowub) ICL_HIP(ctx, hipMemsetAsync(d_rowub, 0x7f, (size_t)n * sizeof(unsigned int), strm)); // 0x7f7f7f7f = 3.39e38: "nothing known"
    di8_args a{Q, d_nrm, d_l1, d_ex, d_out, d_rowoff, n, (int)T, Kp, d, gam, d_rowub};
    const double pairs = 0.5 * (double)n * (double)(n - 1);
    icl_prof_scope ps(ctx, ICL_K_DIST_MFMA, 2.0 * pairs * 6.0 * Kp, 4.0 * pairs + (double)n * 3.0 * Kp);
    hipLaunchKernelGGL(dist_bound_i8_kernel, dim3((unsigned)nblocks), dim3(512), 0, strm, a);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}
