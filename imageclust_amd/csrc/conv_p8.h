// conv_p8.h -- the deep-pipelined implicit-GEMM convolution of the K-heavy ResNet50 layers (bf16; included by resnet.hip).
//
// Replaces, for those layers, the 128 x 128 / two-stage / barrier-per-k-step loop of conv_igemm_kernel and conv3x3_halo_kernel, whose
// ceiling is ~810 TFLOP/s on a plain GEMM, inside the forward pass that stands for OpenCV-DNN's Net.Forward
// (/root/reference/internal/embeddings/embeddings.go:141).  Proven first on a plain GEMM (scratch/gemm8p_bench.hip: 1 258 TFLOP/s
// at 4096^3 on random data).
//
//   tile      256 output pixels x 256 output channels (Cout % 256 == 0) or 512 pixels x 128 channels (Cout = 128) x 64 k per K-tile;
//             512 threads = 8 waves as MW (pixels) x NWV (channels) = 2 x 4 or 4 x 2; wave tile 128 pixels x 64 channels = 8 x 4
//             accumulators of v_mfma_f32_16x16x32_bf16, weights as the A operand (each lane ends up with 4 consecutive channels of one pixel)
//   LDS       ONE array: 2 K-tile buffers x 4 half-tile slots (WA, XA, WB, XB: NWV * 32 weight rows / MW * 64 pixel rows of 128 B,
//             XOR-swizzled on the DMA's source address and again on the fragment read): 2 x 64 KiB or 2 x 80 KiB
//   loads     LDS-DMA through buffer descriptors (out-of-range lanes = the convolution's zero padding / rows beyond M), kept in
//             flight ACROSS raw s_barriers; one counted s_waitcnt vmcnt(6) per K-tile (three half-tiles stay in flight), never 0 in the loop
//   phases    four per K-tile, each {fragment ds_reads + one half-tile of LDS-DMA | s_barrier | 16 MFMAs at s_setprio 1 | s_barrier};
//             waves 4-7 run half a phase behind waves 0-3 (one extra barrier up front): on every SIMD one wave's MFMA segment lies
//             beside its partner's load segment
//   hazards   a half-tile is read one phase after the counted wait that retires it; a slot is restaged two phases after its last
//             ds_read, or one phase after when those reads were retired (lgkmcnt) before the reading phase's first barrier (WA)
//   A operand implicit GEMM: tile row = output pixel (b, oy, ox) linear in M; K-tile t = (tap (kh, kw), 64 input channels); per-lane
//             row offsets + a 9-bit tap validity mask; DUAL: K = [Cin of X | Cin2 of the strided X2] (a bottleneck's downsample branch)
//   epilogue  in registers: pairs of accumulator tiles trade lane rows (v_permlane16_swap) so that a lane holds 8 consecutive channels of
//             one pixel; y = relu(acc * scale + shift (+ residual)) in fp32, one rounding; 16-byte residual loads and stores
#pragma once
#include "conv_select.h"
#include "mfma_tile.h"
#include "resnet_fused.h"

// geometry of a wave layout: MW pixel waves x NWV channel waves (MW * NWV == 8)
template <int MW, int NWV>
struct p8_geom {
    static_assert(MW * NWV == 8 && (NWV == 4 || NWV == 2), "8 waves");
    static constexpr int BM = MW * 128, BN = NWV * 64;
    static constexpr int PX = MW, PW = NWV / 2;             // LDS-DMA pieces (64 rows each) per X / W half-tile slot
    static constexpr int SX = PX * 8192, SW = PW * 8192;    // slot bytes
    static constexpr int O_WA = 0, O_XA = SW, O_WB = SW + SX, O_XB = 2 * SW + SX; // slot order = the order the phases need them
    static constexpr int BUF = 2 * (SW + SX);               // one K-tile buffer: 64 KiB (2 x 4) or 80 KiB (4 x 2)
    static constexpr int LDS = 2 * BUF;
    static constexpr int INFLIGHT = 2 * PW + PX;            // pieces of WA, XA, WB of K-tile t + 2 that stay in flight over the counted wait: 6 either way
    static_assert(INFLIGHT == 6 && LDS <= 160 * 1024, "counted vmcnt(6); the CU's 160 KiB");
};

// NP LDS-DMA pieces (64 lanes x 16 B -> 1 KiB each, 8 KiB apart: the 8 waves' pieces interleave) of one half-tile slot
template <int NP>
__device__ __forceinline__ void p8_dma(const i32x4_t &srd, const unsigned (&voff)[NP], unsigned soff, unsigned lds0)
{
    unsigned keep;
    // (a scalar per destination instead of s_add on m0: s_add would clobber SCC behind hipcc's back)
    if constexpr (NP == 1) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff[0]), "s"(srd), "s"(soff), "s"(lds0)
                     : "memory");
    } else if constexpr (NP == 2) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\t"
                     "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff[0]), "v"(voff[1]), "s"(srd), "s"(soff), "s"(lds0), "s"(lds0 + 0x2000u)
                     : "memory");
    } else {
        static_assert(NP == 4, "1, 2 or 4 pieces");
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %7\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %5, %6 offen lds\n\t"
                     "s_mov_b32 m0, %8\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %5, %6 offen lds\n\t"
                     "s_mov_b32 m0, %9\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %5, %6 offen lds\n\t"
                     "s_mov_b32 m0, %10\n\ts_nop 0\n\tbuffer_load_dwordx4 %4, %5, %6 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "s"(srd), "s"(soff), "s"(lds0), "s"(lds0 + 0x2000u), "s"(lds0 + 0x4000u),
                       "s"(lds0 + 0x6000u)
                     : "memory");
    }
}

// SPLIT (the 7 x 7 layers: 98 tiles of 256 x 256 per batch of 256 on 256 CUs): every tile is computed by TWO workgroups, each over half of the
// K-tiles.  The workgroups [0, tiles) take the second half, write their raw fp32 sums (in the accumulator layout: 16 B per lane, coalesced)
// and raise the tile's flag; the workgroups [tiles, 2 tiles) take the first half, wait for the flag, form own + partner -- one fixed order,
// so the result does not depend on timing or on the batch -- and run the epilogue.  The writers have the lower block indices, i.e. all of them
// are dispatched before any waiter: a waiter never holds a CU its writer needs.
// X3 (ICL_PREC_BF16X3): operands in the split bf16 layout (mfma_tile.h, BF16X3; the caller passes Cin, Cin2 and K in bf16 elements, i.e.
// doubled), so the staging is the bf16 kernel's; fragment slot s = 0 is hi and s = 1 is lo of the same 32 k, the MFMA segment issues
// wh.xh, wl.xh, wh.xl (24 MFMAs instead of 16, same fragments, same barriers: the LDS hazards above are unchanged), the epilogue writes hi / lo.
template <int MW, int NWV, bool TAPS, bool DUAL, bool SPLIT = false, bool X3 = false>
__global__ __launch_bounds__(512) void conv_p8_kernel(const conv_args p)
{
    static_assert(!(SPLIT && DUAL), "the split form covers single-operand layers");
    static_assert(!(SPLIT && X3), "the split form is bf16 only");
    typedef p8_geom<MW, NWV> G;
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
    constexpr int PX = G::PX, PW = G::PW;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[G::LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid / NWV, wc = wid % NWV;
    const int grp = wid >> 2; // waves 4-7 run half a phase behind waves 0-3 (SIMD partners: MI355X_MICROARCH.md "Two waves per SIMD", item 9)
    const int ntile = p.gx * p.gy;
    const int role = SPLIT ? (int)blockIdx.x / ntile : 0; // SPLIT: 0 = second half of K, sums written out; 1 = first half + the partner's sums + epilogue
    const int tile = xcd_remap((int)blockIdx.x - role * ntile, ntile);
    const int m0 = (tile / p.gy) * G::BM, n0 = (tile % p.gy) * G::BN;
    const i32x4_t xsrd = bn56_srd(p.X, (unsigned)((size_t)p.B * p.H * p.W * p.Cin * 2));
    const i32x4_t wsrd = bn56_srd(p.Wt, (unsigned)((size_t)p.Cout * p.K * 2));
    const i32x4_t x2srd = DUAL ? bn56_srd(p.X2, (unsigned)((size_t)p.B * p.H2 * p.W2 * p.Cin2 * 2)) : xsrd;

    // ---- LDS-DMA roles: piece j of a slot covers slot rows (j * 8 + wid) * 8 + (lane >> 3), physical 16-byte chunk lane & 7
    // vmask[j] (TAPS): the 9-bit tap validity masks of piece j's two rows, half h in bits 16 h .. 16 h + 8 (one register for both halves)
    unsigned vx[2][PX], vw[2][PW], vx2[DUAL ? 2 : 1][PX], vmask[PX];
    // The weight offsets need no division: they are formed first, and WA(0) is requested before any pixel arithmetic.
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        const int sr = (j * 8 + wid) * 8 + (lane >> 3);
        const unsigned ls16 = (unsigned)(((lane & 7) ^ ((sr >> 1) & 7)) << 4); // source-side swizzle: the logical chunk this physical position holds
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int wrow = n0 + (sr >> 5) * 64 + h * 32 + (sr & 31); // W slot row sr = wc * 32 + r: channel wc * 64 + h * 32 + r
            vw[h][j] = (unsigned)wrow * (unsigned)p.K * 2u + ls16;
        }
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + wid * 1024);
    // X half h: per-lane row offsets and tap masks.  The taps (kh, kw) a row may read form a rectangle: kw is valid iff 0 <= ix0 + kw < W, i.e. for
    // kw in [clamp(-ix0), clamp(W - ix0)) (clamped to [0, KW]), and likewise kh; so the mask -- bit kh * KW + kw set iff ok, iy0 + kh in [0, H) and
    // ix0 + kw in [0, W) -- is the column bits repeated once per kernel row (a multiplication by taprep: the copies do not overlap), cut to the
    // valid kernel rows.  No loop over the taps, any KH * KW <= 9.
    unsigned taprep = 0;
    if (TAPS)
        for (int kh = 0; kh < p.KH; ++kh) taprep |= 1u << (kh * p.KW);
    auto xrows = [&](int h) {
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            const int sr = (j * 8 + wid) * 8 + (lane >> 3);
            const unsigned ls16 = (unsigned)(((lane & 7) ^ ((sr >> 1) & 7)) << 4);
            const int m = m0 + (sr >> 6) * 128 + h * 64 + (sr & 63); // X slot row sr = wr * 64 + r: tile row wr * 128 + h * 64 + r
            const bool ok = (int64_t)m < p.M;
            const unsigned mm = ok ? (unsigned)m : 0u;
            const unsigned tq = mm / (unsigned)p.Wo;
            const int ox = (int)(mm - tq * (unsigned)p.Wo);
            const int b = (int)(tq / (unsigned)p.Ho);
            const int oy = (int)(tq - (unsigned)b * (unsigned)p.Ho);
            const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
            const unsigned off = (unsigned)((((b * p.H + iy0) * p.W + ix0) * p.Cin) * 2) + ls16; // (may wrap for padded taps: only used where the tap is valid)
            if (TAPS) {
                const int c0 = std::min(std::max(-ix0, 0), p.KW), c1 = std::min(std::max(p.W - ix0, 0), p.KW); // c0 <= c1 (W > 0)
                const int r0 = std::min(std::max(-iy0, 0), p.KH), r1 = std::min(std::max(p.H - iy0, 0), p.KH);
                const unsigned cols = ((1u << (c1 - c0)) - 1u) << c0;
                const unsigned rows = ((1u << ((r1 - r0) * p.KW)) - 1u) << (r0 * p.KW);
                const unsigned mk = ok ? (cols * taprep) & rows : 0u;
                vmask[j] = h ? vmask[j] | (mk << 16) : mk;
                vx[h][j] = off;
            } else {
                vx[h][j] = ok ? off : BN56_OOB;
            }
            if (DUAL) vx2[DUAL ? h : 0][j] = ok ? (unsigned)((((b * p.H2 + oy * p.stride2) * p.W2 + ox * p.stride2) * p.Cin2) * 2) + ls16 : BN56_OOB;
        }
    };

    const int nt = SPLIT ? p.K / 128 : p.K / 64;  // K-tiles of this workgroup (SPLIT: half of them; conv_select.h, conv_p8_split_eligible: K % 256 == 0)
    const int kt0 = (SPLIT && role == 0) ? nt : 0; // its first K-tile
    const int nt1 = (p.KH * p.KW * p.Cin) / 64; // K-tiles of the first operand (== nt unless DUAL)
    // running position of the X half-tile being staged (XA(u), XB(u), XA(u + 1), ... in this order): uniform scalars
    int xs_t = kt0, xs_ci = 0, xs_kw = 0, xs_kh = 0;
    unsigned xs_off = 0, xs_bit = 1;
    if (SPLIT && TAPS && kt0) {
        const int cpt = p.Cin / 64, tap = kt0 / cpt; // K-tiles per tap; the tap K-tile kt0 lies in
        xs_ci = (kt0 - tap * cpt) * 64;
        xs_kh = tap / p.KW;
        xs_kw = tap - xs_kh * p.KW;
        xs_bit = 1u << tap;
        xs_off = (unsigned)(((xs_kh * p.W + xs_kw) * p.Cin + xs_ci) * 2);
    }
    auto stage_w = [&](int h, int buf, int t) { // W half h of this workgroup's K-tile t
        p8_dma<PW>(wsrd, vw[h], (unsigned)(kt0 + t) * 128u, lds0 + buf * G::BUF + (h ? G::O_WB : G::O_WA));
    };
    auto stage_x = [&](int h, int buf) { // X half h of K-tile xs_t; after half 1 the position moves on
        const unsigned dst = lds0 + buf * G::BUF + (h ? G::O_XB : G::O_XA);
        if (DUAL && xs_t >= nt1) {
            p8_dma<PX>(x2srd, vx2[DUAL ? h : 0], (unsigned)(xs_t - nt1) * 128u, dst);
        } else if (TAPS) {
            const unsigned bit = h ? xs_bit << 16 : xs_bit;
            unsigned v[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j] = (vmask[j] & bit) ? vx[h][j] + xs_off : BN56_OOB;
            p8_dma<PX>(xsrd, v, 0u, dst);
        } else {
            p8_dma<PX>(xsrd, vx[h], (unsigned)xs_t * 128u, dst);
        }
        if (h == 1) {
            ++xs_t;
            if (TAPS) {
                xs_ci += 64;
                if (xs_ci == p.Cin) {
                    xs_ci = 0;
                    xs_bit <<= 1;
                    if (++xs_kw == p.KW) {
                        xs_kw = 0;
                        ++xs_kh;
                    }
                }
                xs_off = (unsigned)(((xs_kh * p.W + xs_kw) * p.Cin + xs_ci) * 2);
            }
        }
    };
    // prologue: all of K-tile 0, three half-tiles of K-tile 1 (conv_p8_eligible: nt even, >= 2).  The first weight half goes out before any pixel
    // arithmetic, each X half as soon as its offsets exist, the second weight half between them (both weight halves in front of the X halves
    // measured slower: every workgroup of a launch then asks for the same few weight rows at the same moment -- DESIGN.md section 4); the
    // stagings of K-tile 1 stay last and in the loop's order, so that the counted wait below means what it means in the loop: everything but
    // WA(1), XA(1), WB(1) has landed.
    stage_w(0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    xrows(0);
    stage_x(0, 0);
    stage_w(1, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    xrows(1);
    stage_x(1, 0);
    stage_w(0, 1, 1);
    stage_x(0, 1);
    stage_w(1, 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    // ---- fragment roles: lane (q = lane >> 4, l15 = lane & 15) reads row l15 of a 16-row fragment, logical chunk 4 s + q
    const int l15 = lane & 15, q = lane >> 4, fsw = (l15 >> 1) & 7;
    const unsigned char *xrd[2], *wrd[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int ph = ((4 * s + q) ^ fsw) << 4;
        xrd[s] = smem + (wr * 64 + l15) * 128 + ph;
        wrd[s] = smem + (wc * 32 + l15) * 128 + ph;
    }
    f32x4 acc[8][4]; // (zeroed behind the requests, not in front of them)
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the epilogue's folded BN scale / shift of this lane's 2 x 8 channels: requested at the start of the LAST K-tile (ktile, MODE 2), where the
    // staging offsets are dead; SPLIT: behind the partner sums, whose loads need the registers
    float4 sc4[2][2], sh4[2][2];
    auto load_affine = [&]() {
        const int cb = n0 + wc * 64 + (q & 1) * 16 + (q >> 1) * 8; // (cbl of the epilogue)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sc4[i][0] = *reinterpret_cast<const float4 *>(p.scale + cb + i * 32);
            sc4[i][1] = *reinterpret_cast<const float4 *>(p.scale + cb + i * 32 + 4);
            sh4[i][0] = *reinterpret_cast<const float4 *>(p.shift + cb + i * 32);
            sh4[i][1] = *reinterpret_cast<const float4 *>(p.shift + cb + i * 32 + 4);
        }
    };

    uint4 xf[4][2], w0[2][2], w1[2][2];
    auto mma = [&](int hx, int hw, uint4 (&wf)[2][2]) {
        __builtin_amdgcn_s_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_setprio(1);
        if constexpr (X3) { // (w slot, x slot) = (hi, hi), (lo, hi), (hi, lo); 8 independent accumulators between dependent MFMAs
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[hx * 4 + m][hw * 2 + n] = mfma16(wf[n][u == 1], xf[m][u == 2], acc[hx * 4 + m][hw * 2 + n]);
        } else {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 2; ++n) acc[hx * 4 + m][hw * 2 + n] = mfma16(wf[n][s], xf[m][s], acc[hx * 4 + m][hw * 2 + n]);
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_s_barrier();
    };
    // MODE 0: steady state, 1: K-tile nt - 2 (only XB(nt - 1) is still to be staged), 2: K-tile nt - 1
    auto ktile = [&](auto bufc, auto modec, int t) {
        constexpr int BUF = decltype(bufc)::value, MODE = decltype(modec)::value;
        const size_t bo = (size_t)BUF * G::BUF;
        // MODE 2: no LDS-DMA is in flight any more (MODE 1 ended on vmcnt(0)) and none follows, so from here on the VM counter is the compiler's
        // and the 8 scale / shift loads land under the last 64 MFMAs.  Not earlier: in the loop vmcnt(6) must count LDS-DMA pieces only (loads of
        // another kind may retire out of order with respect to them: distance_i8.hip, "hi complete").
        if constexpr (MODE == 2 && !SPLIT && !X3) load_affine();
        // phase 1: W0 (4 reads, retired before the barrier: WA is restaged next phase), X0 (8 reads); stage XB(t + 1)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int s = 0; s < 2; ++s) w0[n][s] = *reinterpret_cast<const uint4 *>(wrd[s] + bo + G::O_WA + n * 2048);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[m][s] = *reinterpret_cast<const uint4 *>(xrd[s] + bo + G::O_XA + m * 2048);
        if (MODE <= 1) stage_x(1, BUF ^ 1);
        asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");
        mma(0, 0, w0);
        // phase 2: W1; stage WA(t + 2)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int s = 0; s < 2; ++s) w1[n][s] = *reinterpret_cast<const uint4 *>(wrd[s] + bo + G::O_WB + n * 2048);
        if (MODE == 0) stage_w(0, BUF, t + 2);
        mma(0, 1, w1);
        // phase 3: X1; stage XA(t + 2)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s) xf[m][s] = *reinterpret_cast<const uint4 *>(xrd[s] + bo + G::O_XB + m * 2048);
        if (MODE == 0) stage_x(0, BUF);
        mma(1, 1, w1);
        // phase 4: no reads (W0 is still in registers); stage WB(t + 2); the ONE counted wait of the K-tile: everything up to
        // XB(t + 1) has landed, the three half-tiles of t + 2 stay in flight.  They are read from the next phase on.
        if (MODE == 0) {
            stage_w(1, BUF, t + 2);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        } else if (MODE == 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        mma(1, 0, w0);
    };
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier(); // the stagger
    int t = 0;
    for (; t + 4 <= nt; t += 2) {
        ktile(std::integral_constant<int, 0>(), std::integral_constant<int, 0>(), t);
        ktile(std::integral_constant<int, 1>(), std::integral_constant<int, 0>(), t + 1);
    }
    ktile(std::integral_constant<int, 0>(), std::integral_constant<int, 1>(), t);
    ktile(std::integral_constant<int, 1>(), std::integral_constant<int, 2>(), t + 1);
    if (grp == 0) __builtin_amdgcn_s_barrier(); // every wave has passed its last fragment read: the staging buffers are free

    if constexpr (SPLIT) {
        // The partner sums: [tile][accumulator 0..31][thread], 16 B per lane (whole lines per wave), handed over the write-through way
        // (MI355X_MICROARCH.md, "Valid forms", first row of the table): every byte stored sc1, every storing wave drains (vmcnt(0)), workgroup barrier,
        // ONE lane raises the tile's flag with an sc1 store; each wave of the partner polls the flag (sc1 load) and then reads every byte with sc1
        // loads.  No L2 write-back and no invalidate: the first version of this hand-off -- plain stores, an agent release in each of the 8 waves,
        // an agent acquire in each reading wave -- cost ~40 us per launch (96 write-backs per XCD) and the embedding 6.5 % with two passes in flight.
        typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
        const __amdgpu_buffer_rsrc_t psrd = __builtin_amdgcn_make_buffer_rsrc(p.sk_part, 0, (int)((size_t)ntile * (32 * 512 * 16)), 0x00020000);
        const int voff = tid * 16;
        const int soff0 = tile * (32 * 512 * 16); // (conv_p8_split_scratch: at most 4 096 tiles, 1 GiB)
        if (role == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[i][j]), psrd, voff, soff0 + (i * 4 + j) * 8192, 16 /* sc1 */);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store(p.sk_flag + tile, p.sk_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        // (bounded: a writer that never arrives -- impossible on a healthy device, see the dispatch order above -- yields a wrong tile, not a hung GPU)
        for (int spin = 0; spin < (1 << 22); ++spin) {
            if (__hip_atomic_load(p.sk_flag + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p.sk_epoch) break;
            __builtin_amdgcn_s_sleep(2);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (orders the compiler's loads behind the poll; no cache operation)
#pragma unroll
        for (int g = 0; g < 4; ++g) { // groups of 8 loads (32 registers: the fragments' are free by now)
            u32x4_t o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = __builtin_amdgcn_raw_buffer_load_b128(psrd, voff, soff0 + (g * 8 + k) * 8192, 16 /* sc1 */);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[(g * 8 + k) >> 2][(g * 8 + k) & 3] += __builtin_bit_cast(f32x4, o[k]); // own (first half of K) + partner (second half): one fixed order
        }
    }

    // ---- epilogue, in registers: two accumulator tiles 16 channels apart trade half their lane rows (v_permlane16_swap), after which
    // a lane holds 8 CONSECUTIVE channels of one pixel -- a 16-byte residual load and a 16-byte store per lane, 16 pixels x 64
    // contiguous bytes per instruction -- and y = relu(acc * scale + shift (+ residual)) is formed in fp32 and rounded once.
    // No LDS, no barrier: the staging buffers are not touched again.
    //   before the swap lane (q, l15) holds channels 16 n + 4 q + j of pixel l15 (j = 0..3) for tiles n = A, B;
    //   after: even q: channels 4 q .. 4 q + 7 of tile A;  odd q: channels 4 (q - 1) .. 4 (q - 1) + 7 of tile B
    if constexpr (SPLIT || X3) load_affine(); // (X3: the 24-MFMA phases leave no room for 32 more registers in the last K-tile)
    typedef uint16_t elem;
    const int cbl = (q & 1) * 16 + (q >> 1) * 8; // this lane's first channel inside a pair of accumulator tiles (32 channels)
    elem *Yg = (elem *)p.Y;
    const elem *Rg = (const elem *)p.R;
    // row stride and (X3) the split layout's position of channel c: hi at c + (c & ~31), lo 32 elements further
    const int64_t yld = X3 ? 2 * (int64_t)p.Cout : (int64_t)p.Cout;
    auto ycol = [&](int c) { return X3 ? c + (c & ~31) : c; };
    float sc[2][8], sh[2][8]; // (requested at the start of the last K-tile)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float4 a0 = sc4[i][0], a1 = sc4[i][1], b0 = sh4[i][0], b1 = sh4[i][1];
        sc[i][0] = a0.x; sc[i][1] = a0.y; sc[i][2] = a0.z; sc[i][3] = a0.w; sc[i][4] = a1.x; sc[i][5] = a1.y; sc[i][6] = a1.z; sc[i][7] = a1.w;
        sh[i][0] = b0.x; sh[i][1] = b0.y; sh[i][2] = b0.z; sh[i][3] = b0.w; sh[i][4] = b1.x; sh[i][5] = b1.y; sh[i][6] = b1.z; sh[i][7] = b1.w;
    }
    // FULL: every row of the tile lies inside M (decided once, wave-uniform) -- no bounds test around any load or store; a ragged tile tests each row
    auto epilogue = [&](auto fullc) {
    constexpr bool FULL = decltype(fullc)::value;
    auto inside = [&](int64_t mrow) { return FULL || mrow < p.M; };
#pragma unroll
    for (int hx = 0; hx < 2; ++hx) {
        uint4 rv[4][2], rl[2];
        if (Rg && !X3) { // the 8 residual chunks of this half are requested before any arithmetic (X3: 4 per pixel row, below -- registers)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int64_t mrow = (int64_t)m0 + wr * 128 + hx * 64 + m * 16 + l15;
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    rv[m][i] = inside(mrow) ? *reinterpret_cast<const uint4 *>(Rg + mrow * p.Cout + n0 + wc * 64 + i * 32 + cbl) : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int64_t mrow = (int64_t)m0 + wr * 128 + hx * 64 + m * 16 + l15;
            if (X3 && Rg) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const elem *r = Rg + mrow * yld + ycol(n0 + wc * 64 + i * 32 + cbl);
                    rv[m][i] = inside(mrow) ? *reinterpret_cast<const uint4 *>(r) : make_uint4(0, 0, 0, 0);
                    rl[i] = inside(mrow) ? *reinterpret_cast<const uint4 *>(r + 32) : make_uint4(0, 0, 0, 0);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const f32x4 ta = acc[hx * 4 + m][2 * i], tb = acc[hx * 4 + m][2 * i + 1];
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(ta[j]), __float_as_uint(tb[j]), false, false);
                    v[j] = __uint_as_float(r[0]);
                    v[4 + j] = __uint_as_float(r[1]);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[i][e] + sh[i][e];
                if (Rg) {
                    const elem *re = reinterpret_cast<const elem *>(&rv[m][i]);
                    if constexpr (X3) {
                        const elem *rle = reinterpret_cast<const elem *>(&rl[i]);
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += BF16::to_f(re[e]) + BF16::to_f(rle[e]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] += BF16::to_f(re[e]);
                    }
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.0f);
                }
                uint4 ov, ol;
                elem *oe = reinterpret_cast<elem *>(&ov);
                if constexpr (X3) {
                    elem *ole = reinterpret_cast<elem *>(&ol);
#pragma unroll
                    for (int e = 0; e < 8; ++e) BF16X3::split(v[e], oe[e], ole[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) oe[e] = BF16::from_f(v[e]);
                }
                elem *yo = Yg + mrow * yld + ycol(n0 + wc * 64 + i * 32 + cbl);
                if (inside(mrow)) {
                    *reinterpret_cast<uint4 *>(yo) = ov;
                    if (X3) *reinterpret_cast<uint4 *>(yo + 32) = ol;
                }
            }
        }
    }
    };
    // (X3 and SPLIT keep the one general path: their epilogues are at the register budget, and a second copy costs them spills)
    if (!X3 && !SPLIT && (int64_t)m0 + G::BM <= p.M) epilogue(std::true_type());
    else epilogue(std::false_type());
}

// the per-stream scratch of the split form: 256 KiB of partner sums + a flag per tile (flags compare against a per-slot launch counter: never reset)
static int conv_p8_split_scratch(icl_ctx *ctx, hipStream_t strm, int tiles, conv_args &a)
{
    icl_sk_slot *sl = nullptr;
    for (auto &s : ctx->sk)
        if (s.part && s.stream == strm) sl = &s;
    if (!sl)
        for (auto &s : ctx->sk)
            if (!s.part && !sl) sl = &s;
    if (!sl) return ICL_ERR_NOMEM; // more streams than slots: the caller falls back to the one-workgroup-per-tile form
    if (sl->cap < tiles) {
        if (sl->part) {
            ICL_HIP(ctx, hipStreamSynchronize(strm));
            (void)hipFree(sl->part);
            (void)hipFree(sl->flag);
            sl->part = nullptr;
            sl->flag = nullptr;
            sl->cap = 0;
        }
        if (tiles > 4096) return ICL_ERR_UNSUPPORTED; // (32-bit offsets into the partner sums)
        const int cap = std::max(tiles, 128);
        ICL_HIP(ctx, hipMalloc(&sl->part, (size_t)cap * 32 * 512 * 16));
        ICL_HIP(ctx, hipMalloc((void **)&sl->flag, (size_t)cap * 4));
        ICL_HIP(ctx, hipMemsetAsync(sl->flag, 0, (size_t)cap * 4, strm)); // (on the launch stream: the streams are non-blocking, a null-stream memset would not be ordered with them)
        sl->cap = cap;
        sl->stream = strm;
        sl->epoch = 0;
    }
    a.sk_part = sl->part;
    a.sk_flag = sl->flag;
    a.sk_epoch = ++sl->epoch;
    return ICL_OK;
}

// c: conv_select's choice (family CONV_P8) for a, whose gx and gy are the choice's.  Returns whether the split form ran: it is what the choice
// wanted AND its scratch could be had (otherwise: one workgroup per tile).
template <int MW, int NWV, bool X3>
static bool launch_conv_p8_t(icl_ctx *ctx, conv_args &a, const conv_choice &c)
{
    hipStream_t strm = ctx->cur_stream ? ctx->cur_stream : ctx->stream;
    if constexpr (NWV == 4 && !X3) {
        if (c.split && conv_p8_split_scratch(ctx, strm, (int)c.blocks, a) == ICL_OK) {
            const dim3 grid2(2 * c.blocks);
            if (c.taps) hipLaunchKernelGGL((conv_p8_kernel<MW, NWV, true, false, true>), grid2, dim3(512), 0, strm, a);
            else hipLaunchKernelGGL((conv_p8_kernel<MW, NWV, false, false, true>), grid2, dim3(512), 0, strm, a);
            return true;
        }
    }
    const dim3 grid(c.blocks);
    if (c.dual) hipLaunchKernelGGL((conv_p8_kernel<MW, NWV, false, true, false, X3>), grid, dim3(512), 0, strm, a);
    else if (c.taps) hipLaunchKernelGGL((conv_p8_kernel<MW, NWV, true, false, false, X3>), grid, dim3(512), 0, strm, a);
    else hipLaunchKernelGGL((conv_p8_kernel<MW, NWV, false, false, false, X3>), grid, dim3(512), 0, strm, a);
    return false;
}
template <bool X3 = false>
static bool launch_conv_p8(icl_ctx *ctx, conv_args &a, const conv_choice &c)
{
    return c.layout == 1 ? launch_conv_p8_t<2, 4, X3>(ctx, a, c) : launch_conv_p8_t<4, 2, X3>(ctx, a, c);
}
