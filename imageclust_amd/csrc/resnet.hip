// resnet.hip -- hand-written ResNet50-v1 forward for gfx950: the embedding half of the hot path.
//
// Replaces LoadPretrainedModelONNX / GetImageEmbedding
//   (/root/reference/internal/embeddings/embeddings.go:28-43, :119-163), i.e. the OpenCV-DNN forward
// of resnet50-v1-7.onnx that the reference reaches through gocv (batch 1, CPU, serialised by NetMutex :133).
// PreprocessImage (:46-116) is image_io.hip.  This unit holds the kernels, the launch dispatch, the forward pass and the embed drivers;
// the model and its loader are model.hip, icl_embed_file's coalescing queue is embed_file.hip, what they share is resnet_model.h.
//
// Layout: activations NHWC (channels contiguous) in bf16 (throughput), split bf16 or f32 (parity); weights re-packed once
// at load to [Cout][KH][KW][Cin] so every implicit-GEMM K-chunk is a contiguous run of input channels of ONE
// filter tap.  Which kernel a convolution takes is decided in conv_select.h (conv_wr_kernel, conv_p8_kernel, conv3x3_halo_kernel or
// conv_igemm_kernel, in that order of precedence); launch_conv_t is that choice followed by one switch.  The kernels of this file are the
// 128 x BN ones: conv_igemm_kernel computes a 128(pixels) x BN(channels) output tile
// per 256-thread workgroup, K staged through XOR-swizzled LDS in 64-byte row chunks, v_mfma_f32_32x32x16_bf16
// (or v_mfma_f32_32x32x2_f32 in parity mode) with the WEIGHTS as the MFMA A operand so that each lane ends up
// holding 4 consecutive output channels of one pixel -> contiguous NHWC stores; BatchNorm (folded to
// scale/shift), conv bias, residual add and ReLU are fused into the epilogue.  The 7x7/2 stem (stem_conv_kernel) shares
// the MFMA step and the epilogue but gathers its A tile straight from the u8 image (K = 147 padded to 192), which also
// performs the reference's RGB/255 scaling (embeddings.go:96).
#include "icl_common.h"
#include "mfma_tile.h"
#include "resnet_model.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "conv_select.h" // conv_args, the kernel choice
static_assert(CONV_PREC_FP32 == ICL_PREC_FP32 && CONV_PREC_BF16 == ICL_PREC_BF16 && CONV_PREC_BF16X3 == ICL_PREC_BF16X3 && CONV_TILE_M == CV_BM && CONV_ROW_BYTES == CV_ROWB,
              "conv_select.h restates these constants");

#include "resnet_fused.h"
#include "conv_p8.h"
#include "conv_wr.h"

// Epilogue: y = relu(acc*scale + shift (+ residual)).
// accumulators (lane = pixel, 4 consecutive channels per register quad) -> fp32 LDS tile [pixel][channel] -> one
// 16-byte channel chunk per lane, so residual reads and output stores are whole contiguous rows; a lane's chunk column
// is fixed, so it needs only its own KE scale/shift values.  Callers must have finished reading the staged tiles.
// residual chunks of one lane for both 64-row halves of a tile (conv_epilogue's access pattern); EARLY kernels issue
// these loads before the K loop so their latency is hidden behind it
template <typename T, int BN>
struct conv_resid {
    static constexpr int NPASS = 64 / (256 / (BN / T::KE));
    uint4 v[2][NPASS];
    uint4 lo[is_x3<T>::value ? 2 : 1][is_x3<T>::value ? NPASS : 1]; // BF16X3: the lo halves
};
// a tensor's row stride and the element offset of real channel c in a row: the split bf16 layout (BF16X3) holds 2 elements per channel
template <typename T>
__device__ __forceinline__ int64_t act_ld(int C) { return is_x3<T>::value ? 2 * (int64_t)C : (int64_t)C; }
template <typename T>
__device__ __forceinline__ int act_off(int c) { return is_x3<T>::value ? c + (c & ~31) : c; }
template <typename T, int BN, bool FULL>
__device__ __forceinline__ void conv_resid_load(const conv_args &p, conv_resid<T, BN> &r, int64_t m0, int n0, int tid)
{
    typedef typename T::elem elem;
    constexpr int CPR = BN / T::KE, RPP = 256 / CPR, NPASS = 64 / RPP;
    const elem *Rg = (const elem *)p.R;
    const int nl = (tid % CPR) * T::KE;
    constexpr bool X3 = is_x3<T>::value;
    if (!Rg) {
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                r.v[half][i] = make_uint4(0, 0, 0, 0);
                if (X3) r.lo[X3 ? half : 0][X3 ? i : 0] = make_uint4(0, 0, 0, 0);
            }
        return;
    }
    const elem *r0 = Rg + (m0 + tid / CPR) * act_ld<T>(p.Cout) + act_off<T>(n0 + nl); // one 64-bit row address, then uniform strides
    const int64_t pstride = (int64_t)RPP * act_ld<T>(p.Cout);
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int64_t m = m0 + half * 64 + tid / CPR + i * RPP;
            const bool in = FULL || m < p.M;
            r.v[half][i] = in ? *reinterpret_cast<const uint4 *>(r0 + (half * NPASS + i) * pstride) : make_uint4(0, 0, 0, 0);
            if (X3) r.lo[X3 ? half : 0][X3 ? i : 0] = in ? *reinterpret_cast<const uint4 *>(r0 + (half * NPASS + i) * pstride + 32) : make_uint4(0, 0, 0, 0);
        }
}

template <typename T, int BN, bool TILE2D = false, bool FULL = false, bool PRE = false>
__device__ __forceinline__ void conv_epilogue(const conv_args &p, unsigned char *smem, f32x16 (&acc)[BN / 64][2], int64_t m0, int n0,
                                              int tid, int wm, int wn, int fr, int fh, const conv_resid<T, BN> &pre)
{
    // TILE2D (stem): tile row r is pixel (r/16, r%16) of an 8x16 patch whose top-left output pixel is m0
    auto row_m = [&](int ml) -> int64_t { return TILE2D ? m0 + (int64_t)(ml >> 4) * p.Wo + (ml & 15) : m0 + ml; };
    typedef typename T::elem elem;
    constexpr int NT = BN / 64;
    constexpr int EP_LD = BN + 4; // fp32 epilogue tile row stride (floats)
    float *ep = reinterpret_cast<float *>(smem);
    elem *Yg = (elem *)p.Y;
    const elem *Rg = (const elem *)p.R;
    constexpr int CPR = BN / T::KE;   // 16-byte output chunks per tile row
    constexpr int RPP = 256 / CPR;    // tile rows covered per pass
    constexpr int NPASS = 64 / RPP;   // passes per 64-row half tile
    const int nl = (tid % CPR) * T::KE;
    constexpr bool X3 = is_x3<T>::value;
    const int64_t yld = act_ld<T>(p.Cout);
    const int ycol = act_off<T>(n0 + nl);
    elem *Yfull = Yg + (m0 + tid / CPR) * yld + ycol;
    float sc[T::KE], sh[T::KE];
#pragma unroll
    for (int q = 0; q < T::KE; q += 4) {
        const float4 a4 = *reinterpret_cast<const float4 *>(p.scale + n0 + nl + q);
        const float4 b4 = *reinterpret_cast<const float4 *>(p.shift + n0 + nl + q);
        sc[q] = a4.x; sc[q + 1] = a4.y; sc[q + 2] = a4.z; sc[q + 3] = a4.w;
        sh[q] = b4.x; sh[q + 1] = b4.y; sh[q + 2] = b4.z; sh[q + 3] = b4.w;
    }
    // the 128-row tile goes through LDS in two 64-row halves (the waves with wm == half own those rows): the
    // epilogue then needs 64 x (BN+4) x 4 B of LDS, which lets single-k-step layers run 4 workgroups per CU
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        // all residual loads of the lane for this half are issued before any arithmetic
        uint4 rv[NPASS], rl[X3 ? NPASS : 1];
        if (PRE) {
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                rv[i] = pre.v[half][i];
                if (X3) rl[X3 ? i : 0] = pre.lo[X3 ? half : 0][X3 ? i : 0];
            }
        } else if (Rg) {
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                const int64_t m = row_m(half * 64 + tid / CPR + i * RPP);
                rv[i] = m < p.M ? *reinterpret_cast<const uint4 *>(Rg + m * yld + ycol) : make_uint4(0, 0, 0, 0);
                if (X3) rl[X3 ? i : 0] = m < p.M ? *reinterpret_cast<const uint4 *>(Rg + m * yld + ycol + 32) : make_uint4(0, 0, 0, 0);
            }
        }
        if (half) __syncthreads(); // everybody finished reading the first half
        if (wm == half) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ml = b * 32 + fr;
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nn = wn * (BN / 2) + a * 32 + 8 * g + 4 * fh;
                        *reinterpret_cast<float4 *>(ep + ml * EP_LD + nn) =
                            make_float4(acc[a][b][4 * g + 0], acc[a][b][4 * g + 1], acc[a][b][4 * g + 2], acc[a][b][4 * g + 3]);
                    }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            const int ml = tid / CPR + i * RPP;
            const int64_t m = row_m(half * 64 + ml);
            if (!FULL && m >= p.M) break;
            float v[T::KE];
#pragma unroll
            for (int q = 0; q < T::KE; q += 4) {
                const float4 t = *reinterpret_cast<const float4 *>(ep + ml * EP_LD + nl + q);
                v[q] = t.x * sc[q] + sh[q];
                v[q + 1] = t.y * sc[q + 1] + sh[q + 1];
                v[q + 2] = t.z * sc[q + 2] + sh[q + 2];
                v[q + 3] = t.w * sc[q + 3] + sh[q + 3];
            }
            if (Rg) {
                const elem *re = reinterpret_cast<const elem *>(&rv[i]);
                if constexpr (X3) {
                    const elem *rle = reinterpret_cast<const elem *>(&rl[i]);
#pragma unroll
                    for (int q = 0; q < T::KE; ++q) v[q] += T::to_f(re[q]) + T::to_f(rle[q]);
                } else {
#pragma unroll
                    for (int q = 0; q < T::KE; ++q) v[q] += T::to_f(re[q]);
                }
            }
            if (p.relu) {
#pragma unroll
                for (int q = 0; q < T::KE; ++q) v[q] = fmaxf(v[q], 0.0f);
            }
            uint4 ov, ol;
            elem *oe = reinterpret_cast<elem *>(&ov);
            if constexpr (X3) {
                elem *ole = reinterpret_cast<elem *>(&ol);
#pragma unroll
                for (int q = 0; q < T::KE; ++q) T::split(v[q], oe[q], ole[q]);
            } else {
#pragma unroll
                for (int q = 0; q < T::KE; ++q) oe[q] = T::from_f(v[q]);
            }
            elem *yo = (FULL && !TILE2D) ? Yfull + (int64_t)(half * NPASS + i) * ((int64_t)RPP * yld) // whole tile inside M: one 64-bit row address, then uniform strides
                                         : Yg + m * yld + ycol;
            *reinterpret_cast<uint4 *>(yo) = ov;
            if (X3) *reinterpret_cast<uint4 *>(yo + 32) = ol;
        }
    }
}

template <typename T, int BN, bool DUAL = false, int NST = 2, bool EARLY = false>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const conv_args p)
{
    typedef typename T::elem elem;
    constexpr int NT = BN / 64;                     // 32-channel MFMA row tiles per wave
    constexpr int STAGE = (BN + CV_BM) * CV_ROWB;   // one pipeline stage: BN weight rows then CV_BM activation rows
    constexpr int XI = CV_BM / 32;                  // activation LDS-DMA pieces per wave per stage (8 rows each)
    constexpr int WI = BN / 32;                     // weight pieces per wave per stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const int tile = xcd_remap(blockIdx.x, p.gx * p.gy);
    const int64_t m0 = (int64_t)(tile / p.gy) * CV_BM;
    const int n0 = (tile % p.gy) * BN;
    const elem *Xg = (const elem *)p.X;
    const elem *Wg = (const elem *)p.Wt;

    // ---- per-lane LDS-DMA roles (fixed for the whole K loop) ----
    // one piece = one wave-instruction = 8 tile rows x 128 B; lane -> (row = lane>>3, physical slot = lane&7)
    const int prow = lane >> 3, ps = lane & 7;
    int64_t xbase[XI];
    int xiy[XI], xix[XI];
    bool xok[XI];
    int xls[XI]; // logical k-chunk this lane fetches for its row (source-side swizzle)
    int64_t xbase2[DUAL ? XI : 1];
    const elem *X2g = (const elem *)p.X2;
    const int K1 = p.KH * p.KW * p.Cin; // k-steps below K1 read X, the rest read X2
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int row = wid * (CV_BM / 4) + i * 8 + prow;
        const int64_t m = m0 + row;
        xok[i] = m < p.M;
        // 32-bit index math (launch_conv checks M < 2^31): 64-bit divisions cost ~100 instructions each, and tiles
        // with few k-steps are bound by instruction issue
        const unsigned mm = xok[i] ? (unsigned)m : 0u;
        const unsigned t = mm / (unsigned)p.Wo;
        const int ox = (int)(mm - t * (unsigned)p.Wo);
        const int b = (int)(t / (unsigned)p.Ho);
        const int oy = (int)(t - (unsigned)b * (unsigned)p.Ho);
        xiy[i] = oy * p.stride - p.pad;
        xix[i] = ox * p.stride - p.pad;
        xbase[i] = (((int64_t)b * p.H + xiy[i]) * p.W + xix[i]) * p.Cin;
        xls[i] = lds_swz(row, ps);
        if (DUAL) xbase2[i] = (((int64_t)b * p.H2 + (int64_t)oy * p.stride2) * p.W2 + (int64_t)ox * p.stride2) * p.Cin2;
    }
    int64_t wbase[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = wid * (BN / 4) + i * 8 + prow;
        wbase[i] = (int64_t)(n0 + row) * p.K + lds_swz(row, ps) * T::KE;
    }

    f32x16 acc[NT][2];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;

    int kh = 0, kw = 0, ci0 = 0, k0 = 0; // position of the k-step being STAGED
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const unsigned wave_w = __builtin_amdgcn_readfirstlane(wid * (BN / 4) * CV_ROWB);
    const unsigned wave_x = __builtin_amdgcn_readfirstlane(BN * CV_ROWB + wid * (CV_BM / 4) * CV_ROWB);
    auto stage = [&](int buf) {
        const unsigned wdst = smem_base + buf * STAGE + wave_w;
        const unsigned xdst = smem_base + buf * STAGE + wave_x;
#pragma unroll
        for (int i = 0; i < WI; ++i) glds16_asm(Wg + wbase[i] + k0, wdst + i * 8 * CV_ROWB);
        if (DUAL && k0 >= K1) { // second operand: plain channel run of the strided pixel
#pragma unroll
            for (int i = 0; i < XI; ++i) {
                const elem *src = xok[i] ? X2g + xbase2[i] + (k0 - K1) + xls[i] * T::KE : (const elem *)p.zero;
                glds16_asm(src, xdst + i * 8 * CV_ROWB);
            }
            k0 += T::BK;
            return;
        }
        const int64_t tap_off = ((int64_t)kh * p.W + kw) * p.Cin + ci0;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const bool ok = xok[i] && (unsigned)(xiy[i] + kh) < (unsigned)p.H && (unsigned)(xix[i] + kw) < (unsigned)p.W;
            const elem *src = ok ? Xg + xbase[i] + tap_off + xls[i] * T::KE : (const elem *)p.zero;
            glds16_asm(src, xdst + i * 8 * CV_ROWB);
        }
        // advance to the next k-step (uniform)
        k0 += T::BK;
        ci0 += T::BK;
        if (ci0 == p.Cin) {
            ci0 = 0;
            if (++kw == p.KW) {
                kw = 0;
                ++kh;
            }
        }
    };

    const int nk = p.K / T::BK;
    constexpr int OPS = WI + XI; // vector-memory operations one wave issues per stage (vmcnt counts them in order)
    const int fr = lane & 31, fh = lane >> 5;
    static_assert(!EARLY || NST == 2, "EARLY uses the two-stage ring");
    if constexpr (EARLY) {
        // Few k-steps per tile: memory latency (~2 us) dwarfs a k-step's MFMAs, so the tile time is the number of
        // load round trips on its critical path.  Everything that can be requested at once is: the residual chunks of
        // the epilogue first, then BOTH stages; a stage buffer is refilled as soon as its step's MFMAs are done
        // (a second barrier per k-step), so two k-steps stay in flight.
        const bool full = m0 + CV_BM <= p.M; // every tile but the last along M
        conv_resid<T, BN> res;
        if (full) conv_resid_load<T, BN, true>(p, res, m0, n0, tid);
        else conv_resid_load<T, BN, false>(p, res, m0, n0, tid);
        stage(0);
        if (nk > 1) stage(1);
        for (int ks = 0; ks < nk; ++ks) {
            if (ks + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory"); // stage ks landed, ks+1 may be in flight
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            const unsigned char *wsm = smem + (ks & 1) * STAGE;
            conv_mma_kstep<T, BN>(wsm, wsm + BN * CV_ROWB, wm, wn, fr, fh, acc);
            if (ks + 2 < nk) {
                __syncthreads(); // everybody has read buffer ks&1
                stage(ks & 1);
            }
        }
        __syncthreads(); // the epilogue reuses the staging buffers
        if (full) conv_epilogue<T, BN, false, true, true>(p, smem, acc, m0, n0, tid, wm, wn, fr, fh, res);
        else conv_epilogue<T, BN, false, false, true>(p, smem, acc, m0, n0, tid, wm, wn, fr, fh, res);
        return;
    }
    // NST-stage ring, NST-1 k-steps of LDS-DMA in flight
    static_assert(NST >= 2 && NST <= 4 && (NST - 2) * OPS < 64, "counted vmcnt waits");
#pragma unroll
    for (int s0 = 0; s0 < NST - 1; ++s0)
        if (s0 < nk) stage(s0);
    for (int ks = 0; ks < nk; ++ks) {
        // stage ks must have landed; the (up to NST-2) stages issued after it may stay in flight
        const int later = (ks + NST - 2 < nk - 1 ? ks + NST - 2 : nk - 1) - ks;
        if (NST >= 4 && later >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * OPS) : "memory");
        else if (NST >= 3 && later >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads(); // everybody's pieces of stage ks are visible; all reads of stage ks-1 are done
        if (ks + NST - 1 < nk) stage((ks + NST - 1) % NST); // into the buffer read at step ks-1
        const unsigned char *wsm = smem + (ks % NST) * STAGE;
        conv_mma_kstep<T, BN>(wsm, wsm + BN * CV_ROWB, wm, wn, fr, fh, acc);
    }
    __syncthreads(); // the epilogue reuses the staging buffers
    conv_epilogue<T, BN>(p, smem, acc, m0, n0, tid, wm, wn, fr, fh, conv_resid<T, BN>());
}

// ------------------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolutions (every bottleneck's c2: 16 of the 53 launches, 37 % of the conv time) with an
// LDS-staged HALO tile.  conv_igemm_kernel stages, for each of the 9 taps, the 128 x 128-byte activation rows of that tap: the
// same input pixel crosses L2 -> LDS nine times, and the K-heavy layers sit at the CU's L2 -> LDS delivery rate, not at the
// MFMA rate.  Here a tile's 128 output pixels (linear in (b, oy, ox), as in conv_igemm_kernel) keep ONE image of
// their input neighbourhood in LDS per 128-byte channel chunk -- the input rows oy-1 .. oy+1 of every output row touched, W + 2
// pixels each (zero columns left and right) -- and all 9 taps read their A operand from it through per-lane pixel indices;
// only the weights (BN x 128 B) are staged per k-step.  L2 -> LDS bytes per k-step: 16 KB + 30 KB / 9 instead of 32 KB
// (Cin = 128, W = 28), LDS-DMA pieces per wave and k-step 4 + 1 instead of 8.
//   k order: (channel chunk, kh, kw, channel in chunk) -- fixed per output element, so results do not depend on the batch.
//   rows of a neighbouring IMAGE that fall into the halo are loaded like any other row; a lane whose output row is the first /
//   last of its image reads the three "zero pixels" behind the image instead (the conv's zero padding).
// ------------------------------------------------------------------------------------------------------------
// (HALO_MAXP, conv_select.h: halo pieces of 8 pixels x 128 B a wave fetches per channel chunk, i.e. tiles of up to 384 halo pixels)
// HALO_WS weight stages: 3 (two k-steps of weights in flight) where two workgroups still fit a CU's 160 KB of LDS, else 2 --
// measured (W = 28, Cin = 128: 81 KB with three stages): one workgroup per CU costs 37 % on that layer, the third stage gains 0-2 % elsewhere
template <typename T, int BN, int HALO_WS>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(const conv_args p, int npw /* halo pieces per wave */)
{
    typedef typename T::elem elem;
    constexpr int NT = BN / 64;
    constexpr int WI = BN / 32;          // weight pieces per wave per k-step
    constexpr int WST = BN * CV_ROWB;    // one weight stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; // [halo image: 4*npw pieces][4 zero pixels][HALO_WS weight stages]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const int tile = xcd_remap(blockIdx.x, p.gx * p.gy);
    const int64_t m0 = (int64_t)(tile / p.gy) * CV_BM;
    const int n0 = (tile % p.gy) * BN;
    const elem *Xg = (const elem *)p.X;
    const elem *Wg = (const elem *)p.Wt;
    const int Wd = p.W, P = Wd + 2, H = p.H;
    const int halo_bytes = 4 * npw * 1024;
    const int ZP = halo_bytes >> 7; // pixel index of the first zero pixel
    const int R0 = (int)((unsigned)m0 / (unsigned)Wd), Rlo = R0 - 1, totalR = p.B * H; // global rows (b * H + y); launch_conv checks M < 2^31
    // ---- halo fill roles: piece = 8 consecutive halo pixels x 128 B; lane -> (pixel = lane >> 3, physical 16-byte slot = lane & 7)
    const int prow = lane >> 3, ps = lane & 7;
    int64_t hoff[HALO_MAXP]; // element offset of this lane's source chunk for channel chunk 0, or -1: the zero page
#pragma unroll
    for (int i = 0; i < HALO_MAXP; ++i) {
        const int px = (wid * npw + i) * 8 + prow;
        const int r = (int)((unsigned)px / (unsigned)P), c = px - r * P - 1, Rg = Rlo + r;
        const bool ok = i < npw && (unsigned)Rg < (unsigned)totalR && (unsigned)c < (unsigned)Wd;
        hoff[i] = ok ? ((int64_t)Rg * Wd + c) * p.Cin + lds_swz(px, ps) * T::KE : -1;
    }
    int64_t wbase[WI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int row = wid * (BN / 4) + i * 8 + prow;
        wbase[i] = (int64_t)(n0 + row) * p.K + lds_swz(row, ps) * T::KE;
    }
    // ---- A-operand roles: the two output pixels of this lane (tile rows wm*64 + b*32 + fr) and, per filter row kh, the halo
    // pixel under tap (kh, kw = 0); kw adds to the pixel index
    const int fr = lane & 31, fh = lane >> 5;
    int abase[2][3];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int64_t m = m0 + wm * 64 + b * 32 + fr;
        const bool valid = m < p.M;
        const unsigned mm = valid ? (unsigned)m : (unsigned)m0;
        const int R = (int)(mm / (unsigned)Wd), ox = (int)(mm - (unsigned)R * (unsigned)Wd);
        const int oy = R - (int)((unsigned)R / (unsigned)H) * H;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int iy = oy + kh - 1;
            abase[b][kh] = (valid && (unsigned)iy < (unsigned)H) ? (R + kh - 1 - Rlo) * P + ox : ZP;
        }
    }
    f32x16 acc[NT][2];
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.0f;
    const unsigned smem_base = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    const unsigned halo_dst = __builtin_amdgcn_readfirstlane(smem_base + wid * npw * 1024);
    const unsigned w_dst = __builtin_amdgcn_readfirstlane(smem_base + halo_bytes + 512 + wid * (BN / 4) * CV_ROWB);
    auto stage_halo = [&](int ci0) {
#pragma unroll
        for (int i = 0; i < HALO_MAXP; ++i)
            if (i < npw) glds16_asm(hoff[i] >= 0 ? (const void *)(Xg + hoff[i] + ci0) : p.zero, halo_dst + i * 1024);
    };
    auto stage_w = [&](int k0, int buf) {
#pragma unroll
        for (int i = 0; i < WI; ++i) glds16_asm(Wg + wbase[i] + k0, w_dst + buf * WST + i * 8 * CV_ROWB);
    };
    if (tid < 32) reinterpret_cast<uint4 *>(smem + halo_bytes)[tid] = make_uint4(0, 0, 0, 0); // the zero pixels
    const int nchunk = p.Cin / T::BK;
    const int nk = 9 * nchunk;
    auto kof = [&](int q) { // k offset of k-step q = (chunk q / 9, tap q % 9) in the [Cout][kh][kw][Cin] weights
        const int c = q / 9, t = q - 9 * c;
        return t * p.Cin + c * T::BK;
    };
    constexpr int AHEAD = HALO_WS - 1; // k-steps of weights in flight beyond the current one
    stage_halo(0);
    stage_w(kof(0), 0);
    if (AHEAD > 1 && nk > 1) stage_w(kof(1), 1);
    int ks = 0; // k-step counter
    for (int c = 0; c < nchunk; ++c) {
#pragma unroll
        for (int t = 0; t < 9; ++t, ++ks) {
            const int kh = t / 3, kw = t % 3;
            // this step's weights have landed once only the next step's are outstanding; at a chunk's first tap the halo (issued
            // after them) must be in as well
            if (AHEAD < 2 || t == 0 || ks + 1 >= nk) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WI) : "memory");
            __syncthreads(); // ... and are visible to every wave; the weight buffer read at step ks-1 is free
            if (ks + AHEAD < nk) stage_w(kof(ks + AHEAD), (ks + AHEAD) % HALO_WS);
            const unsigned char *wsm = smem + halo_bytes + 512 + (ks % HALO_WS) * WST;
            if constexpr (is_x3<T>::value) { // split bf16: slot 2s + fh (hi) with slot 2s + 4 + fh (lo), three products (mfma_tile.h)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    uint4 wf[NT][2], xf[2][2];
#pragma unroll
                    for (int a = 0; a < NT; ++a) {
                        const int row = wn * (BN / 2) + a * 32 + fr;
#pragma unroll
                        for (int l = 0; l < 2; ++l) wf[a][l] = *reinterpret_cast<const uint4 *>(wsm + row * CV_ROWB + (lds_swz(row, 2 * s + 4 * l + fh) << 4));
                    }
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int px = abase[b][kh] + kw;
#pragma unroll
                        for (int l = 0; l < 2; ++l) xf[b][l] = *reinterpret_cast<const uint4 *>(smem + px * CV_ROWB + (lds_swz(px, 2 * s + 4 * l + fh) << 4));
                    }
#pragma unroll
                    for (int a = 0; a < NT; ++a)
#pragma unroll
                        for (int b = 0; b < 2; ++b) T::mma3(wf[a][0], wf[a][1], xf[b][0], xf[b][1], acc[a][b]);
                }
            } else
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uint4 wf[NT], xf[2];
#pragma unroll
                for (int a = 0; a < NT; ++a) {
                    const int row = wn * (BN / 2) + a * 32 + fr;
                    wf[a] = *reinterpret_cast<const uint4 *>(wsm + row * CV_ROWB + (lds_swz(row, 2 * s + fh) << 4));
                }
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int px = abase[b][kh] + kw;
                    xf[b] = *reinterpret_cast<const uint4 *>(smem + px * CV_ROWB + (lds_swz(px, 2 * s + fh) << 4));
                }
#pragma unroll
                for (int a = 0; a < NT; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) T::mma(wf[a], xf[b], acc[a][b]);
            }
            if (t == 8 && c + 1 < nchunk) {
                __syncthreads(); // every wave has read the last tap of this chunk's halo
                stage_halo((c + 1) * T::BK);
            }
        }
    }
    __syncthreads(); // the epilogue reuses the LDS
    conv_epilogue<T, BN>(p, smem, acc, m0, n0, tid, wm, wn, fr, fh, conv_resid<T, BN>());
}

// c: conv_select's choice (family CONV_HALO) for a, whose gx and gy are the choice's
template <typename T, int BN, int RING>
static void launch_conv3x3_halo(icl_ctx *ctx, const conv_args &a, const conv_choice &c)
{
    icl_lds_optin(ctx, (const void *)conv3x3_halo_kernel<T, BN, RING>, (int)conv3x3_halo_lds(BN, HALO_MAXP, RING));
    hipLaunchKernelGGL((conv3x3_halo_kernel<T, BN, RING>), dim3(c.blocks), dim3(c.threads), c.lds, ctx->cur_stream ? ctx->cur_stream : ctx->stream, a, c.npw);
}

// ------------------------------------------------------------------------------------------------------------
// Stem: conv0 7x7/2 p3 (3 -> 64) + BN + ReLU straight from the u8 image (K1 fused into the conv).
// Implicit GEMM with K ordered (kh, 24-slot row): k = kh*24 + kw*3 + c for kw*3+c < 21, the 3 slots that pad each
// filter row and the rows 168..191 carry ZERO weights.  With that order a 16-byte A chunk is KE consecutive BYTES of
// one input row, so nothing ever straddles a filter row.  One workgroup = an 8x16 patch of output pixels (98 per
// image, no ragged tiles): the 21 x 37-pixel u8 input patch is loaded once into LDS (zero outside the image = the
// conv's zero padding), chunks are cut out of it with aligned ds_read_b32 + v_alignbyte, scaled by float(1/255) as
// BlobFromImage does (embeddings.go:96), converted, and written into the swizzled LDS image the MFMA step reads.
// ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void stem_conv_kernel(const uint8_t *__restrict__ img, const conv_args p)
{
    // PERSISTENT workgroups (the grid holds as many as fit the CUs): the 64 x 192 weights are brought into LDS once per
    // workgroup, not once per 8x16 tile (25 088 tiles per batch of 256: 0.6 GB of L2 -> LDS traffic and a DMA round trip in front
    // of every tile), and the next tile's input patch is fetched into registers while this tile's MFMAs run.
    typedef typename T::elem elem;
    constexpr int BN = 64;
    constexpr int NKS = STEM_K / T::BK;            // k-steps: 3 (bf16) or 6 (f32)
    constexpr int WST = BN * CV_ROWB;              // bytes of one weight k-step image
    constexpr int XST = CV_BM * CV_ROWB;
    constexpr int PATCH = STEM_PH * STEM_PW + 16;  // + slack: chunk reads run up to 11 bytes past a row's last pixel
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[]; // [NKS weight steps][2 activation buffers][patch][fp32 epilogue tile]
    unsigned char *patch = smem + NKS * WST + 2 * XST;
    unsigned char *ep_smem = smem + ((NKS * WST + 2 * XST + PATCH + 15) & ~15);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const int ntiles = p.gx;
    const elem *Wg = (const elem *)p.Wt;
    // all weights (64 x 192) by LDS-DMA, once
    {
        const int prow = lane >> 3, ps = lane & 7;
#pragma unroll
        for (int j = 0; j < NKS; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wid * 16 + i * 8 + prow;
                __builtin_amdgcn_global_load_lds((gptr_t)(Wg + (int64_t)row * STEM_K + j * T::BK + lds_swz(row, ps) * T::KE),
                                                 (lptr_t)(smem + j * WST + (wid * 16 + i * 8) * CV_ROWB), 16, 0, 0);
            }
    }
    // input patch of a tile: rows iy = ty*16-3 .. +20, byte columns (tx*32-3)*3 .. ; zero outside the image.  The first byte
    // column is 3 mod 4 for every tile (tx*96 - 9), rows are 672 bytes and images 150528 bytes apart, so the patch is
    // fetched as ALIGNED dwords from byte column bx0-3 on (a dword is entirely inside or outside the image) and the
    // chunk addresses below carry the 3-byte offset
    constexpr int RW = STEM_PW / 4; // dwords per patch row
    static_assert(STEM_PW % 4 == 0, "patch rows are whole dwords");
    constexpr int NDW = STEM_PH * RW + 4;
    constexpr int NV = (NDW + 255) / 256;
    uint32_t pv[NV];
    auto patch_fetch = [&](int tile) {
        const int tx = tile % 7, ty = (tile / 7) % 14;
        const uint8_t *ib = img + (int64_t)(tile / 98) * (int64_t)ICL_IMG_BYTES;
        const int iy0 = ty * 16 - 3, bx0 = (tx * 32 - 3) * 3 - 3;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int i = tid + q * 256;
            const int pr = i / RW, pc = i - pr * RW;
            const int iy = iy0 + pr, bx = bx0 + pc * 4;
            const bool ok = i < NDW && pr < STEM_PH && (unsigned)iy < 224u && (unsigned)bx < 672u;
            pv[q] = ok ? *reinterpret_cast<const uint32_t *>(ib + iy * 672 + bx) : 0u;
        }
    };
    auto patch_store = [&]() {
        uint32_t *p32 = reinterpret_cast<uint32_t *>(patch);
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int i = tid + q * 256;
            if (i < NDW) p32[i] = pv[q];
        }
    };
    // chunk roles: lane cuts the chunk (row, logical slot ls) for 4 tile rows; ls is fixed per lane
    const int ls = tid & 7;
    const float sc255 = (float)(1.0 / 255.0);
    auto gather = [&](int j, int buf) {
        const int k0 = j * T::BK + ls * T::KE;     // first k of the chunk; never straddles a filter row (24 % KE == 0)
        const int kh = k0 / STEM_ROWK, r0 = k0 - kh * STEM_ROWK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 3) + 32 * i;
            const int oyl = row >> 4, oxl = row & 15;
            elem v[T::KE];
            if (kh < 7) {
                const int addr = (oyl * 2 + kh) * STEM_PW + oxl * 6 + r0 + 3; // + 3: the patch starts 3 bytes left of the tile
                const uint32_t *w32 = reinterpret_cast<const uint32_t *>(patch + (addr & ~3));
                const uint32_t d0 = w32[0], d1 = w32[1], d2 = w32[2];
                const int sh = addr & 3;
                const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
#pragma unroll
                for (int e = 0; e < T::KE; ++e) {
                    const uint32_t byte = ((e < 4 ? lo : hi) >> (8 * (e & 3))) & 0xffu;
                    v[e] = T::from_f((float)byte * sc255);
                }
            } else {
#pragma unroll
                for (int e = 0; e < T::KE; ++e) v[e] = T::from_f(0.0f);
            }
            *reinterpret_cast<uint4 *>(smem + NKS * WST + buf * XST + row * CV_ROWB + (lds_swz(row, ls) << 4)) = *reinterpret_cast<const uint4 *>(v);
        }
    };
    const int fr = lane & 31, fh = lane >> 5;
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    patch_fetch(tile);
    patch_store();
    __syncthreads();
    for (;;) {
        const int tx = tile % 7, ty = (tile / 7) % 14;
        const int64_t b = tile / 98;
        const int64_t m0 = (b * 112 + ty * 8) * 112 + tx * 16;
        const int next = tile + (int)gridDim.x;
        const bool has_next = next < ntiles; // workgroup-uniform
        f32x16 acc[1][2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][bb][r] = 0.0f;
        gather(0, 0);
        if (has_next) patch_fetch(next); // in flight while this tile is computed
        __syncthreads();                 // (the first time: also drains the weight DMA)
#pragma unroll
        for (int j = 0; j < NKS; ++j) {
            if (j + 1 < NKS) gather(j + 1, (j + 1) & 1);
            conv_mma_kstep<T, BN>(smem + j * WST, smem + NKS * WST + (j & 1) * XST, wm, wn, fr, fh, acc);
            __syncthreads();
        }
        if (has_next) patch_store(); // every gather of this tile has read the patch
        conv_epilogue<T, BN, true>(p, ep_smem, acc, m0, 0, tid, wm, wn, fr, fh, conv_resid<T, BN>());
        if (!has_next) break;
        tile = next;
        __syncthreads(); // the next patch is in LDS, the epilogue tile is free again
    }
}

template <typename T>
static constexpr size_t stem_lds_bytes()
{
    // weights + two activation buffers + the input patch, then (16-byte aligned) the fp32 epilogue tile: the weights stay resident
    return (((size_t)(STEM_K / T::BK) * 64 * CV_ROWB + 2 * (size_t)CV_BM * CV_ROWB + STEM_PH * STEM_PW + 16 + 15) & ~(size_t)15) + (size_t)64 * (64 + 4) * 4;
}

// MaxPool 3x3/2 p1 (padding never wins), NHWC, one thread per 16-byte channel chunk of one output pixel.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_kernel(const typename T::elem *__restrict__ in, int B, int H, int C,
                                                     typename T::elem *__restrict__ out)
{
    typedef typename T::elem elem;
    const int Ho = H / 2, CH = C / T::KE;
    const int64_t total = (int64_t)B * Ho * Ho * CH;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int ch = (int)(t % CH);
        const int64_t m = t / CH;
        const int ox = (int)(m % Ho), oy = (int)((m / Ho) % Ho), b = (int)(m / ((int64_t)Ho * Ho));
        float best[T::KE];
#pragma unroll
        for (int e = 0; e < T::KE; ++e) best[e] = -INFINITY;
        for (int kh = 0; kh < 3; ++kh)
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = oy * 2 - 1 + kh, ix = ox * 2 - 1 + kw;
                if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)H) continue;
                const uint4 raw = *reinterpret_cast<const uint4 *>(in + (((int64_t)b * H + iy) * H + ix) * C + ch * T::KE);
                const elem *pv = reinterpret_cast<const elem *>(&raw);
#pragma unroll
                for (int e = 0; e < T::KE; ++e) {
                    const float f = T::to_f(pv[e]);
                    if (f > best[e]) best[e] = f;
                }
            }
        elem o[T::KE];
#pragma unroll
        for (int e = 0; e < T::KE; ++e) o[e] = T::from_f(best[e]);
        *reinterpret_cast<uint4 *>(out + m * C + ch * T::KE) = *reinterpret_cast<const uint4 *>(o);
    }
}

// GlobalAveragePool over HW positions -> fp32 [B][C] (sequential fp32 sum, then / HW).
template <typename T>
__global__ __launch_bounds__(256) void avgpool_kernel(const typename T::elem *__restrict__ in, int B, int HW, int C,
                                                     float *__restrict__ out, int64_t out_ld)
{
    const int64_t total = (int64_t)B * C;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(t % C);
        const int64_t b = t / C;
        float s = 0.0f;
        if constexpr (is_x3<T>::value) { // split bf16: hi + lo of every position
            const typename T::elem *q = in + b * HW * 2 * C + c + (c & ~31);
            for (int i = 0; i < HW; ++i) s += T::to_f(q[(int64_t)i * 2 * C]) + T::to_f(q[(int64_t)i * 2 * C + 32]);
        } else {
            for (int i = 0; i < HW; ++i) s += T::to_f(in[(b * HW + i) * C + c]);
        }
        out[b * out_ld + c] = s / (float)HW;
    }
}

// dense0: y[b][o] = sum_i x[b][i] * W[o][i] + bias[o]; one wave per output, fp32.
__global__ __launch_bounds__(256) void fc_kernel(const float *__restrict__ x, const float *__restrict__ W, const float *__restrict__ bias,
                                                int B, int nin, int nout, float *__restrict__ y)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t t = wave; t < (int64_t)B * nout; t += nw) {
        const int o = (int)(t % nout);
        const int64_t b = t / nout;
        float s = 0.0f;
        for (int i = lane * 4; i < nin; i += 256) {
            const float4 xv = *reinterpret_cast<const float4 *>(x + b * nin + i);
            const float4 wv = *reinterpret_cast<const float4 *>(W + (int64_t)o * nin + i);
            s += xv.x * wv.x + xv.y * wv.y + xv.z * wv.z + xv.w * wv.w;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) y[b * nout + o] = s + bias[o];
    }
}

// ------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------
// c: conv_select's choice (family CONV_IGEMM) for a, whose gx and gy are the choice's
template <typename T, int BN, bool DUAL, bool EARLY>
static void launch_conv_igemm(icl_ctx *ctx, const conv_args &a, const conv_choice &c)
{
    icl_lds_optin(ctx, (const void *)conv_igemm_kernel<T, BN, DUAL, 2, EARLY>, (int)conv_igemm_lds(BN, 2)); // > 64 KiB of dynamic LDS
    hipLaunchKernelGGL((conv_igemm_kernel<T, BN, DUAL, 2, EARLY>), dim3(c.blocks), dim3(c.threads), c.lds, ctx->cur_stream ? ctx->cur_stream : ctx->stream, a);
}

// What conv_select reads besides the shape, from the context and the environment.  ICL_CONV_MODE, ICL_FUSE and ICL_WR_PT256 (A/B measurements
// and the tests that compare the forms) are read here, once per process, and nowhere else.
//   ICL_CONV_MODE  0 = plain two-stage loop, 2 = no halo kernel for the 3x3 layers (default 1)
//   ICL_WR_PT256   tile height of conv_wr_kernel's K = 256 layers, 32 | 64 (default 64)
//   ICL_FUSE       bit 0 stem + maxpool in one launch, bit 1 the identity bottlenecks of stage 1 in one launch each, bit 2 stage 1's first
//                  bottleneck (downsample branch), bit 3 (with bit 0, bf16) the stem that reads its B operand straight from a bf16 patch
//                  (stem2_pool_kernel).  Default: all.
struct fwd_env {
    int conv_mode, wr_pt256, fuse;
};
static const fwd_env &forward_env()
{
    static const fwd_env e = [] {
        const char *m = getenv("ICL_CONV_MODE"), *p = getenv("ICL_WR_PT256"), *f = getenv("ICL_FUSE");
        return fwd_env{m ? atoi(m) : 1, p && atoi(p) == 32 ? 32 : 64, f ? atoi(f) : 15};
    }();
    return e;
}
static int fuse_mask() { return forward_env().fuse; }
static conv_opts conv_opts_of(const icl_ctx *ctx)
{
    const fwd_env &e = forward_env();
    return conv_opts{ctx->conv_p8, ctx->conv_wr, ctx->conv_sk, ctx->conv_sk_min_k, e.conv_mode, e.wr_pt256, ctx->prop.multiProcessorCount};
}

// One convolution by its choice (conv_select.h): one switch over the family.  a is given in real channels; the kernels get their own view of it
// (conv_kernel_view: the split layout of BF16X3 as bf16 tensors of twice the channels) with the choice's tile counts.
template <typename T>
static int launch_conv_t(icl_ctx *ctx, int prec, const conv_args &real, const conv_choice &c)
{
    constexpr bool X3 = is_x3<T>::value;
    if (c.family == CONV_UNSUPPORTED) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s", c.why);
    conv_args a = conv_kernel_view(prec, real);
    a.gx = c.gx;
    a.gy = c.gy;
    icl_prof_scope ps(ctx, a.Cout % 128 == 0 ? ICL_K_CONV : ICL_K_CONV64, 2.0 * (double)real.M * real.Cout * real.K, 0.0);
    bool split = false;
    switch (c.family) {
    case CONV_WR:
        launch_conv_wr(ctx, a, c);
        break;
    case CONV_P8:
        if constexpr (std::is_same<T, BF16>::value || X3) split = launch_conv_p8<X3>(ctx, a, c);
        break;
    case CONV_HALO:
        if (c.bn == 128) c.ring == 3 ? launch_conv3x3_halo<T, 128, 3>(ctx, a, c) : launch_conv3x3_halo<T, 128, 2>(ctx, a, c);
        else c.ring == 3 ? launch_conv3x3_halo<T, 64, 3>(ctx, a, c) : launch_conv3x3_halo<T, 64, 2>(ctx, a, c);
        break;
    default: // CONV_IGEMM
        if (c.dual) c.early ? launch_conv_igemm<T, 128, true, true>(ctx, a, c) : launch_conv_igemm<T, 128, true, false>(ctx, a, c);
        else if (c.bn == 128) c.early ? launch_conv_igemm<T, 128, false, true>(ctx, a, c) : launch_conv_igemm<T, 128, false, false>(ctx, a, c);
        else c.early ? launch_conv_igemm<T, 64, false, true>(ctx, a, c) : launch_conv_igemm<T, 64, false, false>(ctx, a, c);
    }
    ++ctx->conv_launches[c.counter];
    ctx->conv_sk_launches += split;
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

static int launch_conv_prec(icl_ctx *ctx, int prec, const conv_args &a)
{
    const conv_choice c = conv_select(prec, a, conv_opts_of(ctx));
    return with_prec(prec, [&](auto t) { return launch_conv_t<decltype(t)>(ctx, prec, a, c); });
}

// the 7x7/2 stem of the loaded model (Y: the 112 x 112 x 64 tensor, or the pooled one of the fused kernels), gx work units
static inline conv_args conv_stem(const icl_model *m, const void *Wt, void *Y, int B, int gx)
{
    const conv_layer &L = m->conv[0];
    conv_args a = conv_plain(nullptr, Wt, Y, nullptr, L.scale, L.shift, m->zero, B, 224, 3, 64, 7, 2, 3, 1);
    a.K = STEM_K; // 147 padded: 7 filter rows of STEM_ROWK k slots
    a.gx = gx;
    a.gy = 1;
    return a;
}

// ---- per-layer entry points of the parity tests: host tensors in, host tensors out -----------------------------------------
// n values in the storage format of prec back to fp32 (unpack_storage; the stream that wrote src has been synchronised).  The other
// direction is upload_as (resnet_model.h), the loader's own.
static int from_dev(icl_ctx *ctx, int prec, const void *src, size_t n, float *dst)
{
    std::vector<uint16_t> t(pack_storage_bytes(prec, n) / 2);
    ICL_HIP(ctx, hipMemcpy(t.data(), src, t.size() * 2, hipMemcpyDeviceToHost));
    unpack_storage(prec, t.data(), n, dst);
    return ICL_OK;
}
// the 256 zero bytes the convolution kernels read for padded taps (the loaded model has its own: icl_model::zero)
static int zero_page(icl_ctx *ctx, const char *who, dev_guard &dz)
{
    ICL_TRY(icl_dev_alloc(ctx, dz, 256, "%s: zero page", who));
    ICL_HIP(ctx, hipMemset(dz.p, 0, 256));
    return ICL_OK;
}
// What the body of an entry point leaves to run_entry: the device buffers it made, which live until the output has been copied back,
// and that output: n values in the storage of prec, written on ctx->stream.
struct entry_io {
    std::deque<dev_guard> bufs;
    dev_guard &buf() { return bufs.emplace_back(); }
    const void *out = nullptr;
    int prec = ICL_PREC_FP32;
    size_t n = 0;
    void returns(int p, const void *d, size_t count) { prec = p; out = d; n = count; }
};
// The scaffold of the five entry points: under ctx->mu and on the context's device (with a model loaded, where the body needs one), the
// body uploads and launches on ctx->stream; the stream is synchronised whatever the body returned (its buffers are freed on return),
// the output goes to y as fp32 and the profile events are collected.
template <typename F>
static int run_entry(icl_ctx *ctx, const char *who, bool need_model, float *y, F &&body)
{
    return no_throw(ctx, who, [&]() -> int {
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        if (need_model && !ctx->model) return icl_fail(ctx, ICL_ERR_NOMODEL, "no model loaded (call icl_model_load_* first)");
        entry_io io;
        int rc = body(io);
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (!rc) rc = e == hipSuccess ? from_dev(ctx, io.prec, io.out, io.n, y) : icl_fail(ctx, ICL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        icl_prof_collect(ctx);
        return rc;
    });
}

extern "C" int icl_conv2d_fused(icl_ctx *ctx, int prec, const float *x, int B, int H, int Cin, const float *w, int Cout, int k,
                                int stride, int pad, const float *scale, const float *shift, const float *residual, int relu, float *y)
{
    if (!ctx || !x || !w || !scale || !shift || !y || B < 1 || H < 1 || k < 1 || stride < 1 || pad < 0)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_conv2d_fused: bad argument");
    if (!prec_ok(prec)) return icl_fail(ctx, ICL_ERR_ARG, "bad prec");
    if (Cin % 64 || Cout % 64) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_conv2d_fused needs Cin %% 64 == 0 and Cout %% 64 == 0");
    const int Ho = (H + 2 * pad - k) / stride + 1;
    if (Ho < 1) return icl_fail(ctx, ICL_ERR_ARG, "empty output");
    return run_entry(ctx, "icl_conv2d_fused", false, y, [&](entry_io &io) -> int {
        const size_t nx = (size_t)B * H * H * Cin, ny = (size_t)B * Ho * Ho * Cout;
        std::vector<float> wp;
        pack_ohwi(w, Cout, Cin, k, wp);
        dev_guard &dx = io.buf(), &dw = io.buf(), &dr = io.buf(), &dy = io.buf(), &dz = io.buf(), &dsc = io.buf(), &dsh = io.buf();
        ICL_TRY(upload_as(ctx, prec, &dx.p, x, nx));
        ICL_TRY(zero_page(ctx, "icl_conv2d_fused", dz));
        ICL_TRY(upload_as(ctx, prec, &dw.p, wp.data(), wp.size()));
        if (residual) ICL_TRY(upload_as(ctx, prec, &dr.p, residual, ny));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsc.p, scale, (size_t)Cout));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsh.p, shift, (size_t)Cout));
        ICL_TRY(icl_dev_alloc(ctx, dy, ny * prec_act_bytes(prec), "icl_conv2d_fused: output"));
        io.returns(prec, dy.p, ny);
        return launch_conv_prec(ctx, prec, conv_plain(dx.p, dw.p, dy.p, dr.p, (const float *)dsc.p, (const float *)dsh.p, dz.p, B, H, Cin, Cout, k, stride, pad, relu));
    });
}

// The dual-operand launch of launch_conv_fused_ds on the caller's tensors: a 1x1 convolution over x plus a 1x1 / stride2 convolution over
// x2 accumulated into the same tiles, weights concatenated per output row as [w1 | w2]; the kernel is chosen by launch_conv_prec as in
// the forward pass (icl_set_conv_options).  No residual: the production launch has none.
extern "C" int icl_conv2d_dual(icl_ctx *ctx, int prec, const float *x, int B, int Ho, int Cin, const float *w1, const float *x2, int H2, int Cin2,
                               const float *w2, int stride2, int Cout, const float *scale, const float *shift, int relu, float *y)
{
    if (!ctx || !x || !w1 || !x2 || !w2 || !scale || !shift || !y || B < 1 || Ho < 1 || H2 < 1 || stride2 < 1 || Cin < 1 || Cin2 < 1 || Cout < 1)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_conv2d_dual: bad argument");
    if (!prec_ok(prec)) return icl_fail(ctx, ICL_ERR_ARG, "bad prec");
    if ((int64_t)(Ho - 1) * stride2 >= H2) return icl_fail(ctx, ICL_ERR_ARG, "icl_conv2d_dual: output pixel %d reads row %lld of a %d-row second operand", Ho - 1, (long long)(Ho - 1) * stride2, H2);
    if (Cin % 64 || Cin2 % 64 || Cout % 128) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_conv2d_dual needs Cin %% 64 == 0, Cin2 %% 64 == 0 and Cout %% 128 == 0");
    if ((int64_t)B * Ho * Ho >= (1LL << 31)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_conv2d_dual: %lld output pixels exceed the kernel's 32-bit pixel index", (long long)B * Ho * Ho);
    return run_entry(ctx, "icl_conv2d_dual", false, y, [&](entry_io &io) -> int {
        const size_t nx = (size_t)B * Ho * Ho * Cin, nx2 = (size_t)B * H2 * H2 * Cin2, ny = (size_t)B * Ho * Ho * Cout;
        std::vector<float> wp;
        pack_row_concat(w1, Cin, w2, Cin2, Cout, wp);
        dev_guard &dx = io.buf(), &dx2 = io.buf(), &dw = io.buf(), &dy = io.buf(), &dz = io.buf(), &dsc = io.buf(), &dsh = io.buf();
        ICL_TRY(upload_as(ctx, prec, &dx.p, x, nx));
        ICL_TRY(upload_as(ctx, prec, &dx2.p, x2, nx2));
        ICL_TRY(zero_page(ctx, "icl_conv2d_dual", dz));
        ICL_TRY(upload_as(ctx, prec, &dw.p, wp.data(), wp.size()));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsc.p, scale, (size_t)Cout));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsh.p, shift, (size_t)Cout));
        ICL_TRY(icl_dev_alloc(ctx, dy, ny * prec_act_bytes(prec), "icl_conv2d_dual: output"));
        conv_args a = conv_plain(dx.p, dw.p, dy.p, nullptr, (const float *)dsc.p, (const float *)dsh.p, dz.p, B, Ho, Cin, Cout, 1, 1, 0, relu);
        conv_add_operand(a, dx2.p, H2, Cin2, stride2);
        io.returns(prec, dy.p, ny);
        return launch_conv_prec(ctx, prec, a);
    });
}

// The mapped 1x1 launch of a pruned block's c3 on the caller's tensors (bf16 operands): x is the compact [B][Ho][Ho][Cin] tensor,
// Ho = (H - 1) / sub + 1; residual (or NULL) and y are full-size [B][H][H][Cout] tensors.  y is read AND written: the launch stores the pixels
// (sub * oy, sub * ox) and every other value of y comes back as it went in (rounded to bf16).  A shape the streaming kernel's mapped form does
// not take is ICL_ERR_UNSUPPORTED: there is no other kernel behind this entry point.
extern "C" int icl_conv1x1_mapped(icl_ctx *ctx, const float *x, int B, int H, int sub, int Cin, const float *w, int Cout, const float *scale,
                                  const float *shift, const float *residual, int relu, float *y)
{
    if (!ctx || !x || !w || !scale || !shift || !y || B < 1 || H < 1 || sub < 1 || Cin < 1 || Cout < 1)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_conv1x1_mapped: bad argument");
    if ((int64_t)B * H * H * Cout * 2 >= (1LL << 31)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_conv1x1_mapped: the full tensor exceeds the kernel's 32-bit buffer offsets");
    return run_entry(ctx, "icl_conv1x1_mapped", false, y, [&](entry_io &io) -> int {
        const int prec = ICL_PREC_BF16;
        const prune_map pm = prune_map_make(sub, H, H);
        const size_t nx = (size_t)B * pm.Ho * pm.Wo * Cin, ny = (size_t)B * H * H * Cout;
        dev_guard &dx = io.buf(), &dw = io.buf(), &dr = io.buf(), &dy = io.buf(), &dz = io.buf(), &dsc = io.buf(), &dsh = io.buf();
        ICL_TRY(upload_as(ctx, prec, &dx.p, x, nx));
        ICL_TRY(zero_page(ctx, "icl_conv1x1_mapped", dz));
        ICL_TRY(upload_as(ctx, prec, &dw.p, w, (size_t)Cout * Cin));
        if (residual) ICL_TRY(upload_as(ctx, prec, &dr.p, residual, ny));
        ICL_TRY(upload_as(ctx, prec, &dy.p, y, ny));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsc.p, scale, (size_t)Cout));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &dsh.p, shift, (size_t)Cout));
        conv_args a = conv_plain(dx.p, dw.p, dy.p, dr.p, (const float *)dsc.p, (const float *)dsh.p, dz.p, B, pm.Ho, Cin, Cout, 1, 1, 0, relu);
        a.omap = pm;
        io.returns(prec, dy.p, ny);
        if (conv_select(prec, a, conv_opts_of(ctx)).family != CONV_WR) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_conv1x1_mapped: Cin = %d, Cout = %d is no shape of the streaming kernel's mapped form", Cin, Cout);
        return launch_conv_prec(ctx, prec, a);
    });
}

// workgroups per CU of the stem kernel a precision takes under an ICL_FUSE mask (forward_make_plan: stem2_pool_kernel, stem_pool_kernel or stem_conv_kernel)
static int stem_per_cu(int prec, int fuse)
{
    const size_t cu_lds = (size_t)160 * 1024;
    if (prec == ICL_PREC_BF16 && (fuse & 1) && (fuse & 8)) return std::max<int>(1, std::min<int>(5, (int)(cu_lds / stem2_lds_bytes())));
    if (prec == ICL_PREC_BF16X3 || (fuse & 1)) return std::max<int>(1, (int)(cu_lds / (prec == ICL_PREC_BF16 ? stem_pool_lds_bytes<BF16>() : stem_pool_lds_bytes<F32>())));
    return std::max<int>(1, (int)(cu_lds / (prec == ICL_PREC_BF16 ? stem_lds_bytes<BF16>() : stem_lds_bytes<F32>())));
}
static fwd_opts forward_opts_of(const icl_ctx *ctx, int prec)
{
    return fwd_opts{conv_opts_of(ctx), fuse_mask(), ctx->fwd_prune, stem_per_cu(prec, fuse_mask()), ctx->fwd_prune_fused, ctx->stem_max_blocks};
}

// grid: fwd_stem_blocks over the B * SP_STRIPS strips
template <typename T>
static void launch_stem_pool(icl_ctx *ctx, int prec, const uint8_t *d_img, int B, void *pooled, unsigned grid, hipStream_t strm)
{
    icl_model *m = ctx->model;
    if (prec == ICL_PREC_BF16 && (fuse_mask() & 8)) { // no im2col staging: B fragments straight from the bf16 patch
        const conv_layer &L0 = m->conv[0];
        icl_prof_scope ps(ctx, ICL_K_CONV64, 2.0 * (double)B * 112 * 112 * 64 * 147, 0.0);
        const int nunits = B * SP_STRIPS;
        hipLaunchKernelGGL(stem2_pool_kernel, dim3(grid), dim3(256), stem2_lds_bytes(), strm, d_img, (const uint16_t *)L0.wfold, L0.shift, (uint16_t *)pooled, nunits);
        return;
    }
    // BF16X3: the f32 stem (236 MFLOP per image), its pooled output written in the split layout
    constexpr bool SPLIT = is_x3<T>::value;
    typedef typename std::conditional<SPLIT, F32, T>::type TS;
    icl_lds_optin(ctx, (const void *)stem_pool_kernel<TS, SPLIT>, (int)stem_pool_lds_bytes<TS>());
    const conv_args a = conv_stem(m, m->conv[0].w[SPLIT ? ICL_PREC_FP32 : prec], pooled, B, B * SP_STRIPS * SP_TILES);
    icl_prof_scope ps(ctx, ICL_K_CONV64, 2.0 * (double)a.M * 64 * 147, 0.0);
    const int nunits = B * SP_STRIPS;
    hipLaunchKernelGGL((stem_pool_kernel<TS, SPLIT>), dim3(grid), dim3(256), stem_pool_lds_bytes<TS>(), strm, d_img, a, nunits);
}

// One stage-1 bottleneck in one launch (bf16): c1 -> c2 -> c3 (+ residual x | + downsample branch ds) + ReLU.  a: tensors, weights
// and B, H, W; the grid is decided here.  sub == 2 (identity form only): the pruned instantiation -- Y's pixels (2 oy, 2 ox) are written, the
// others keep what the buffer held (forward_make_plan decides when; prune_map.h).
static int launch_bneck56_args(icl_ctx *ctx, bneck_args &a, bool ds, int sub, hipStream_t strm)
{
    if (sub != 1 && (sub != 2 || ds)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "fused bottleneck: no kernel for sub = %d%s", sub, ds ? " with a downsample branch" : "");
    const int B = a.B;
    if ((int64_t)B * a.H * a.W * 512 >= (1LL << 31)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "fused bottleneck: batch of %d images exceeds the 32-bit buffer offsets", B);
    bneck56_grid(B, a.W, ctx->prop.multiProcessorCount, &a.nstrips, &a.ngroups);
#ifdef BN56_TIMERS
    static unsigned long long *dbg = nullptr;
    if (!dbg) (void)hipMalloc((void **)&dbg, 16 * 8);
    a.dbg = dbg;
#endif
    // the flops the result needs: conv1 on every pixel, conv2 and conv3 on the pixels that are read
    const double px = (double)B * a.H * a.W, px23 = (double)B * prune_extent(a.H, sub) * prune_extent(a.W, sub);
    icl_prof_scope ps(ctx, ICL_K_CONV, 2.0 * (px * 64.0 * (ds ? 64 : 256) + px23 * (64.0 * 576 + 256.0 * (ds ? 128 : 64))), 0.0);
    const dim3 grid((unsigned)(a.nstrips * a.ngroups));
    if (ds) {
        icl_lds_optin(ctx, (const void *)bneck56_kernel<true>, (int)bneck56_lds_bytes<true>());
        hipLaunchKernelGGL((bneck56_kernel<true>), grid, dim3(512), bneck56_lds_bytes<true>(), strm, a);
    } else if (sub == 2) {
        icl_lds_optin(ctx, (const void *)bneck56_kernel<false, 2>, (int)bneck56_lds_bytes<false>());
        hipLaunchKernelGGL((bneck56_kernel<false, 2>), grid, dim3(512), bneck56_lds_bytes<false>(), strm, a);
    } else {
        icl_lds_optin(ctx, (const void *)bneck56_kernel<false>, (int)bneck56_lds_bytes<false>());
        hipLaunchKernelGGL((bneck56_kernel<false>), grid, dim3(512), bneck56_lds_bytes<false>(), strm, a);
    }
    ICL_HIP(ctx, hipGetLastError());
#ifdef BN56_TIMERS
    if (getenv("BN56_PRINT")) {
        unsigned long long h[16];
        (void)hipStreamSynchronize(strm);
        (void)hipMemcpy(h, dbg, sizeof h, hipMemcpyDeviceToHost);
        const char *fn[8] = BN56_FRONT_SEGMENTS;
        const char *bn[8] = BN56_BACK_SEGMENTS;
        const int nsteps = ((B / a.ngroups) * (a.H + 1) + BN56_ROWS - 1) / BN56_ROWS;
        fprintf(stderr, "[bn56 %s] cycles per step (steps %d):\n  front:", ds ? "ds" : "id", nsteps);
        for (int k = 0; k < 8 && fn[k][0]; ++k) fprintf(stderr, " %s %.0f |", fn[k], (double)h[k] / nsteps);
        fprintf(stderr, "\n  back :");
        for (int k = 0; k < 8 && bn[k][0]; ++k) fprintf(stderr, " %s %.0f |", bn[k], (double)h[8 + k] / nsteps);
        fprintf(stderr, "\n");
    }
#endif
    return ICL_OK;
}

static int launch_bneck56(icl_ctx *ctx, const conv_layer &c1, const conv_layer &c2, const conv_layer &c3, const conv_layer *ds, const void *x, void *y,
                          int B, int sub, hipStream_t strm)
{
    bneck_args a = {};
    a.X = (const uint16_t *)x;
    a.Y = (uint16_t *)y;
    a.W1 = (const uint16_t *)c1.wfold;
    a.W2 = (const uint16_t *)c2.wfold;
    a.W3 = (const uint16_t *)(ds ? c3.wfused[ICL_PREC_BF16] : c3.wfold);
    a.sh1 = c1.shift; a.sh2 = c2.shift;
    a.sh3 = ds ? c3.shift_fused : c3.shift;
    a.B = B; a.H = c2.rec.hin; a.W = c2.rec.hin;
    return launch_bneck56_args(ctx, a, ds != nullptr, sub, strm);
}

// The plan of one forward pass of B images of the loaded model under the context's options as they are now (forward_make_plan, conv_select.h).
static int forward_plan_of(icl_ctx *ctx, int prec, int B, int head, int tap, fwd_plan *plan)
{
    const icl_model *m = ctx->model;
    icl_conv_rec recs[ICL_RESNET50_NCONV];
    for (int i = 0; i < m->nconv; ++i) recs[i] = m->conv[i].rec;
    *plan = forward_make_plan(recs, m->nconv, prec, B, head == ICL_HEAD_DENSE0, tap, forward_opts_of(ctx, prec));
    if (plan->err) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "forward pass, convolution %d (cin=%d cout=%d k=%d): %s", plan->err_layer, recs[plan->err_layer].cin, recs[plan->err_layer].cout, recs[plan->err_layer].k, plan->err);
    return ICL_OK;
}

// Runs a plan on lane `lane` and stream strm: each step's pointers are the lane's buffers and the model's weights.  d_out: the embeddings
// (no tap plan); a tap plan leaves its tensor in the lane's buffer plan.out.
template <typename T>
static int forward_batch(icl_ctx *ctx, int prec, const fwd_plan &plan, const uint8_t *d_img, int head, float *d_out, int lane, hipStream_t strm)
{
    typedef typename T::elem elem;
    icl_model *m = ctx->model;
    ctx->cur_stream = strm;
    const int B = plan.B;
    void *const *buf = m->buf[lane];
    float *pooled = head == ICL_HEAD_POOLED ? d_out : m->pooled[lane];
    for (const fwd_step &s : plan.steps) {
        const conv_layer &L = m->conv[s.layer];
        switch (s.kind) {
        case FWD_STEM2_POOL:
        case FWD_STEM_POOL: // conv0 + BN + ReLU + maxpool: the 112x112 tensor stays on the CU
            launch_stem_pool<T>(ctx, prec, d_img, B, buf[s.y], s.blocks, strm);
            break;
        case FWD_STEM:
            if constexpr (!is_x3<T>::value) {
                icl_lds_optin(ctx, (const void *)stem_conv_kernel<T>, (int)stem_lds_bytes<T>());
                const conv_args a = conv_stem(m, L.w[prec], buf[s.y], B, B * 98); // 8x16-pixel tiles: 14 x 7 per image
                icl_prof_scope ps(ctx, ICL_K_CONV64, 2.0 * (double)a.M * 64 * 147, 0.0);
                hipLaunchKernelGGL((stem_conv_kernel<T>), dim3(s.blocks), dim3(s.threads), stem_lds_bytes<T>(), strm, d_img, a);
            }
            break;
        case FWD_MAXPOOL:
            if constexpr (!is_x3<T>::value) {
                icl_prof_scope ps(ctx, ICL_K_EMBED_OTHER, 0.0, (double)B * (802816.0 + 200704.0) * sizeof(elem));
                hipLaunchKernelGGL((maxpool_kernel<T>), dim3(s.blocks), dim3(s.threads), 0, strm, (const elem *)buf[s.x], B, 112, 64, (elem *)buf[s.y]);
            }
            break;
        case FWD_BNECK56: // the whole bottleneck in one launch
            ICL_TRY(launch_bneck56(ctx, L, m->conv[s.layer + 1], m->conv[s.layer + 2], s.ds ? &m->conv[s.layer + 3] : nullptr, buf[s.x], buf[s.y], B, s.sub, strm));
            ctx->pruned_fused += s.sub == 2;
            break;
        case FWD_CONV: {
            conv_args a = s.a;
            a.X = buf[s.x]; a.Y = buf[s.y]; a.R = s.r != FWD_NONE ? buf[s.r] : nullptr; a.zero = m->zero;
            if (s.ds) { // both BN scales are folded into the concatenated weights
                a.Wt = L.wfused[prec]; a.scale = m->ones; a.shift = L.shift_fused; a.X2 = buf[s.x2];
            } else {
                a.Wt = L.w[prec]; a.scale = L.scale; a.shift = L.shift;
            }
            ICL_TRY(launch_conv_t<T>(ctx, prec, a, s.c));
            ctx->pruned_blocks += s.pruned;
            break;
        }
        case FWD_AVGPOOL: {
            icl_prof_scope ps(ctx, ICL_K_EMBED_OTHER, 0.0, (double)B * 49.0 * 2048.0 * (is_x3<T>::value ? 4 : sizeof(elem)));
            hipLaunchKernelGGL((avgpool_kernel<T>), dim3(s.blocks), dim3(s.threads), 0, strm, (const elem *)buf[s.x], B, 49, ICL_FEAT_DIM, pooled, (int64_t)ICL_FEAT_DIM);
            break;
        }
        default: { // FWD_FC
            icl_prof_scope ps(ctx, ICL_K_EMBED_OTHER, 2.0 * B * 2048.0 * 1000.0, 0.0);
            hipLaunchKernelGGL(fc_kernel, dim3(s.blocks), dim3(s.threads), 0, strm, pooled, m->fcw, m->fcb, B, ICL_FEAT_DIM, ICL_FC_OUT, d_out);
        }
        }
    }
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}

// The fused stem of the loaded model alone (conv0 7x7/2 + BN + ReLU + maxpool 3x3/2, stem_pool_kernel): img is B x 224x224x3
// u8 HWC RGB (host), out is [B][56][56][64] NHWC fp32 (host).  For the per-layer parity tests.
extern "C" int icl_stem_pool(icl_ctx *ctx, int prec, const uint8_t *img, int B, float *out)
{
    if (!ctx || !img || !out || B < 1) return icl_fail(ctx, ICL_ERR_ARG, "icl_stem_pool: bad argument");
    if (!prec_ok(prec)) return icl_fail(ctx, ICL_ERR_ARG, "bad prec");
    return run_entry(ctx, "icl_stem_pool", true, out, [&](entry_io &io) -> int {
        const size_t ny = (size_t)B * 56 * 56 * 64;
        dev_guard &dimg = io.buf(), &dy = io.buf();
        ICL_TRY(icl_dev_alloc(ctx, dimg, (size_t)B * ICL_IMG_BYTES, "icl_stem_pool: images"));
        ICL_TRY(icl_dev_alloc(ctx, dy, ny * prec_act_bytes(prec), "icl_stem_pool: output"));
        if (hipMemcpy(dimg.p, img, (size_t)B * ICL_IMG_BYTES, hipMemcpyHostToDevice) != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "icl_stem_pool: upload");
        const unsigned grid = fwd_stem_blocks((int64_t)B * SP_STRIPS, stem_per_cu(prec, fuse_mask() | 1), ctx->prop.multiProcessorCount, ctx->stem_max_blocks);
        with_prec(prec, [&](auto t) { launch_stem_pool<decltype(t)>(ctx, prec, (const uint8_t *)dimg.p, B, dy.p, grid, ctx->stream); });
        io.returns(prec, dy.p, ny);
        const hipError_t e = hipGetLastError();
        return e == hipSuccess ? ICL_OK : icl_fail(ctx, ICL_ERR_HIP, "icl_stem_pool: %s", hipGetErrorString(e));
    });
}

// One fused stage-1 bottleneck (bneck56_kernel, bf16 operands), host buffers, for the per-layer parity tests:
//   identity (wds == NULL, Cin = 256): y = relu(bn3(conv3(relu(bn2(conv2(relu(bn1(conv1(x))))))) + x)
//   downsample (wds != NULL, Cin = 64): y = relu(bn3(conv3(t2)) + bn_ds(conv_ds(x)))  (both BN scales folded into the weights)
// x: [B][H][W][Cin] NHWC, w1: [64][Cin], w2: [64][64][3][3] (OIHW), w3: [256][64], wds: [256][Cin]; y: [B][H][W][256].
// sub == 2 (icl_bottleneck56_sub): the pruned instantiation; every 16-bit element of y is set to `fill` before the launch.
static int bottleneck56_entry(icl_ctx *ctx, const float *x, int B, int H, int W, int Cin, const float *w1, const float *sc1, const float *sh1,
                              const float *w2, const float *sc2, const float *sh2, const float *w3, const float *sc3, const float *sh3,
                              const float *wds, const float *scds, const float *shds, int sub, const uint16_t *fill, float *y)
{
    if (!ctx || !x || !w1 || !sc1 || !sh1 || !w2 || !sc2 || !sh2 || !w3 || !sc3 || !sh3 || !y || B < 1 || H < 1 || W < 1)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_bottleneck56: bad argument");
    const bool has_ds = wds != nullptr;
    if (has_ds && (!scds || !shds)) return icl_fail(ctx, ICL_ERR_ARG, "icl_bottleneck56: downsample scale / shift missing");
    if (Cin != (has_ds ? 64 : 256)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_bottleneck56: Cin must be 256 (identity) or 64 (downsample branch)");
    if ((int64_t)B * H * W * 512 >= (1LL << 31)) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "icl_bottleneck56: tensor exceeds the kernel's 32-bit buffer offsets");
    return run_entry(ctx, "icl_bottleneck56", false, y, [&](entry_io &io) -> int {
        const size_t nx = (size_t)B * H * W * Cin, ny = (size_t)B * H * W * 256;
        // the loader's packing of stage 1: every BatchNorm scale goes into the weights before they are rounded; the downsample form
        // concatenates [W3 * s3 | Wds * sds] and adds the two shifts
        std::vector<float> f1, p2, f2, f3, fds, f3ds, h3(sh3, sh3 + 256);
        pack_row_scale(w1, sc1, 64, Cin, f1);
        pack_ohwi(w2, 64, 64, 3, p2);
        pack_row_scale(p2.data(), sc2, 64, 576, f2);
        pack_row_scale(w3, sc3, 256, 64, f3);
        if (has_ds) {
            pack_row_scale(wds, scds, 256, 64, fds);
            pack_row_concat(f3.data(), 64, fds.data(), 64, 256, f3ds);
            for (int co = 0; co < 256; ++co) h3[(size_t)co] = sh3[co] + shds[co];
        }
        const std::vector<float> &w3p = has_ds ? f3ds : f3;
        dev_guard &dx = io.buf(), &dy = io.buf(), &dw1 = io.buf(), &dw2 = io.buf(), &dw3 = io.buf(), &d1h = io.buf(), &d2h = io.buf(), &d3h = io.buf();
        ICL_TRY(upload_as(ctx, ICL_PREC_BF16, &dx.p, x, nx));
        ICL_TRY(upload_as(ctx, ICL_PREC_BF16, &dw1.p, f1.data(), f1.size()));
        ICL_TRY(upload_as(ctx, ICL_PREC_BF16, &dw2.p, f2.data(), f2.size()));
        ICL_TRY(upload_as(ctx, ICL_PREC_BF16, &dw3.p, w3p.data(), w3p.size()));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &d1h.p, sh1, 64));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &d2h.p, sh2, 64));
        ICL_TRY(upload_as(ctx, ICL_PREC_FP32, &d3h.p, h3.data(), 256));
        ICL_TRY(icl_dev_alloc(ctx, dy, ny * 2, "icl_bottleneck56: output"));
        bneck_args a = {};
        a.X = (const uint16_t *)dx.p; a.Y = (uint16_t *)dy.p; a.W1 = (const uint16_t *)dw1.p; a.W2 = (const uint16_t *)dw2.p; a.W3 = (const uint16_t *)dw3.p;
        a.sh1 = (const float *)d1h.p; a.sh2 = (const float *)d2h.p; a.sh3 = (const float *)d3h.p;
        a.B = B; a.H = H; a.W = W;
        io.returns(ICL_PREC_BF16, dy.p, ny);
        if (fill && hipMemsetD16Async((hipDeviceptr_t)dy.p, *fill, ny, ctx->stream) != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "icl_bottleneck56: fill");
        return launch_bneck56_args(ctx, a, has_ds, sub, ctx->stream); // the launch code of the forward pass
    });
}
extern "C" int icl_bottleneck56(icl_ctx *ctx, const float *x, int B, int H, int W, int Cin, const float *w1, const float *sc1, const float *sh1,
                                const float *w2, const float *sc2, const float *sh2, const float *w3, const float *sc3, const float *sh3,
                                const float *wds, const float *scds, const float *shds, float *y)
{
    return bottleneck56_entry(ctx, x, B, H, W, Cin, w1, sc1, sh1, w2, sc2, sh2, w3, sc3, sh3, wds, scds, shds, 1, nullptr, y);
}
// The identity form with the launch's `sub` (1: every pixel; 2: the pruned instantiation, which writes the pixels (2 oy, 2 ox) only) on a y
// whose every 16-bit element holds `fill` when the kernel starts: the pixels a launch does not write come back as that pattern.
extern "C" int icl_bottleneck56_sub(icl_ctx *ctx, const float *x, int B, int H, int W, const float *w1, const float *sc1, const float *sh1,
                                    const float *w2, const float *sc2, const float *sh2, const float *w3, const float *sc3, const float *sh3,
                                    int sub, int fill, float *y)
{
    if (sub < 1 || sub > 2 || fill < 0 || fill > 0xffff) return icl_fail(ctx, ICL_ERR_ARG, "icl_bottleneck56_sub: sub must be 1 or 2, fill a 16-bit pattern");
    const uint16_t f16 = (uint16_t)fill;
    return bottleneck56_entry(ctx, x, B, H, W, 256, w1, sc1, sh1, w2, sc2, sh2, w3, sc3, sh3, nullptr, nullptr, nullptr, sub, &f16, y);
}

// The forward pass of the loaded model up to a tap, for the per-block parity tests: forward_batch on lane 0 for ONE batch of B images
// (B <= the context's batch), ended after the stem + maxpool (tap 0: [B][56][56][64]) or after bottleneck `tap` (1..16, the 16th is
// [B][7][7][2048]); out receives that tensor as fp32 NHWC.
extern "C" int icl_embed_taps(icl_ctx *ctx, int prec, const uint8_t *img, int B, int tap, float *out)
{
    if (!ctx || !img || !out || B < 1 || tap < 0 || tap > 16) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_taps: bad argument");
    if (!prec_ok(prec)) return icl_fail(ctx, ICL_ERR_ARG, "bad prec");
    return run_entry(ctx, "icl_embed_taps", true, out, [&](entry_io &io) -> int {
        if (B > ctx->batch) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_taps: %d images exceed the batch of %d", B, ctx->batch);
        ICL_TRY(icl_model_ensure_ws(ctx, B, prec, 1));
        fwd_plan plan; // ends at the tapped block, whose tensor ([B][H][H][C]) it leaves in the lane's buffer plan.out
        ICL_TRY(forward_plan_of(ctx, prec, B, ICL_HEAD_POOLED, tap, &plan));
        dev_guard &dimg = io.buf();
        ICL_TRY(icl_dev_alloc(ctx, dimg, (size_t)B * ICL_IMG_BYTES, "icl_embed_taps: image buffer"));
        if (hipMemcpy(dimg.p, img, (size_t)B * ICL_IMG_BYTES, hipMemcpyHostToDevice) != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "icl_embed_taps: upload");
        const int rc = with_prec(prec, [&](auto t) { return forward_batch<decltype(t)>(ctx, prec, plan, (const uint8_t *)dimg.p, ICL_HEAD_POOLED, nullptr, 0, ctx->stream); });
        ctx->cur_stream = nullptr;
        io.returns(prec, ctx->model->buf[0][plan.out], (size_t)B * plan.H * plan.H * plan.C);
        return rc; // (run_entry synchronises also after a failed launch: dimg is freed on its return)
    });
}

int icl_embed_dev_locked(icl_ctx *ctx, const uint8_t *d_img, int64_t n, int head, int prec, float *d_out)
{
    if (!ctx->model) return icl_fail(ctx, ICL_ERR_NOMODEL, "no model loaded (call icl_model_load_* first)");
    if (!head_ok(head)) return icl_fail(ctx, ICL_ERR_ARG, "head must be 2048 or 1000");
    if (!prec_ok(prec)) return icl_fail(ctx, ICL_ERR_ARG, "prec must be ICL_PREC_FP32, ICL_PREC_BF16 or ICL_PREC_BF16X3");
    if (n == 0) return ICL_OK;
    const int batch = (int)std::min<int64_t>(ctx->batch, n);
    // Two forward passes in flight on two streams (each its own activation workspace): batches stay at the configured
    // size, and the launches of one pass fill the CUs the other leaves idle (late stages have few tiles, HBM-bound
    // layers meet MFMA-bound ones).  Per-kernel profiling brackets launches with events on the main stream: one lane.
    static const int lanes_env = [] {
        const char *e = getenv("ICL_EMBED_STREAMS");
        return e ? atoi(e) : 2;
    }();
    int lanes = (ctx->prof_mask || lanes_env < 2) ? 1 : std::min(lanes_env, ICL_MAX_LANES);
    lanes = (int)std::min<int64_t>(lanes, (n + batch - 1) / batch);
    ICL_TRY(icl_model_ensure_ws(ctx, batch, prec, lanes));
    fwd_plan full, rest; // one plan for the full batches and, for a ragged call, one for the last
    ICL_TRY(forward_plan_of(ctx, prec, batch, head, -1, &full));
    if (n % batch) ICL_TRY(forward_plan_of(ctx, prec, (int)(n % batch), head, -1, &rest));
    // whatever the exit: the events of this call are destroyed and no launch stream stays selected
    constexpr int DEPTH = 16;
    hipEvent_t ring[DEPTH + 2] = {}; // one per batch in flight, then the two that time the call
    hipEvent_t &e0 = ring[DEPTH], &e1 = ring[DEPTH + 1];
    struct exit_guard {
        icl_ctx *c;
        hipEvent_t *r;
        ~exit_guard()
        {
            c->cur_stream = nullptr;
            for (int q = 0; q < DEPTH + 2; ++q) if (r[q]) (void)hipEventDestroy(r[q]);
        }
    } eg{ctx, ring};
    ICL_HIP(ctx, hipEventCreate(&e0));
    ICL_HIP(ctx, hipEventCreate(&e1));
    ICL_HIP(ctx, hipEventRecord(e0, ctx->stream));
    auto lane_stream = [&](int l) { return l == 0 ? ctx->stream : l == 1 ? ctx->stream2 : ctx->model->xstream[l]; };
    auto join = [&]() -> hipError_t { // the main stream waits for every side stream; the first error, after trying them all
        hipError_t first = hipSuccess;
        for (int l = 1; l < lanes; ++l) {
            hipEvent_t ej = l == 1 ? ctx->ev_join : ctx->model->xjoin[l];
            hipError_t e = hipEventRecord(ej, lane_stream(l));
            if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ej, 0);
            if (first == hipSuccess) first = e;
        }
        return first;
    };
    if (lanes > 1) { // fork: the side streams start after everything already queued on the main stream
        ICL_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
        for (int l = 1; l < lanes; ++l) ICL_HIP(ctx, hipStreamWaitEvent(lane_stream(l), ctx->ev_fork, 0));
    }
    // At most DEPTH batches (DEPTH x 55 launches) are enqueued ahead of the GPU: the host waits for batch bi-DEPTH before it
    // enqueues batch bi.  The queues never run dry (hundreds of launches deep), and the number of dispatches in flight stays
    // bounded however many images a call embeds -- unbounded, a 100 000-image call had 21 500 launches outstanding, which
    // `rocprofv3 --pmc` does not survive (SIGSEGV in the tool once several thousand counter-instrumented dispatches are pending;
    // 2 200 are fine, 8 600 are not: profiles/README.md).
    int64_t bi = 0;
    for (int64_t i = 0; i < n; i += batch, ++bi) {
        const int B = (int)std::min<int64_t>(batch, n - i);
        const int lane = (int)(bi % lanes);
        hipStream_t strm = lane_stream(lane);
        hipEvent_t &ev = ring[bi % DEPTH];
        if (ev) ICL_HIP(ctx, hipEventSynchronize(ev)); // batch bi-DEPTH has finished
        else ICL_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ICL_TRY(with_prec(prec, [&](auto t) { return forward_batch<decltype(t)>(ctx, prec, B == batch ? full : rest, d_img + i * ICL_IMG_BYTES, head, d_out + i * head, lane, strm); }));
        ICL_HIP(ctx, hipEventRecord(ev, strm));
        if (ctx->embed_hook) { // rows [i, i + B) of d_out are complete once ev has fired
            const int hrc = ctx->embed_hook(i, B, ev);
            if (hrc) { // (leave the lanes the way a completed loop does: the side streams joined)
                (void)join();
                return hrc;
            }
        }
    }
    ICL_HIP(ctx, join());
    ICL_HIP(ctx, hipEventRecord(e1, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    ctx->last_embed_ms = ms;
    icl_prof_collect(ctx);
    return ICL_OK;
}

extern "C" int icl_embed_u8_dev(icl_ctx *ctx, const uint8_t *d_img, int64_t n, int head, int prec, float *d_out)
{
    if (!ctx || n < 0 || (n && (!d_img || !d_out))) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_u8_dev: bad argument");
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return icl_embed_dev_locked(ctx, d_img, n, head, prec, d_out);
}

extern "C" int icl_embed_u8(icl_ctx *ctx, const uint8_t *img, int64_t n, int head, int prec, float *out)
{
    if (!ctx || n < 0 || (n && (!img || !out))) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_u8: bad argument");
    if (!head_ok(head)) return icl_fail(ctx, ICL_ERR_ARG, "head must be 2048 or 1000");
    if (n == 0) return ICL_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    // Stream the images through in slabs of at most 4096, so host-side callers never need N*150 KB of HBM at once, with two slab
    // buffers: a helper thread uploads slab i+1 on its own stream (pageable host memory is staged by the runtime, which keeps the
    // calling thread busy for the whole copy) while the forward passes of slab i run -- the PCIe-inclusive rate of DESIGN.md 5.
    const int64_t slab = std::min<int64_t>(n, 4096);
    const int nbuf = n > slab ? 2 : 1;
    hip_guard<hipStream_t, hipStreamDestroy> g_cs; // (declared first: destroyed behind the buffers)
    dev_guard g_img[2], g_out;
    ICL_HIP(ctx, hipStreamCreateWithFlags(&g_cs.p, hipStreamNonBlocking));
    for (int q = 0; q < nbuf; ++q) ICL_TRY(icl_dev_alloc(ctx, g_img[q], (size_t)slab * ICL_IMG_BYTES, "embed image slab (%lld images)", (long long)slab));
    ICL_TRY(icl_dev_alloc(ctx, g_out, (size_t)slab * head * 4, "embed output buffer"));
    uint8_t *const d_img[2] = {g_img[0].as<uint8_t>(), g_img[1].as<uint8_t>()};
    float *const d_out = g_out.as<float>();
    const hipStream_t cs = g_cs.p;
    auto upload = [&](int64_t i, uint8_t *dst) -> hipError_t {
        const int64_t cnt = std::min(slab, n - i);
        hipError_t e = hipMemcpyAsync(dst, img + i * ICL_IMG_BYTES, (size_t)cnt * ICL_IMG_BYTES, hipMemcpyHostToDevice, cs);
        return e == hipSuccess ? hipStreamSynchronize(cs) : e;
    };
    hipError_t e = upload(0, d_img[0]);
    if (e != hipSuccess) return icl_fail(ctx, ICL_ERR_HIP, "image upload: %s", hipGetErrorString(e));
    int rc = ICL_OK;
    double total_ms = 0;
    int64_t k = 0;
    for (int64_t i = 0; rc == ICL_OK && i < n; i += slab, ++k) {
        const int64_t cnt = std::min(slab, n - i), inext = i + slab;
        hipError_t e_up = hipSuccess;
        std::thread up;
        if (inext < n) {
            uint8_t *dst = d_img[(k + 1) & 1]; // last read by slab k-1, which has finished
            try {
                up = std::thread([&, inext, dst] {
                    (void)hipSetDevice(ctx->device);
                    e_up = upload(inext, dst);
                });
            } catch (...) { // no thread to be had: upload in line
                e_up = upload(inext, dst);
            }
        }
        rc = icl_embed_dev_locked(ctx, d_img[k & 1], cnt, head, prec, d_out);
        total_ms += ctx->last_embed_ms;
        if (rc == ICL_OK) {
            e = hipMemcpyAsync(out + i * head, d_out, (size_t)cnt * head * 4, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) rc = icl_fail(ctx, ICL_ERR_HIP, "embedding copy-back: %s", hipGetErrorString(e));
        }
        if (up.joinable()) up.join();
        if (rc == ICL_OK && e_up != hipSuccess) rc = icl_fail(ctx, ICL_ERR_HIP, "image upload: %s", hipGetErrorString(e_up));
    }
    ctx->last_embed_ms = total_ms;
    return rc;
}

