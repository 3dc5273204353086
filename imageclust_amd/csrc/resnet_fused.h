// resnet_fused.h -- cross-layer fusions of the ResNet50-v1 forward pass (included by resnet.hip).
//
// The reference's forward pass (internal/embeddings/embeddings.go:141, Net.Forward inside OpenCV-DNN) fuses layers
// internally; the unfused graph of this engine is HBM-bound in its first quarter: the 112x112 stem output and
// the 56x56 stage-1 tensors are each written once and read back once per layer.  Two kernels remove those round trips:
//
//   stem_pool_kernel  conv0 7x7/2 + BN + ReLU + maxpool 3x3/2 in one launch: the 411 MB stem output never reaches HBM.
//   bneck56_kernel    one whole stage-1 bottleneck (1x1 -> 3x3 -> 1x1 (+ residual | + downsample branch) + ReLU) per
//                     launch: reads the block input once, writes the block output once (1 645 -> 822 MB per block).
#pragma once
#include "conv_select.h"
#include "mfma_tile.h"
#include "resnet_model.h" // (resnet_pack.h:) STEM_K, STEM_ROWK, ST2_K, the weight layouts the loader packs

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(const uint4 &a, const uint4 &b, const f32x4 &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
// Raw buffer descriptor over [base, base + bytes): 32-bit byte offsets, and the hardware's range check does the masking -- a lane
// whose offset is out of range (BN56_OOB) loads nothing that matters and stores nothing, while the INSTRUCTION is still issued, so
// the number of vector-memory operations between two counted waits is exact and no lane needs an address select.
#define BN56_OOB 0x80000000u
__device__ __forceinline__ i32x4_t bn56_srd(const void *base, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)base;
    i32x4_t r;
    r.x = (int)(unsigned)a;
    r.y = (int)(unsigned)(a >> 32);
    r.z = (int)bytes;
    r.w = 0x00020000;
    return r;
}
// LDS-DMA piece through a descriptor: 64 lanes x 16 B -> 1 KiB at the wave-uniform LDS byte address lds_dst; the source of lane l
// is base + soff + voff(l).  (s_nop 4: the scalar operands were written by SALU instructions the assembler cannot see.)
__device__ __forceinline__ void bload_lds16_asm(const i32x4_t &srd, unsigned voff, unsigned soff, unsigned lds_dst)
{
    unsigned keep;
    // (readfirstlane: under scalar-register pressure hipcc keeps wave-uniform values in vector registers)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(srd), "s"(__builtin_amdgcn_readfirstlane(soff)), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
                 : "memory");
}
#ifndef BN56_YSTORE_MOD
#define BN56_YSTORE_MOD "" /* cache policy of the bottleneck kernel's output stores (A/B knob: " sc1" drops the line from the XCD's L2, " nt") */
#endif
// one 16-byte store through a descriptor (the trailing s_nop: hipcc may otherwise overwrite the data registers before the store has read them)
__device__ __forceinline__ void bstore16_asm(const i32x4_t &srd, unsigned voff, unsigned soff, const uint4 &v)
{
    const u32x4_t x = __builtin_bit_cast(u32x4_t, v);
    asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, %3 offen" BN56_YSTORE_MOD "\n\ts_nop 1" ::"v"(x), "v"(voff), "s"(srd), "s"(__builtin_amdgcn_readfirstlane(soff)) : "memory");
}
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short i16x2_t __attribute__((ext_vector_type(2)));
// relu(a), relu(b) rounded to bf16 and packed: ONE v_cvt_pk_bf16_f32 (round to nearest even) and ONE v_pk_max_i16 -- a negative
// bf16 is a negative int16, so max(., 0) on the packed halves is the ReLU of both (-0 -> +0); rounding is monotonic, so
// relu-after-round equals round-after-relu bit for bit
__device__ __forceinline__ uint32_t pack_relu_bf16x2(float a, float b)
{
    const f32x2_t f{a, b};
    const bf16x2_t h = __builtin_convertvector(f, bf16x2_t);
    const i16x2_t r = __builtin_elementwise_max(__builtin_bit_cast(i16x2_t, h), i16x2_t{0, 0});
    return __builtin_bit_cast(uint32_t, r);
}

// ------------------------------------------------------------------------------------------------------------
// Stem + maxpool.  Work unit = (image, strip): a strip is 16 conv columns (14s-1 .. 14s+14, 15 of them used) =
// 7 pooled columns, so 8 strips cover the 56 pooled columns (1.14x recompute of the stem along x, none along y).
// A persistent workgroup walks a unit's 14 tiles of 8 conv rows top to bottom; tile t yields the pooled rows
// 4t .. 4t+3, whose windows need the conv rows 8t-1 .. 8t+7: the last conv row of a tile is kept in LDS for
// the next one.  Pooling takes the maximum of the ROUNDED conv outputs (rounding is monotonic: equal to rounding the
// maximum), so the result is bit-identical to conv0 -> store -> maxpool_kernel in both precisions.
// ------------------------------------------------------------------------------------------------------------
#define STEM_PW 120          /* patch row stride in bytes: 1 (alignment) + 37 pixels * 3 = 112, + slack for the padded slots, 4-aligned */
#define STEM_PH 21
#define SP_STRIPS 8
#define SP_TILES 14

template <typename T>
static constexpr size_t stem_pool_lds_bytes()
{
    // [weights][2 activation buffers == pool tile][input patch][fp32 epilogue half tile][2 carried conv rows]
    return (((size_t)(STEM_K / T::BK) * 64 * CV_ROWB + 2 * (size_t)CV_BM * CV_ROWB + STEM_PH * STEM_PW + 16 + 15) & ~(size_t)15) + (size_t)64 * (64 + 4) * 4 +
           2 * 16 * 64 * sizeof(typename T::elem);
}

// SPLIT (ICL_PREC_BF16X3, T = F32): the f32 stem, its pooled output written in the split bf16 layout (mfma_tile.h, BF16X3)
template <typename T, bool SPLIT = false>
__global__ __launch_bounds__(256) void stem_pool_kernel(const uint8_t *__restrict__ img, const conv_args p, int nunits)
{
    typedef typename T::elem elem;
    constexpr int BN = 64;
    constexpr int NKS = STEM_K / T::BK;            // k-steps: 3 (bf16) or 6 (f32)
    constexpr int WST = BN * CV_ROWB;              // bytes of one weight k-step image
    constexpr int XST = CV_BM * CV_ROWB;
    constexpr int PATCH = STEM_PH * STEM_PW + 16;  // + slack: chunk reads run past a row's last pixel
    constexpr int PROW = 64 * (int)sizeof(elem);   // one conv pixel's 64 channels in the pool tile
    static_assert(CV_BM * PROW <= 2 * XST, "the pool tile lives in the activation buffers");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *ptile = smem + NKS * WST; // 8 x 16 conv pixels after BN + ReLU, rounded (aliases the activation buffers)
    unsigned char *patch = smem + NKS * WST + 2 * XST;
    unsigned char *ep_smem = smem + ((NKS * WST + 2 * XST + PATCH + 15) & ~15);
    unsigned char *carry = ep_smem + 64 * (BN + 4) * 4; // [2][16 columns][64 channels]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wm = wid & 1, wn = wid >> 1;
    const elem *Wg = (const elem *)p.Wt;
    {   // all weights (64 x 192) by LDS-DMA, once per workgroup
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
    // input patch of tile (unit = image * 8 + strip, t): rows iy = 16t-3 .. +20, byte columns 3*(28s-5) .. ; zero outside the
    // image.  The first byte column, 84s - 15, is 1 mod 4 for every strip and rows / images are 672 / 150528 bytes apart, so the
    // patch is fetched as ALIGNED dwords from byte column 84s - 16 on and the chunk addresses below carry the 1-byte offset.
    constexpr int RW = STEM_PW / 4; // dwords per patch row
    static_assert(STEM_PW % 4 == 0, "patch rows are whole dwords");
    constexpr int NDW = STEM_PH * RW + 4;
    constexpr int NV = (NDW + 255) / 256;
    uint32_t pv[NV];
    auto patch_fetch = [&](int unit, int t) {
        const uint8_t *ib = img + (int64_t)(unit >> 3) * (int64_t)ICL_IMG_BYTES;
        const int iy0 = t * 16 - 3, bx0 = 84 * (unit & 7) - 16;
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
                const int addr = (oyl * 2 + kh) * STEM_PW + oxl * 6 + r0 + 1; // + 1: the patch starts 1 byte left of the tile
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
    // epilogue roles (conv_epilogue's): one 16-byte channel chunk per lane
    constexpr int CPR = BN / T::KE, RPP = 256 / CPR, NPASS = 64 / RPP, EP_LD = BN + 4;
    const int nl = (tid % CPR) * T::KE;
    float sc[T::KE], sh[T::KE];
#pragma unroll
    for (int q = 0; q < T::KE; q += 4) {
        const float4 a4 = *reinterpret_cast<const float4 *>(p.scale + nl + q);
        const float4 b4 = *reinterpret_cast<const float4 *>(p.shift + nl + q);
        sc[q] = a4.x; sc[q + 1] = a4.y; sc[q + 2] = a4.z; sc[q + 3] = a4.w;
        sh[q] = b4.x; sh[q + 1] = b4.y; sh[q + 2] = b4.z; sh[q + 3] = b4.w;
    }
    float *ep = reinterpret_cast<float *>(ep_smem);
    elem *Yg = (elem *)p.Y; // pooled output [B][56][56][64]

    int unit = blockIdx.x, t = 0;
    if (unit >= nunits) return;
    patch_fetch(unit, t);
    patch_store();
    __syncthreads();
    for (;;) {
        int nt = t + 1, nu = unit;
        if (nt == SP_TILES) {
            nt = 0;
            nu = unit + (int)gridDim.x;
        }
        const bool has_next = nu < nunits; // workgroup-uniform
        f32x16 acc[1][2];
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[0][bb][r] = 0.0f;
        gather(0, 0);
        if (has_next) patch_fetch(nu, nt); // in flight while this tile is computed
        __syncthreads();                   // (the first time: also drains the weight DMA)
#pragma unroll
        for (int j = 0; j < NKS; ++j) {
            if (j + 1 < NKS) gather(j + 1, (j + 1) & 1);
            conv_mma_kstep<T, BN>(smem + j * WST, smem + NKS * WST + (j & 1) * XST, wm, wn, fr, fh, acc);
            __syncthreads();
        }
        if (has_next) patch_store(); // every gather of this tile has read the patch
        // ---- epilogue: BN + ReLU, rounded, into the pool tile (row r = conv pixel (r >> 4, r & 15) of the tile); the tile's
        // last conv row also goes to the carry buffer of the next tile
        unsigned char *carry_cur = carry + (t & 1) * 16 * PROW, *carry_nxt = carry + ((t + 1) & 1) * 16 * PROW;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (half) __syncthreads();
            if (wm == half) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int ml = b * 32 + fr;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nn = wn * 32 + 8 * g + 4 * fh;
                        *reinterpret_cast<float4 *>(ep + ml * EP_LD + nn) =
                            make_float4(acc[0][b][4 * g + 0], acc[0][b][4 * g + 1], acc[0][b][4 * g + 2], acc[0][b][4 * g + 3]);
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPASS; ++i) {
                const int ml = tid / CPR + i * RPP;
                const int r = half * 64 + ml;
                float v[T::KE];
#pragma unroll
                for (int q = 0; q < T::KE; q += 4) {
                    const float4 tt = *reinterpret_cast<const float4 *>(ep + ml * EP_LD + nl + q);
                    v[q] = tt.x * sc[q] + sh[q];
                    v[q + 1] = tt.y * sc[q + 1] + sh[q + 1];
                    v[q + 2] = tt.z * sc[q + 2] + sh[q + 2];
                    v[q + 3] = tt.w * sc[q + 3] + sh[q + 3];
                }
                if (p.relu) {
#pragma unroll
                    for (int q = 0; q < T::KE; ++q) v[q] = fmaxf(v[q], 0.0f);
                }
                uint4 ov;
                elem *oe = reinterpret_cast<elem *>(&ov);
#pragma unroll
                for (int q = 0; q < T::KE; ++q) oe[q] = T::from_f(v[q]);
                *reinterpret_cast<uint4 *>(ptile + r * PROW + nl * (int)sizeof(elem)) = ov;
                if ((r >> 4) == 7) *reinterpret_cast<uint4 *>(carry_nxt + (r & 15) * PROW + nl * (int)sizeof(elem)) = ov;
            }
        }
        __syncthreads(); // the pool tile is complete
        // ---- maxpool 3x3/2 p1 (padding never wins): pooled rows 4t .. 4t+3, pooled columns 7s .. 7s+6
        {
            const int s = unit & 7;
            const int64_t b = unit >> 3;
            for (int it = tid; it < 28 * CPR; it += 256) {
                const int ch = it % CPR, pix = it / CPR, pr = pix / 7, pc = pix - 7 * pr;
                float best[T::KE];
#pragma unroll
                for (int e = 0; e < T::KE; ++e) best[e] = -INFINITY;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int rr = 2 * pr + kh; // 0: the carried conv row 8t-1; 1 .. 8: this tile's rows
                    if (rr == 0 && t == 0) continue;
                    const unsigned char *rowp = rr == 0 ? carry_cur : ptile + (rr - 1) * 16 * PROW;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int ci = 2 * pc + kw; // conv column 14s - 1 + ci
                        if (s == 0 && ci == 0) continue;
                        const uint4 raw = *reinterpret_cast<const uint4 *>(rowp + ci * PROW + ch * 16);
                        const elem *pvv = reinterpret_cast<const elem *>(&raw);
#pragma unroll
                        for (int e = 0; e < T::KE; ++e) {
                            const float f = T::to_f(pvv[e]);
                            if (f > best[e]) best[e] = f;
                        }
                    }
                }
                const int64_t opix = (b * 56 + 4 * t + pr) * 56 + 7 * s + pc;
                if constexpr (SPLIT) {
                    static_assert(T::KE == 4, "4 fp32 channels per lane");
                    uint16_t oh[4], ol[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) BF16X3::split(best[e], oh[e], ol[e]);
                    const int c = ch * 4;
                    uint16_t *yo = reinterpret_cast<uint16_t *>(p.Y) + opix * 128 + c + (c & ~31);
                    *reinterpret_cast<uint2 *>(yo) = *reinterpret_cast<const uint2 *>(oh);
                    *reinterpret_cast<uint2 *>(yo + 32) = *reinterpret_cast<const uint2 *>(ol);
                } else {
                    elem o[T::KE];
#pragma unroll
                    for (int e = 0; e < T::KE; ++e) o[e] = T::from_f(best[e]);
                    *reinterpret_cast<uint4 *>(Yg + opix * 64 + ch * T::KE) = *reinterpret_cast<const uint4 *>(o);
                }
            }
        }
        if (!has_next) break;
        unit = nu;
        t = nt;
        __syncthreads(); // the next patch is in LDS; the pool tile (activation buffer 0) and the epilogue tile are free again
    }
}

// ------------------------------------------------------------------------------------------------------------
// Stem + maxpool, bf16, WITHOUT an im2col staging pass (stem_pool_kernel above cuts every 16-byte A chunk out of the u8 patch
// again for each of the 128 x 147 products' operands: ~480 vector instructions per thread and tile around 12 MFMAs -- the
// pass's kernel furthest from its roofline).  Here the input patch is converted ONCE per tile to bf16 pixels padded to four
// channels (R, G, B, 0: 8 bytes), and the implicit GEMM runs with K ordered (kh, kw padded to 8, channel padded to 4) = 7 k-steps
// of 32: the B operand of v_mfma_f32_16x16x32_bf16 for conv pixel (oy, ox), k-step kh, lane quarter q is the 16 bytes
//   patch[2 oy + kh][2 ox + 2q .. 2 ox + 2q + 1][0..3],
// contiguous and 16-byte aligned for every lane -- read straight from the patch, each patch row fragment once per tile and used
// by up to four (oy, kh) pairs.  The weights (64 x 224, BatchNorm scale folded in, zero in the padding) sit in registers: wave w
// owns the output channels 16w .. 16w+15 for all 128 pixels of a tile; the shift is the accumulator's initial value.
// Tile walk, carried conv row and pooling as in stem_pool_kernel.  Pixels are byte / 255 rounded to bf16, as before.
// ------------------------------------------------------------------------------------------------------------
#define ST2_PW 40            /* patch row: 37 pixels used (+ the kw padding's reach), 8 bytes each */
#define ST2_RAWW 120         /* raw u8 patch row stride (as STEM_PW) */
static constexpr size_t stem2_lds_bytes()
{
    // [raw u8 patch][bf16 RGBX patch: 21 rows + 1 of slack][pool tile: 8 x 16 conv pixels x 64 channels][2 carried conv rows]
    return (size_t)((STEM_PH * ST2_RAWW + 16 + 15) & ~15) + (size_t)(STEM_PH + 1) * ST2_PW * 8 + (size_t)128 * 128 + 2 * 16 * 128;
}

__global__ __launch_bounds__(256) void stem2_pool_kernel(const uint8_t *__restrict__ img, const uint16_t *__restrict__ W2k /* [64][224] */,
                                                        const float *__restrict__ shift, uint16_t *__restrict__ Yg /* [B][56][56][64] */, int nunits)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int RAWB = (STEM_PH * ST2_RAWW + 16 + 15) & ~15;
    unsigned char *raw = smem;
    unsigned char *pbf = smem + RAWB;                            // [22][40] pixels x 8 bytes
    unsigned char *ptile = pbf + (STEM_PH + 1) * ST2_PW * 8;     // [128 pixels][128 B], 16-byte slots XOR-swizzled by (pixel >> 1) & 7
    unsigned char *carry = ptile + 128 * 128;                    // [2][16 pixels][128 B], same swizzle
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    uint4 wr[7];
#pragma unroll
    for (int kh = 0; kh < 7; ++kh) wr[kh] = *reinterpret_cast<const uint4 *>(W2k + (size_t)(16 * w + r16) * ST2_K + 32 * kh + 8 * q);
    const float4 hf = *reinterpret_cast<const float4 *>(shift + 16 * w + 4 * q);
    const f32x4 hv = f32x4{hf.x, hf.y, hf.z, hf.w};
    const int swc = (r16 >> 1) & 7;
    const unsigned boff = (unsigned)((2 * r16 + 2 * q) * 8);     // this lane's B fragment inside a patch row
    const unsigned toff = (unsigned)(r16 * 128 + ((((2 * w + (q >> 1)) ^ swc) & 7) << 4) + 8 * (q & 1));
    // raw patch of tile (unit = image * 8 + strip, t), fetched as aligned dwords (stem_pool_kernel's scheme)
    constexpr int RW = ST2_RAWW / 4, NDW = STEM_PH * RW + 4, NV = (NDW + 255) / 256;
    uint32_t pv[NV];
    auto patch_fetch = [&](int unit, int t) {
        const uint8_t *ib = img + (int64_t)(unit >> 3) * (int64_t)ICL_IMG_BYTES;
        const int iy0 = t * 16 - 3, bx0 = 84 * (unit & 7) - 16;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = tid + k * 256;
            const int pr = i / RW, pc = i - pr * RW;
            const int iy = iy0 + pr, bx = bx0 + pc * 4;
            const bool ok = i < NDW && pr < STEM_PH && (unsigned)iy < 224u && (unsigned)bx < 672u;
            pv[k] = ok ? *reinterpret_cast<const uint32_t *>(ib + iy * 672 + bx) : 0u;
        }
    };
    auto patch_store = [&]() {
        uint32_t *p32 = reinterpret_cast<uint32_t *>(raw);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = tid + k * 256;
            if (i < NDW) p32[i] = pv[k];
        }
    };
    const float sc255 = (float)(1.0 / 255.0);
    auto convert = [&]() { // raw bytes -> bf16 RGBX pixels (the raw patch starts 1 byte left of the tile's first pixel)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + k * 256;
            if (i < STEM_PH * ST2_PW) {
                const int pr = i / ST2_PW, pc = i - pr * ST2_PW;
                uint2 o = make_uint2(0u, 0u);
                if (pc < 38) {
                    const int addr = pr * ST2_RAWW + pc * 3 + 1;
                    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(raw + (addr & ~3));
                    const uint32_t v3 = __builtin_amdgcn_alignbyte(w32[1], w32[0], addr & 3);
                    const float r = (float)(v3 & 0xffu) * sc255, g = (float)((v3 >> 8) & 0xffu) * sc255, b = (float)((v3 >> 16) & 0xffu) * sc255;
                    o.x = (uint32_t)BF16::from_f(r) | ((uint32_t)BF16::from_f(g) << 16);
                    o.y = (uint32_t)BF16::from_f(b);
                }
                *reinterpret_cast<uint2 *>(pbf + i * 8) = o;
            }
        }
    };
    int unit = blockIdx.x, t = 0;
    if (unit >= nunits) return;
    if (tid < ST2_PW) *reinterpret_cast<uint2 *>(pbf + (STEM_PH * ST2_PW + tid) * 8) = make_uint2(0u, 0u); // the slack row
    patch_fetch(unit, t);
    patch_store();
    __syncthreads();
    for (;;) {
        int nt = t + 1, nu = unit;
        if (nt == SP_TILES) {
            nt = 0;
            nu = unit + (int)gridDim.x;
        }
        const bool has_next = nu < nunits; // workgroup-uniform
        convert();
        if (has_next) patch_fetch(nu, nt); // in flight while this tile is computed
        __syncthreads();                   // the bf16 patch is complete; the raw patch may be overwritten
        if (has_next) patch_store();
        // ---- conv0: 8 output rows x 16 columns x this wave's 16 channels; patch row r feeds (oy, kh) with 2 oy + kh = r
        f32x4 acc[8];
#pragma unroll
        for (int r = 0; r < STEM_PH; ++r) {
            const uint4 bf = *reinterpret_cast<const uint4 *>(pbf + r * (ST2_PW * 8) + boff);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int kh = r - 2 * m;
                if (kh >= 0 && kh < 7) acc[m] = mfma16(wr[kh], bf, kh == 0 ? hv : acc[m]);
            }
        }
        // ---- ReLU, rounded, into the pool tile; the tile's last conv row also goes to the carry buffer of the next tile
        unsigned char *carry_cur = carry + (t & 1) * 2048, *carry_nxt = carry + ((t + 1) & 1) * 2048;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            uint2 o;
            o.x = pack_relu_bf16x2(acc[m][0], acc[m][1]);
            o.y = pack_relu_bf16x2(acc[m][2], acc[m][3]);
            *reinterpret_cast<uint2 *>(ptile + m * 2048 + toff) = o;
            if (m == 7) *reinterpret_cast<uint2 *>(carry_nxt + toff) = o;
        }
        __syncthreads(); // the pool tile is complete
        // ---- maxpool 3x3/2 p1: pooled rows 4t .. 4t+3, pooled columns 7s .. 7s+6; one 16-byte chunk per thread.  Every value in the
        // tile is a ReLU output, i.e. a non-negative bf16, whose bit pattern orders like a signed 16-bit integer: the maximum is
        // taken on the packed halves (v_pk_max_i16), and 0 stands for the padding, which never wins
        if (tid < 28 * 8) {
            const int s = unit & 7;
            const int64_t b = unit >> 3;
            const int ch = tid & 7, pix = tid >> 3, pr = pix / 7, pc = pix - 7 * pr;
            i16x2_t best[4] = {i16x2_t{0, 0}, i16x2_t{0, 0}, i16x2_t{0, 0}, i16x2_t{0, 0}};
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int rr = 2 * pr + kh; // 0: the carried conv row 8t-1; 1 .. 8: this tile's rows
                if (rr == 0 && t == 0) continue;
                const unsigned char *rowp = rr == 0 ? carry_cur : ptile + (rr - 1) * 2048;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int ci = 2 * pc + kw; // conv column 14s - 1 + ci
                    if (s == 0 && ci == 0) continue;
                    const uint4 rawv = *reinterpret_cast<const uint4 *>(rowp + ci * 128 + (((ch ^ (ci >> 1)) & 7) << 4));
                    best[0] = __builtin_elementwise_max(best[0], __builtin_bit_cast(i16x2_t, rawv.x));
                    best[1] = __builtin_elementwise_max(best[1], __builtin_bit_cast(i16x2_t, rawv.y));
                    best[2] = __builtin_elementwise_max(best[2], __builtin_bit_cast(i16x2_t, rawv.z));
                    best[3] = __builtin_elementwise_max(best[3], __builtin_bit_cast(i16x2_t, rawv.w));
                }
            }
            const uint4 o = make_uint4(__builtin_bit_cast(uint32_t, best[0]), __builtin_bit_cast(uint32_t, best[1]), __builtin_bit_cast(uint32_t, best[2]),
                                       __builtin_bit_cast(uint32_t, best[3]));
            *reinterpret_cast<uint4 *>(Yg + ((b * 56 + 4 * t + pr) * 56 + 7 * s + pc) * 64 + ch * 8) = o;
        }
        if (!has_next) break;
        unit = nu;
        t = nt;
        __syncthreads(); // the next raw patch is in LDS; the pool tile is free again
    }
}

// ------------------------------------------------------------------------------------------------------------
// One stage-1 bottleneck per launch (bf16):  y = relu(bn3(conv3(relu(bn2(conv2_3x3(relu(bn1(conv1(x))))))) + x)           [identity]
//                                            y = relu(bn3(conv3(t2)) + bn_ds(conv_ds(x)))                               [DS: block 0]
// mid = 64 channels, Cout = 256, Cin = 256 (identity) or 64 (DS); any H, W.  Every BatchNorm scale is folded into the bf16
// weights at load time (W' = bf16(W * scale), as an inference engine does; the downsample fusion of round 1 already did), the
// shift is the accumulator's initial value: the epilogues are ReLU + convert only.
//
//   * One 512-thread workgroup per CU, two waves per SIMD.  Every WEIGHT lives in registers for the whole launch -- no weight
//     byte crosses L2 -> LDS after the prologue -- as A operands of v_mfma_f32_16x16x32_bf16; activations are the B operand, read
//     from LDS.  The waves form a two-stage pipeline inside the workgroup:
//       front waves 0..3 (W1, W2: rows 16w .. 16w+15): conv1 and conv2 of step j        -> t2[j & 1] in LDS
//       back  waves 4..7 (W3: rows 64b .. 64b+63):     conv3 + residual / downsample + ReLU + stores of step j-1
//     so on each SIMD an MFMA-heavy wave runs beside an epilogue-heavy one (alone on its SIMD a wave is bound by instruction issue:
//     ~10 vector / scalar instructions per 16-cycle MFMA; measured 13.7 us per step for the one-wave-per-SIMD form of this kernel).
//   * A workgroup owns a strip of 14 output columns of a run of images and walks it top to bottom in steps of BN56_ROWS = 4 rows.
//     The images of a run are stacked with ONE zero row between them (a "virtual" row index v: image v / (H+1), row v % (H+1),
//     row H = padding), so the walk never restarts: step j brings the x tile of virtual rows S+4j .. S+4j+3 (16 columns:
//     the strip + one halo column each side) in by LDS-DMA, conv1 turns it into 4 new rows of t1 behind the two rows kept
//     from the previous step (no halo recompute along y, 16/14 along x), conv2 produces t2 for the virtual rows
//     S+4j-1 .. S+4j+2 from the 6 t1 rows, conv3 (+ residual / + downsample operand, both B fragments read from the x tiles in
//     LDS) writes y.  t1 and t2 never leave the CU; every byte of x is read from global memory ONCE, by the front waves' DMA.
//   * Three workgroup barriers per step (D: t2 / x tile complete, E: conv1 has read the x tile and the kept t1 rows are moved,
//     C: t1 written); the back waves work on one half of their step (a "quarter": 2 rows) between D and E and on the other
//     between C and D.
//   * The x tiles form a RING OF THREE slots (tile j lives in slot j % 3), because the back waves need x one step after conv1:
//     the outputs of step j-1 are the virtual rows S+4(j-1)-1 .. S+4(j-1)+2 = row 3 of tile j-2 and rows 0..2 of tile j-1.
//     Iteration j, in barrier order  D(j-1) | E(j) | C(j) | D(j):
//         front   conv1 reads tile j          | DMA of tile j+1 issued, t1 written | conv2, vmcnt(0)  |
//         back    quarter 1: tile j-2 row 3,  |                                    | quarter 2: tile  |
//                 tile j-1 row 0              |                                    | j-1 rows 1, 2    |
//     Slot (j+1) % 3 == (j-2) % 3, written by the DMA behind E(j):
//       WAR  its last reader is the back waves' quarter 1 of iteration j (tile j-2, row 3).  Those ds_reads retire before the
//            back wave arrives at E(j) (bn56_barrier waits for lgkmcnt(0)), and no DMA is issued before every wave has arrived.
//            (conv1 read tile j-2 two steps ago; quarter 1 / 2 of iteration j-1 read its rows 0..2 before D(j-1).)
//       RAW  every front wave waits for vmcnt(0) -- its own pieces -- before it arrives at D(j); the first readers of tile j+1
//            (conv1 of step j+1, quarter 1 of iteration j+2) run behind D(j) / D(j+1).
//     Slot (j-1) % 3 and slot j % 3 are only read in iteration j: the next write to slot (j-1) % 3 is tile j+2, issued behind
//     E(j+1), i.e. after D(j), which quarter 2 of iteration j precedes; the next write to slot j % 3 is tile j+3.
//     Nothing is carried in registers across a barrier and no wait is counted: the back waves issue no loads from global memory.
//     (Iteration 1 reads "tile -1" from slot 2, which nothing has written: that row is the padding row above the run, never stored.
//     Whatever LDS held there, NaN patterns included, stays in that row: a B column of the MFMA is one pixel, and columns do not mix.)
//   k order per output element: channels ascending for the 1x1s, (row, kw, channel) for the 3x3, [t2 | x] for conv3: fixed,
//   so results do not depend on the batch, on the strip decomposition or on the step height.
//   * The PRUNED form, bneck56_kernel<false, 2> (the last identity block in front of a block 0 that reads at stride 2: forward_make_plan,
//     prune_map.h): only the pixels (2 oy, 2 ox) of y are computed behind conv1 and stored; every other pixel of y keeps what the buffer held.
//     Strip walk, ring, barriers (D | E | C | D, 3 nsteps + 3 in both wave groups), the WAR / RAW argument, the DMA and conv1 with its t1
//     epilogue are the code above, unchanged.
//       rows     a virtual row is needed if its image row t.r is even and t.r < H (bn56_row_needed), read off the bn56_row cursor -- never
//                off the step index: images are stacked at H + 1 rows, so the parity of a virtual row flips from one image of a run to the
//                next, and around an image boundary the pattern inside a step shifts.  Two rows in a row are never both needed, so a step
//                has at most two needed rows (bn56_step_rows) and a quarter at most one (bn56_quarter_row); both are wave-uniform.
//       front    conv2 accumulates and writes t2 for the step's two rows only: units (kh, k half) of 3 fragments (kw) per row, i.e. the sum
//                order (kh, k half, kw) of the unpruned loop; 36 MFMAs instead of 72.  With fewer than two needed rows the spare index
//                names an unneeded row, whose t2 nobody reads: no branch in the loop.  The other t2 rows hold what an earlier step left.
//       back     a quarter computes conv3, the selector-MFMA residual, the ReLU and the OT write for its needed row (12 MFMAs instead of
//                24; none and no store for a quarter without one, e.g. (row 55, padding)); the barriers stand outside the quarter.
//       columns  c0 = 14 strip is even, so the even image columns are the even strip columns.  OT holds the row with the even columns first
//                (see aoff2 below), and ONE buffer_store_dwordx4 carries them: 8 lanes per pixel's 128 B, strip columns 0, 2, .. 12, lanes
//                56..63 ("column 14") and columns outside the image out of range (BN56_OOB) -- one store per quarter instead of four, each
//                lane group a whole 128-byte line of a pixel that is read.
//     The values that are stored are the unpruned kernel's bit for bit (tests/test_bneck56_pruned_gpu.py); which pixels those are is walked on
//     the host against the triple loop (tests/bneck56_needed_main.cpp).
// ------------------------------------------------------------------------------------------------------------
// in-kernel segment timers for tuning (a separate diagnostic build: -DBN56_TIMERS; launch_bneck56 prints them when BN56_PRINT is set)
#ifdef BN56_TIMERS
#define BN56_STAMP(k)                                                                              \
    do {                                                                                           \
        unsigned long long t__;                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t__)::"memory");                \
        __builtin_amdgcn_sched_barrier(0);                                                         \
        tacc[k] += t__ - tlast;                                                                    \
        tlast = t__;                                                                               \
    } while (0)
#define BN56_TIMER_DECL unsigned long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0
#define BN56_TIMER_START asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory")
#define BN56_TIMER_FLUSH(role)                                                                     \
    if (p.dbg && blockIdx.x == 0 && w == 0 && lane == 0)                                            \
        for (int k__ = 0; k__ < 8; ++k__) p.dbg[(role)*8 + k__] = tacc[k__]
// segment names, in stamp order (launch_bneck56 prints them)
#define BN56_FRONT_SEGMENTS {"carry+conv1", "wait E", "dma+t1 epi", "wait C", "conv2+t2 epi", "wait x", "wait D", ""}
#define BN56_BACK_SEGMENTS {"t2 + side reads", "MFMAs + epilogue", "read-back + stores", "barrier waits", "", "", "", ""}
#else
#define BN56_STAMP(k)
#define BN56_TIMER_DECL
#define BN56_TIMER_START
#define BN56_TIMER_FLUSH(role)
#endif

struct bneck_args {
    const uint16_t *X;  // [B][H][W][CIN]
    uint16_t *Y;        // [B][H][W][256]
    const uint16_t *W1; // [64][CIN]        * scale1
    const uint16_t *W2; // [64][3][3][64]   * scale2
    const uint16_t *W3; // identity: [256][64] * scale3; DS: [256][64 + 64] = [W3*scale3 | Wds*scale_ds]
    const float *sh1, *sh2, *sh3; // folded BN shifts (DS: sh3 = shift3 + shift_ds)
    int B, H, W;        // (B * H * W * 256 * 2 bytes < 2^31: 32-bit buffer offsets)
    int nstrips, ngroups; // grid = nstrips * ngroups; group g owns the images [g*B/ngroups, (g+1)*B/ngroups)
#ifdef BN56_TIMERS
    unsigned long long *dbg; // [2 roles][8 segments] cycles of workgroup 0 (front wave 0, back wave 4)
#endif
};

/* BN56_COLS (conv_select.h, where the forward plan sizes the grid): 14 output columns per strip */
#define BN56_ROWS 4                                  /* virtual rows per step: one x tile, 4 new t1 rows, 4 t2 rows, two quarters of output */
#define BN56_ROW_BYTES (16 * 128)                    /* one tile row: 16 pixels x 64 channels */
#define BN56_XCH_BYTES (BN56_ROWS * BN56_ROW_BYTES)  /* one 64-channel chunk of an x tile */
#define BN56_T1_BYTES ((2 + BN56_ROWS + 1) * BN56_ROW_BYTES) /* t1: 2 kept rows + the new ones + 1 row of slack for the garbage columns' taps */
#define BN56_T2_BYTES (BN56_ROWS * BN56_ROW_BYTES)
#define BN56_OT_BYTES (2 * BN56_ROW_BYTES)           /* a back wave's output tile: one quarter = 2 rows of its 64 channels */

template <bool DS>
static constexpr size_t bneck56_lds_bytes()
{
    return (size_t)3 * (DS ? 1 : 4) * BN56_XCH_BYTES + BN56_T1_BYTES + 2 * BN56_T2_BYTES + 4 * BN56_OT_BYTES; // ring of 3 x tiles, t1, t2[2], the back waves' output tiles
}

// workgroup barrier that waits for this wave's LDS traffic only (the front waves' LDS-DMA stays in flight across it; their own
// vmcnt(0) covers it before the barrier that publishes the tile)
__device__ __forceinline__ void bn56_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// (bn56_row, the (image, row) cursor of a virtual row, and the rules of the pruned form: prune_map.h)

template <bool DS, int SUB = 1>
__global__ __launch_bounds__(512, 2) void bneck56_kernel(const bneck_args p)
{
    static_assert(BN56_ROWS == 4, "the quarters below are rows {-1, 0} and {1, 2} of a 4-row step");
    static_assert(SUB == 1 || (SUB == 2 && !DS && BN56_COLS % 2 == 0), "the pruned form: an identity block read at stride 2; a strip starts at an even column");
    constexpr int CIN = DS ? 64 : 256;
    constexpr int NCH = CIN / 64;       // 64-channel chunks of x
    constexpr int K3 = DS ? 128 : 64;   // conv3's K: [t2 | x] or t2
    constexpr int RB = BN56_ROW_BYTES;
    constexpr unsigned SLOT = NCH * BN56_XCH_BYTES; // one x tile
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *XT = smem;                       // [3 slots][NCH][64 pixels][128 B], swizzled
    unsigned char *T1 = smem + 3 * SLOT;            // [7 rows][16 columns][128 B], swizzled
    unsigned char *T2 = T1 + BN56_T1_BYTES;         // [2][64 pixels][128 B], swizzled
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = wid & 3;
    const int r16 = lane & 15, q = lane >> 4;
    const int H = p.H, Wd = p.W, VH = H + 1;
    const int strip = (int)blockIdx.x % p.nstrips, grp = (int)blockIdx.x / p.nstrips;
    const int b0 = (int)(((int64_t)grp * p.B) / p.ngroups), b1 = (int)(((int64_t)(grp + 1) * p.B) / p.ngroups);
    if (b0 >= b1) return; // (workgroup-uniform: no wave of this workgroup reaches a barrier)
    const int c0 = strip * BN56_COLS;
    const int nsteps = ((b1 - b0) * VH + BN56_ROWS - 1) / BN56_ROWS;
    // B-fragment reads: pixel px = 16 * row + column; (px >> 1) & 7 depends on the column only, so a lane's swizzled byte
    // offset inside a pixel row is fixed and every (row, chunk) is an immediate offset
    const int swc = (r16 >> 1) & 7;
    unsigned xoff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) xoff[ks] = (unsigned)(r16 * 128 + ((((4 * ks + q) ^ swc) & 7) << 4));

    const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
    if (wid < 4) {
        // =========================================== front waves: conv1, conv2 ===========================================
        uint4 w1r[NCH * 2], w2r[18];
#pragma unroll
        for (int kk = 0; kk < NCH * 2; ++kk) w1r[kk] = *reinterpret_cast<const uint4 *>(p.W1 + (size_t)(16 * w + r16) * CIN + 32 * kk + 8 * q);
#pragma unroll
        for (int kk = 0; kk < 18; ++kk) w2r[kk] = *reinterpret_cast<const uint4 *>(p.W2 + (size_t)(16 * w + r16) * 576 + 32 * kk + 8 * q);
        const float4 h1f = *reinterpret_cast<const float4 *>(p.sh1 + 16 * w + 4 * q), h2f = *reinterpret_cast<const float4 *>(p.sh2 + 16 * w + 4 * q);
        const f32x4 h1 = f32x4{h1f.x, h1f.y, h1f.z, h1f.w}, h2 = f32x4{h2f.x, h2f.y, h2f.z, h2f.w}; // the shifts: C operand of a chain's first MFMA
        unsigned t1off[3][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int c = r16 + kw;
                t1off[kw][ks] = (unsigned)(c * 128 + ((((4 * ks + q) ^ (c >> 1)) & 7) << 4));
            }
        // t1 / t2 stores: this lane's 4 channels 16w + 4q .. of pixel (row, r16): 8 bytes in slot 2w + (q >> 1)
        const unsigned toff = (unsigned)(r16 * 128 + ((((2 * w + (q >> 1)) ^ swc) & 7) << 4) + 8 * (q & 1));
        const bool col_in = (unsigned)(c0 - 1 + r16) < (unsigned)Wd; // t1 column of this lane inside the image
        // LDS-DMA roles: wave w fills the tile row w (pieces of 8 pixels x 128 B): piece i of a row = columns 8i ..
        const int dcol = lane >> 3, dps = lane & 7;
        const unsigned xt_wave = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + (unsigned)w * (unsigned)RB);
        const i32x4_t xsrd = bn56_srd(p.X, (unsigned)((size_t)p.B * H * Wd * CIN * 2));
        const unsigned xrow_bytes = (unsigned)(Wd * CIN * 2);
        unsigned dvoff[2]; // byte offset of this lane's source chunk inside an image row (channel chunk 0), or out of range: column outside the image
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = 8 * i + dcol, col = c0 - 1 + c;
            dvoff[i] = (unsigned)col < (unsigned)Wd ? (unsigned)(col * CIN + ((dps ^ (c >> 1)) & 7) * 8) * 2u : BN56_OOB;
        }
        auto stage_x = [&](const bn56_row &t, unsigned slot) { // the tile row w of the x tile at byte offset `slot`; t = its virtual row
            const bool rok = t.b < b1 && t.r < H;
            const unsigned soff = rok ? (unsigned)t.p * xrow_bytes : 0u;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned vo = rok ? dvoff[i] : BN56_OOB;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) bload_lds16_asm(xsrd, vo, soff + (unsigned)(128 * ch), xt_wave + slot + (unsigned)(ch * BN56_XCH_BYTES + i * 1024));
            }
        };
        bn56_row cur{b0, 0, b0 * H}; // virtual row S + 4j: the first new t1 row of step j
        bn56_row dma = cur;          // ... + w: this wave's DMA row
        for (int i = 0; i < w; ++i) dma.step(VH);
        [[maybe_unused]] bn56_row o2{b0 - 1, H, b0 * H}; // SUB == 2: virtual row S + 4j - 1, the first t2 row of step j (the back waves' `out`)
        reinterpret_cast<uint4 *>(T1)[tid] = make_uint4(0, 0, 0, 0); // the two kept t1 rows of step 0: padding
        stage_x(dma, 0u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bn56_barrier(); // D
        unsigned xs = 0u; // byte offset of slot j % 3
        BN56_TIMER_DECL;
        BN56_TIMER_START;
#pragma unroll 1
        for (int j = 0; j < nsteps; ++j) {
            // ---- conv1: t1[rows 2..5] = relu(W1' . x + shift1).  The 4 B fragments of the k-step after next are requested before the
            // MFMAs of this one (alone, hipcc keeps two fragments in flight and every MFMA group waits out an LDS round trip)
            f32x4 a1[BN56_ROWS];
            {
                // units of 4 fragments (one k-step, the four tile rows), requested two units ahead of their MFMAs
                constexpr int NU = NCH * 2;
                const unsigned char *Xc = XT + xs;
                uint4 f[3][4];
                auto ld = [&](int kk, uint4 (&d)[4]) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) d[m] = *reinterpret_cast<const uint4 *>(Xc + (kk >> 1) * BN56_XCH_BYTES + m * RB + xoff[kk & 1]);
                };
                ld(0, f[0]);
                ld(1, f[1]);
#pragma unroll
                for (int kk = 0; kk < NU; ++kk) {
                    if (kk + 2 < NU) ld(kk + 2, f[(kk + 2) % 3]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a1[m] = mfma16(w1r[kk], f[kk % 3][m], kk == 0 ? h1 : a1[m]);
                }
            }
            BN56_STAMP(0); // conv1
            bn56_barrier(); // E: every front wave has read x tile j, every back wave row 3 of tile j-2; the kept rows are in place
            BN56_STAMP(1); // wait at E
            for (int i = 0; i < BN56_ROWS; ++i) dma.step(VH);
            const unsigned xn = xs + SLOT == 3 * SLOT ? 0u : xs + SLOT; // slot (j + 1) % 3: tile j-2 until now
            if (j + 1 < nsteps) stage_x(dma, xn);
            {
                bn56_row t = cur;
#pragma unroll
                for (int m = 0; m < BN56_ROWS; ++m) {
                    const bool ok = t.b < b1 && t.r < H && col_in; // conv2 pads t1 with zeros, not with relu(shift1)
                    uint2 o;
                    o.x = ok ? pack_relu_bf16x2(a1[m][0], a1[m][1]) : 0u;
                    o.y = ok ? pack_relu_bf16x2(a1[m][2], a1[m][3]) : 0u;
                    *reinterpret_cast<uint2 *>(T1 + (2 + m) * RB + toff) = o;
                    t.step(VH);
                }
                cur = t;
            }
            BN56_STAMP(2); // DMA issue + t1 epilogue
            bn56_barrier(); // C: t1 rows 2..5 are written
            BN56_STAMP(3); // wait at C
            // ---- conv2: t2 = relu(W2' * t1 + shift2): every t1 fragment (row R, kw, k half) is read once and feeds the taps kh = R - m;
            // the 3 fragments of the next unit are requested before the MFMAs of this one
            if constexpr (SUB == 2) {
                // Pruned form: t2 for the step's needed rows only -- at most two, bn56_step_rows (prune_map.h), from the cursor o2.  Row m of
                // the step takes the t1 rows m + kh: units (kh, k half) of 3 fragments (kw) per row, both rows' requested one unit ahead, so
                // an output element still sums in the order (kh, k half, kw) of the loop over u = (R, ks) below.  36 MFMAs instead of 72.
                const bn56_rows2 nr = bn56_step_rows(o2, H, VH, SUB);
                for (int i = 0; i < BN56_ROWS; ++i) o2.step(VH);
                const unsigned rowb[2] = {(unsigned)nr.a * (unsigned)RB, (unsigned)nr.b * (unsigned)RB};
                f32x4 a2[2];
                constexpr int NU = 6;
                uint4 f[2][2][3];
                auto ld = [&](int u, uint4 (&d)[2][3]) {
#pragma unroll
                    for (int s = 0; s < 2; ++s)
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw) d[s][kw] = *reinterpret_cast<const uint4 *>(T1 + rowb[s] + (u >> 1) * RB + t1off[kw][u & 1]);
                };
                ld(0, f[0]);
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int kh = u >> 1, ks = u & 1;
                    if (u + 1 < NU) ld(u + 1, f[(u + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                        for (int s = 0; s < 2; ++s) a2[s] = mfma16(w2r[(kh * 3 + kw) * 2 + ks], f[u & 1][s][kw], (u == 0 && kw == 0) ? h2 : a2[s]);
                }
                unsigned char *T2w = T2 + (j & 1) * BN56_T2_BYTES;
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    uint2 o;
                    o.x = pack_relu_bf16x2(a2[s][0], a2[s][1]);
                    o.y = pack_relu_bf16x2(a2[s][2], a2[s][3]);
                    *reinterpret_cast<uint2 *>(T2w + rowb[s] + toff) = o;
                }
            } else {
                f32x4 a2[BN56_ROWS];
                {
                    // units of 3 fragments (t1 row R, k half ks, kw = 0..2: up to 9 MFMAs), requested one unit ahead
                    constexpr int NU = 2 * (BN56_ROWS + 2);
                    uint4 f[2][3];
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) f[0][kw] = *reinterpret_cast<const uint4 *>(T1 + t1off[kw][0]);
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int R = u >> 1, ks = u & 1;
                        if (u + 1 < NU) {
#pragma unroll
                            for (int kw = 0; kw < 3; ++kw) f[(u + 1) & 1][kw] = *reinterpret_cast<const uint4 *>(T1 + ((u + 1) >> 1) * RB + t1off[kw][(u + 1) & 1]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                            for (int kh = 0; kh < 3; ++kh) {
                                const int m = R - kh;
                                if (m >= 0 && m < BN56_ROWS) a2[m] = mfma16(w2r[(kh * 3 + kw) * 2 + ks], f[u & 1][kw], (kh == 0 && kw == 0 && ks == 0) ? h2 : a2[m]);
                            }
                    }
                }
                unsigned char *T2w = T2 + (j & 1) * BN56_T2_BYTES;
#pragma unroll
                for (int m = 0; m < BN56_ROWS; ++m) {
                    uint2 o;
                    o.x = pack_relu_bf16x2(a2[m][0], a2[m][1]);
                    o.y = pack_relu_bf16x2(a2[m][2], a2[m][3]);
                    *reinterpret_cast<uint2 *>(T2w + m * RB + toff) = o;
                }
            }
            BN56_STAMP(4); // conv2 + t2 epilogue
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of the next x tile have landed
            BN56_STAMP(5); // wait for the x tile
            bn56_barrier(); // D: t2[j & 1] and x tile j+1 are complete; every front wave has read t1
            BN56_STAMP(6); // wait at D
            // keep the last two t1 rows for the next step (rows 4, 5 -> 0, 1: same swizzle, the pixel index moves by 64); the next
            // step's t1 rows are written behind its barrier E
            reinterpret_cast<uint4 *>(T1)[tid] = reinterpret_cast<const uint4 *>(T1 + BN56_ROWS * RB)[tid];
            xs = xn;
        }
        BN56_TIMER_FLUSH(0);
        // the back waves still work on the last step: join its two barriers (E, C)
        bn56_barrier();
        bn56_barrier();
    } else {
        // =========================================== back waves: conv3 + residual / downsample + ReLU + stores ===========================================
        // A wave works on QUARTERS of its 64 output channels (2 rows = 32 pixels).  Its operands are all in LDS:
        //   t2       the quarter's two rows of t2[(j-1) & 1];
        //   side     the operand from x for those pixels -- identity: the residual x[pixel][64w .. 64w+63], i.e. chunk w of the x
        //            tile; DS: x[pixel][0 .. 63], the downsample branch's B operand, the tile's only chunk.  It is the B-fragment
        //            shape conv1 reads, one column to the right: output pixel r16 is image column c0 + r16 = tile column r16 + 1
        //            (the tile starts at the halo column c0 - 1), so the lane offsets carry the swizzle of column r16 + 1.  For
        //            r16 = 15 that is "column 16", pixel 0 of the next tile row (or the bytes behind the tile): garbage, like
        //            r16 = 14's halo column, in the two output columns that are never stored.  LDS banks: the 16 lanes of a
        //            ds_read_b128 group are the columns 1 .. 16 at one logical chunk k: columns 2i, 2i+1 share the physical chunk
        //            k ^ i and lie 128 B apart (the two halves of the 64 banks); columns 1 and 16 both have chunk k ^ 0, in the odd
        //            and the even half (16 * 128 = 0 mod 256): 16 distinct 16-byte bank groups, conflict-free, as xoff's.
        //            Both side operands enter the accumulator through the matrix core: DS with the downsample weights, identity
        //            with a 0 / 1 selector as the A operand (x * 1.0 + acc in fp32 is the plain fp32 add, and it costs one MFMA
        //            per 16 x 16 outputs instead of 2 vector instructions per output);
        //   OT       (wave-private) the quarter's outputs, written in the accumulator layout (8 bytes per lane) and read back as
        //            16-byte chunks with 8 consecutive lanes on one pixel's 128 bytes, so every global store instruction covers 8
        //            whole lines.
        // (With the accumulator layout on the global side -- adjacent lanes on pixels 512 B apart, 8 bytes each -- the CU's
        // address path took 64 line look-ups per instruction and 6 000 cycles per step segment: stamped)
        constexpr int NW3 = DS ? 4 : 2; // k-steps of conv3's weights per 16-channel group: [t2 | x] or t2
        uint4 w3r[4 * NW3];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int ks = 0; ks < NW3; ++ks)
                w3r[g * NW3 + ks] = *reinterpret_cast<const uint4 *>(p.W3 + (size_t)(64 * w + 16 * g + r16) * K3 + 32 * ks + 8 * q);
        uint4 sel[2]; // identity: A operand that copies channel 16h + i of a 32-channel k-step into output row i
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t e[4];
#pragma unroll
            for (int d2 = 0; d2 < 4; ++d2) e[d2] = ((8 * q + 2 * d2 == 16 * h + r16) ? 0x3F80u : 0u) | ((8 * q + 2 * d2 + 1 == 16 * h + r16) ? 0x3F800000u : 0u);
            sel[h] = make_uint4(e[0], e[1], e[2], e[3]);
        }
        f32x4 h3[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 t = *reinterpret_cast<const float4 *>(p.sh3 + 64 * w + 16 * g + 4 * q);
            h3[g] = f32x4{t.x, t.y, t.z, t.w};
        }
        unsigned char *OT = T2 + 2 * BN56_T2_BYTES + w * BN56_OT_BYTES;
        const unsigned char *XS = XT + (DS ? 0 : w) * BN56_XCH_BYTES; // this wave's chunk of slot 0
        unsigned soff[2]; // side fragment: tile column r16 + 1
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) soff[ks] = (unsigned)((r16 + 1) * 128 + ((((4 * ks + q) ^ ((r16 + 1) >> 1)) & 7) << 4));
        // accumulator-layout offsets inside a quarter tile: pixel (mm, r16), this lane's 4 channels 16g + 4q ..
        unsigned aoff[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) aoff[g] = (unsigned)(r16 * 128 + ((((2 * g + (q >> 1)) ^ swc) & 7) << 4) + 8 * (q & 1));
        // line-layout roles (the output read-back): lane -> pixel column 8i + (lane >> 3), physical 16-byte slot lane & 7
        const int lcol = lane >> 3, lps = lane & 7;
        const i32x4_t ysrd = bn56_srd(p.Y, (unsigned)((size_t)p.B * H * Wd * 256 * 2));
        const unsigned yrow_bytes = (unsigned)(Wd * 256 * 2);
        const unsigned ybase = (unsigned)((c0 * 256 + 64 * w) * 2);
        unsigned yvoff[2]; // this lane's byte offsets from a row's first strip pixel (out of range: no such output column)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = 8 * i + lcol, chunk = (lps ^ (c >> 1)) & 7;
            const bool ok = c < BN56_COLS && c0 + c < Wd;
            yvoff[i] = ok ? (unsigned)(c * 256 + chunk * 8) * 2u : BN56_OOB;
        }
        auto row_ok = [&](const bn56_row &t) { return t.b >= b0 && t.b < b1 && t.r < H; };
        // Pruned form (SUB == 2): a quarter stores ONE row at most (bn56_quarter_row), and of it the even image columns -- the even strip
        // columns, c0 = 14 * strip being even.  OT holds that row with the even columns first: pixel r16 at (r16 >> 1) * 128, the odd ones 1 KiB
        // behind; 16-byte chunk k of a pixel sits in slot k ^ (r16 >> 1) ^ (r16 & 1).  Writes: the 32 lanes of a ds_write_b64 group (r16, q & 1
        // at fixed q >> 1) fall on 16 distinct 16-byte slots of the 256 bank bytes -- (r16 >> 1) & 1 picks the half, and within a half the even
        // and the odd columns take slots of opposite parity.  Read-back: lane l reads OT + 16 l, i.e. slot l & 7 of strip column 2 (l >> 3) --
        // contiguous, conflict-free -- and ONE store instruction carries the 7 needed columns' whole 128-byte lines of this wave's channels
        // (lanes 56 .. 63, "column 14", and columns outside the image: out of range).
        [[maybe_unused]] unsigned aoff2[4], yvoff2 = BN56_OOB;
        if constexpr (SUB == 2) {
#pragma unroll
            for (int g = 0; g < 4; ++g)
                aoff2[g] = (unsigned)((r16 >> 1) * 128 + (r16 & 1) * 1024 + ((((2 * g + (q >> 1)) ^ (r16 >> 1) ^ (r16 & 1)) & 7) << 4) + 8 * (q & 1));
            const int c = SUB * lcol, chunk = (lps ^ lcol) & 7;
            if (c < BN56_COLS && bn56_col_needed(c0 + c, Wd, SUB)) yvoff2 = (unsigned)(c * 256 + chunk * 8) * 2u;
        }
        BN56_TIMER_DECL;
        // T2q: the quarter's two t2 rows; S0, S1: the x-tile rows (this wave's chunk) of its two rows; t0: its first virtual row
        auto quarter = [&](const unsigned char *T2q, const unsigned char *S0, const unsigned char *S1, bn56_row t0) {
            if constexpr (SUB == 2) {
                const int mm = bn56_quarter_row(t0, b0, b1, H, VH, SUB); // wave-uniform
                if (mm < 0) return;
                if (mm) t0.step(VH);
                const unsigned char *Tq = T2q + mm * RB, *S = mm ? S1 : S0;
                uint4 tb[2], xb[2];
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    tb[ks] = *reinterpret_cast<const uint4 *>(Tq + xoff[ks]);
                    xb[ks] = *reinterpret_cast<const uint4 *>(S + soff[ks]);
                }
                BN56_STAMP(0);
                f32x4 a3[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    a3[g] = mfma16(w3r[g * NW3 + 0], tb[0], h3[g]);
                    a3[g] = mfma16(w3r[g * NW3 + 1], tb[1], a3[g]);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) a3[g] = mfma16(sel[g & 1], xb[g >> 1], a3[g]); // + residual
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 o;
                    o.x = pack_relu_bf16x2(a3[g][0], a3[g][1]);
                    o.y = pack_relu_bf16x2(a3[g][2], a3[g][3]);
                    *reinterpret_cast<uint2 *>(OT + aoff2[g]) = o;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave's OT writes are done (the tile is private to the wave)
                __builtin_amdgcn_sched_barrier(0);
                BN56_STAMP(1);
                const uint4 v = *reinterpret_cast<const uint4 *>(OT + lane * 16);
                bstore16_asm(ysrd, yvoff2, (unsigned)t0.p * yrow_bytes + ybase, v);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // OT is read: the next quarter may overwrite it
                BN56_STAMP(2);
                return;
            }
            uint4 tb[2][2], xb[2][2];
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) tb[mm][ks] = *reinterpret_cast<const uint4 *>(T2q + mm * RB + xoff[ks]);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                xb[0][ks] = *reinterpret_cast<const uint4 *>(S0 + soff[ks]);
                xb[1][ks] = *reinterpret_cast<const uint4 *>(S1 + soff[ks]);
            }
            BN56_STAMP(0); // t2 + side fragment reads
            f32x4 a3[4][2];
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    a3[g][mm] = mfma16(w3r[g * NW3 + 0], tb[mm][0], h3[g]); // shift: the chain's C operand
                    a3[g][mm] = mfma16(w3r[g * NW3 + 1], tb[mm][1], a3[g][mm]);
                }
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if constexpr (DS) {
                        a3[g][mm] = mfma16(w3r[g * NW3 + 2], xb[mm][0], a3[g][mm]);
                        a3[g][mm] = mfma16(w3r[g * NW3 + 3], xb[mm][1], a3[g][mm]);
                    } else {
                        a3[g][mm] = mfma16(sel[g & 1], xb[mm][g >> 1], a3[g][mm]); // + residual
                    }
                }
#pragma unroll
            for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint2 o;
                    o.x = pack_relu_bf16x2(a3[g][mm][0], a3[g][mm][1]);
                    o.y = pack_relu_bf16x2(a3[g][mm][2], a3[g][mm][3]);
                    *reinterpret_cast<uint2 *>(OT + mm * RB + aoff[g]) = o;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // this wave's OT writes are done (the tile is private to the wave)
            __builtin_amdgcn_sched_barrier(0);
            BN56_STAMP(1); // MFMAs + epilogue into OT
            bn56_row t = t0;
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                const bool rok = row_ok(t);
                const unsigned so = rok ? (unsigned)t.p * yrow_bytes + ybase : 0u;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(OT + (2 * mm + i) * 1024 + lane * 16);
                    bstore16_asm(ysrd, rok ? yvoff[i] : BN56_OOB, so, v);
                }
                t.step(VH);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // OT is read: the next quarter may overwrite it
            BN56_STAMP(2); // OT read-back + stores
        };
        bn56_row out{b0 - 1, H, b0 * H}; // virtual row S - 1 (the padding row above the run): the first output row of step 0
        bn56_barrier(); // D (prologue)
        // iteration 0: the front waves compute step 0
        bn56_barrier(); // E
        bn56_barrier(); // C
        bn56_barrier(); // D: t2[0] is complete
        unsigned xp = 2 * SLOT, xc = 0u; // byte offsets of slot (j - 2) % 3 and slot (j - 1) % 3
        BN56_TIMER_START;
#pragma unroll 1
        for (int j = 1; j <= nsteps; ++j) { // outputs of step j - 1: row 3 of tile j-2, rows 0..2 of tile j-1
            const unsigned char *T2r = T2 + ((j - 1) & 1) * BN56_T2_BYTES;
            bn56_row r1 = out;
            r1.step(VH); r1.step(VH);
            quarter(T2r, XS + xp + 3 * RB, XS + xc, out);
            bn56_barrier(); // E: behind it the DMA of tile j+1 overwrites slot (j - 2) % 3
            bn56_barrier(); // C
            BN56_STAMP(3); // wait at E, C
            quarter(T2r + 2 * RB, XS + xc + RB, XS + xc + 2 * RB, r1);
            out = r1;
            out.step(VH); out.step(VH);
            xp = xc;
            xc = xc + SLOT == 3 * SLOT ? 0u : xc + SLOT;
            if (j < nsteps) bn56_barrier(); // D (the front waves' last D belongs to step nsteps - 1; their two trailing barriers pair with this iteration's E, C)
            BN56_STAMP(3); // wait at D
        }
        BN56_TIMER_FLUSH(1);
    }
}
