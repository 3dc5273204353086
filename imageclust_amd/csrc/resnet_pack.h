// resnet_pack.h -- every weight layout the ResNet kernels read, as pure host functions: fp32 tensors in, vectors out; no context, no
// device, no error strings.  icl_model_load_blob (model.hip) and the per-layer entry points (resnet.hip) both pack through these, and
// tests/resnet_pack_main.cpp checks each against its index formula.  This is the one definition of each layout: the order of the
// floating-point operations (multiply in fp32, then round to bf16; the BatchNorm fold in double) is part of it.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// the stem kernels' weight rows (resnet.hip, resnet_fused.h)
#define STEM_K 192   /* stem_conv_kernel / stem_pool_kernel: K = 147 padded, 7 filter rows of STEM_ROWK k slots + zeros */
#define STEM_ROWK 24 /* k slots per filter row (21 used) */
#define ST2_K 224    /* stem2_pool_kernel: 7 filter rows x 8 kw slots x 4 channel slots */

// storage formats, numbered as ICL_PREC_FP32 / ICL_PREC_BF16 / ICL_PREC_BF16X3 (imageclust.h; resnet_model.h asserts it)
enum { PACK_FP32 = 0, PACK_BF16 = 1, PACK_BF16X3 = 2 };

// ---- host bf16 ------------------------------------------------------------------------------------------------------
static inline uint16_t host_bf16(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline float host_from_bf16(uint16_t v)
{
    uint32_t u = (uint32_t)v << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// The split bf16 layout of ICL_PREC_BF16X3 (mfma_tile.h, BF16X3): every run of 32 consecutive fp32 values v (a channel chunk of a pixel, or
// 32 k of a weight row: rows are whole chunks) becomes 64 bf16, [hi = bf16(v) of the 32 | lo = bf16(v - hi) of the same 32].  n % 32 == 0.
static inline void host_split32(const float *src, size_t n, uint16_t *dst)
{
    for (size_t i = 0; i < n; ++i) {
        const uint16_t h = host_bf16(src[i]);
        dst[(i & ~(size_t)31) * 2 + (i & 31)] = h;
        dst[(i & ~(size_t)31) * 2 + 32 + (i & 31)] = host_bf16(src[i] - host_from_bf16(h));
    }
}
// host_split32 undone: dst[i] = hi + lo in fp32
static inline void host_join32(const uint16_t *src, size_t n, float *dst)
{
    for (size_t i = 0; i < n; ++i) {
        const size_t j = (i & ~(size_t)31) * 2 + (i & 31);
        dst[i] = host_from_bf16(src[j]) + host_from_bf16(src[j + 32]);
    }
}

// ---- storage: n fp32 values <-> the bytes of a precision ------------------------------------------------------------------------
// fp32 as is, bf16 one host_bf16 per value, split bf16 two bf16 per value (host_split32, n % 32 == 0): the one place that knows
static inline size_t pack_storage_bytes(int prec, size_t n) { return prec == PACK_BF16 ? 2 * n : 4 * n; }
// -> the stored bytes: src itself for fp32, otherwise buf (filled here)
static inline const void *pack_storage(int prec, const float *src, size_t n, std::vector<uint16_t> &buf)
{
    if (prec == PACK_FP32) return src;
    buf.resize(pack_storage_bytes(prec, n) / 2);
    if (prec == PACK_BF16X3) host_split32(src, n, buf.data());
    else
        for (size_t i = 0; i < n; ++i) buf[i] = host_bf16(src[i]);
    return buf.data();
}
// ... and back (bytes: 2-byte aligned): bf16 widened, split bf16 as hi + lo
static inline void unpack_storage(int prec, const void *bytes, size_t n, float *dst)
{
    const uint16_t *t = (const uint16_t *)bytes;
    if (prec == PACK_FP32) memcpy(dst, bytes, 4 * n);
    else if (prec == PACK_BF16X3) host_join32(t, n, dst);
    else
        for (size_t i = 0; i < n; ++i) dst[i] = host_from_bf16(t[i]);
}

// ---- layouts --------------------------------------------------------------------------------------------------------
// OIHW [cout][cin][k][k] -> [cout][kh][kw][cin]: the K order of the implicit-GEMM convolution kernels (convolutions 1..52, icl_conv2d_fused)
static inline void pack_ohwi(const float *W, int cout, int cin, int k, std::vector<float> &out)
{
    const size_t K = (size_t)cin * k * k;
    out.resize((size_t)cout * K);
    for (int co = 0; co < cout; ++co)
        for (int c = 0; c < cin; ++c)
            for (int a = 0; a < k; ++a)
                for (int b = 0; b < k; ++b) out[(size_t)co * K + ((size_t)a * k + b) * cin + c] = W[(((size_t)co * cin + c) * k + a) * k + b];
}
// the stem's OIHW 64 x 3 x 7 x 7 -> [64][STEM_K]: filter row a in STEM_ROWK k slots, (kw b, channel c) at b * 3 + c, zero elsewhere
// (stem_conv_kernel, stem_pool_kernel)
static inline void pack_stem_rows(const float *W, std::vector<float> &out)
{
    out.assign((size_t)64 * STEM_K, 0.0f);
    for (int co = 0; co < 64; ++co)
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 7; ++a)
                for (int b = 0; b < 7; ++b) out[(size_t)co * STEM_K + (size_t)a * STEM_ROWK + (size_t)b * 3 + c] = W[(((size_t)co * 3 + c) * 7 + a) * 7 + b];
}
// the same source -> [64][ST2_K] = [64][kh][8 kw slots][4 channel slots] of bf16(W * scale[co]), zero in the padding (stem2_pool_kernel)
static inline void pack_stem2(const float *W, const float *scale, std::vector<uint16_t> &out)
{
    out.assign((size_t)64 * ST2_K, 0);
    for (int co = 0; co < 64; ++co)
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 7; ++a)
                for (int b = 0; b < 7; ++b)
                    out[(size_t)co * ST2_K + (size_t)a * 32 + (size_t)b * 4 + c] = host_bf16(W[(((size_t)co * 3 + c) * 7 + a) * 7 + b] * scale[co]);
}
// BatchNormalization folded to y = x * scale + shift, the convolution's bias (or null) folded into the shift: double arithmetic,
// each result rounded to float once
static inline void pack_bn_fold(const float *gamma, const float *beta, const float *mean, const float *var, const float *bias, float eps, int cout,
                                std::vector<float> &scale, std::vector<float> &shift)
{
    scale.resize((size_t)cout);
    shift.resize((size_t)cout);
    for (int c = 0; c < cout; ++c) {
        const double s = (double)gamma[c] / std::sqrt((double)var[c] + (double)eps);
        scale[c] = (float)s;
        shift[c] = (float)((double)beta[c] - (double)mean[c] * s + (bias ? (double)bias[c] * s : 0.0));
    }
}
// W[row][K] * scale[row], one fp32 multiply per element: a BatchNorm scale folded into packed weights before they are rounded
// (wfold of bneck56_kernel, both halves of wfused)
static inline void pack_row_scale(const float *W, const float *scale, int rows, int K, std::vector<float> &out)
{
    out.resize((size_t)rows * K);
    for (size_t e = 0; e < out.size(); ++e) out[e] = W[e] * scale[e / (size_t)K];
}
// [w1 (K1) | w2 (K2)] per output row: the weights of a dual-operand launch (wfused: conv_args with a second operand, bneck56_kernel<true>)
static inline void pack_row_concat(const float *w1, int K1, const float *w2, int K2, int rows, std::vector<float> &out)
{
    const size_t K = (size_t)K1 + K2;
    out.resize((size_t)rows * K);
    for (int r = 0; r < rows; ++r) {
        memcpy(&out[(size_t)r * K], w1 + (size_t)r * K1, (size_t)K1 * 4);
        memcpy(&out[(size_t)r * K + K1], w2 + (size_t)r * K2, (size_t)K2 * 4);
    }
}
