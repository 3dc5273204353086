// resnet_model.h -- what the embedding units share (host only: no kernel, no device code): the loaded model (model.hip fills it,
// resnet.hip runs it), the weight-layout constants the packer and the kernels must agree on, the host bf16 conversions and the
// precision dispatch.
#pragma once
#include "mfma_tile.h" // element traits (F32, BF16, BF16X3)

#include <cstring>

#define ICL_MAX_LANES 4 /* forward passes in flight (ICL_EMBED_STREAMS) */

// weight layouts of the stem kernels (resnet.hip, resnet_fused.h) as icl_model_load_blob packs them
#define STEM_K 192   /* stem_conv_kernel / stem_pool_kernel: K = 147 padded, 7 filter rows of STEM_ROWK k slots + zeros */
#define STEM_ROWK 24 /* k slots per filter row (21 used) */
#define ST2_K 224    /* stem2_pool_kernel: 7 filter rows x 8 kw slots x 4 channel slots */

struct conv_layer {
    icl_conv_rec rec;
    int K = 0, cin_eff = 0; // cin_eff: channel count seen by the kernel (160 for the lowered stem)
    void *w[3] = {nullptr, nullptr, nullptr}; // [ICL_PREC_FP32], [ICL_PREC_BF16], [ICL_PREC_BF16X3] (split layout: host_split32)
    float *scale = nullptr, *shift = nullptr;
    // block-0 c3 only: [Cout][mid + cin] = [W3*scale3 | Wds*scale_ds] and shift3 + shift_ds (downsample fused in)
    void *wfused[3] = {nullptr, nullptr, nullptr};
    float *shift_fused = nullptr;
    // stage 1 only (bneck56_kernel): bf16(W * scale), the BatchNorm scale folded into the weights before rounding
    void *wfold = nullptr;
};

struct icl_model {
    conv_layer conv[ICL_RESNET50_NCONV];
    int nconv = 0;
    float *fcw = nullptr, *fcb = nullptr;
    // activation workspace
    void *buf[ICL_MAX_LANES][5] = {}; // one activation workspace per forward pass in flight
    float *pooled[ICL_MAX_LANES] = {};
    hipStream_t xstream[ICL_MAX_LANES] = {}; // lanes 2.. (lane 0 = ctx->stream, lane 1 = ctx->stream2)
    hipEvent_t xjoin[ICL_MAX_LANES] = {};
    int ws_lanes = 0;
    void *zero = nullptr; // 256 zero bytes: LDS-DMA source for padded taps
    float *ones = nullptr; // [2048] scale of the fused layers (their BN scale is folded into the weights)
    int ws_batch = 0, ws_prec = -1;
};

// activation workspace of the loaded model for `lanes` forward passes of `batch` images in flight (model.hip)
int icl_model_ensure_ws(icl_ctx *ctx, int batch, int prec, int lanes);
// the forward passes of n images already on the device, ctx->mu held (resnet.hip); also called by icl_embed_cluster_dev (ward.hip)
// and the batched file ingest (jpeg_gpu.hip)
int icl_embed_dev_locked(icl_ctx *ctx, const uint8_t *d_img, int64_t n, int head, int prec, float *d_out);

// ---- precision dispatch ---------------------------------------------------------------------------------------------
static inline bool prec_ok(int prec) { return prec == ICL_PREC_FP32 || prec == ICL_PREC_BF16 || prec == ICL_PREC_BF16X3; }
static inline bool head_ok(int head) { return head == ICL_HEAD_POOLED || head == ICL_HEAD_DENSE0; }

// f(tag) with a value of the element-traits type of prec: with_prec(prec, [&](auto t) { using T = decltype(t); ... })
template <typename F>
static inline auto with_prec(int prec, F &&f)
{
    if (prec == ICL_PREC_BF16) return f(BF16{});
    if (prec == ICL_PREC_BF16X3) return f(BF16X3{});
    return f(F32{});
}
// What the host needs to know of a precision, in REAL channels: the split layout keeps two bf16 per channel (the bytes of an fp32
// tensor) and covers 32 channels per 64-element k-step.
template <typename T>
struct prec_host {
    static constexpr size_t act_bytes = is_x3<T>::value ? 4 : sizeof(typename T::elem); // bytes per activation / weight element
    static constexpr int bk = is_x3<T>::value ? T::BK / 2 : T::BK;                      // channels per k-step
};
static inline size_t prec_act_bytes(int prec) { return with_prec(prec, [](auto t) { return prec_host<decltype(t)>::act_bytes; }); }
static inline int prec_bk(int prec) { return with_prec(prec, [](auto t) { return prec_host<decltype(t)>::bk; }); }

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

static inline int upload(icl_ctx *ctx, void **dst, const void *src, size_t bytes)
{
    ICL_HIP(ctx, hipMalloc(dst, bytes));
    ICL_HIP(ctx, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return ICL_OK;
}
