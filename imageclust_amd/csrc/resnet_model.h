// resnet_model.h -- what the embedding units share (host only: no kernel, no device code): the loaded model (model.hip fills it,
// resnet.hip runs it), the precision dispatch and the uploads.  The weight layouts, their constants (STEM_K, STEM_ROWK, ST2_K) and
// the host bf16 conversions are defined once, in resnet_pack.h.
#pragma once
#include "mfma_tile.h" // element traits (F32, BF16, BF16X3)
#include "resnet_pack.h"

#define ICL_MAX_LANES 4 /* forward passes in flight (ICL_EMBED_STREAMS) */

static_assert(PACK_FP32 == ICL_PREC_FP32 && PACK_BF16 == ICL_PREC_BF16 && PACK_BF16X3 == ICL_PREC_BF16X3, "resnet_pack.h numbers the storage formats as imageclust.h");

struct conv_layer {
    icl_conv_rec rec;
    int K = 0; // k of a weight row: cin * k * k, STEM_K for the stem
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

static inline int upload(icl_ctx *ctx, void **dst, const void *src, size_t bytes)
{
    ICL_HIP(ctx, hipMalloc(dst, bytes));
    ICL_HIP(ctx, hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    return ICL_OK;
}
// n fp32 values in the storage format of prec (pack_storage) into a new allocation *dst
static inline int upload_as(icl_ctx *ctx, int prec, void **dst, const float *src, size_t n)
{
    std::vector<uint16_t> buf;
    return upload(ctx, dst, pack_storage(prec, src, n, buf), pack_storage_bytes(prec, n));
}
