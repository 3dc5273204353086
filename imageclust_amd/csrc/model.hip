// model.hip -- the ResNet50-v1 model of a context (host only): the topology, the synthetic weight generator, the ICLW blob loader
// that re-packs and uploads the weights in every layout the kernels of resnet.hip read, and the activation workspace.
//
// Replaces LoadPretrainedModelONNX (internal/embeddings/embeddings.go:28-43); the ONNX graph itself is read by onnx_reader.hip.
#include "icl_common.h"
#include "resnet50_topology.h"
#include "resnet_model.h"

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <new>
#include <vector>

static int64_t blob_floats(const icl_blob_header &h)
{
    icl_conv_rec t[ICL_RESNET50_NCONV];
    const int n = resnet50_topology(t);
    int64_t tot = 0;
    for (int i = 0; i < n; ++i) {
        tot += (int64_t)t[i].cout * t[i].cin * t[i].k * t[i].k + 4 * (int64_t)t[i].cout;
        if (h.has_bias[i]) tot += t[i].cout;
    }
    return tot + (int64_t)ICL_FC_OUT * ICL_FEAT_DIM + ICL_FC_OUT;
}

static void default_header(icl_blob_header &h)
{
    memset(&h, 0, sizeof h);
    h.magic = ICL_BLOB_MAGIC;
    h.version = ICL_BLOB_VERSION;
    h.bn_eps = 1e-5f;
    h.n_conv = ICL_RESNET50_NCONV;
    icl_conv_rec t[ICL_RESNET50_NCONV];
    const int n = resnet50_topology(t);
    // Gluon resnet50_v1: the bottleneck's 1x1 convs carry a bias, 3x3 / stem / downsample do not
    for (int i = 0; i < n; ++i) h.has_bias[i] = (t[i].role == 1 || t[i].role == 3) ? 1 : 0;
}

extern "C" int64_t icl_synthetic_blob_bytes(void)
{
    icl_blob_header h;
    default_header(h);
    return (int64_t)sizeof(h) + 4 * blob_floats(h);
}

// counter-based generator: element e of the blob draws from splitmix64(seed, e)
struct synth_rng {
    uint64_t seed, ctr = 0;
    double uni() { return (double)(icl_splitmix64(seed ^ (0xD1B54A32D192ED03ull * ++ctr)) >> 11) * (1.0 / 9007199254740992.0); }
    double normal()
    {
        const double u1 = uni(), u2 = uni();
        return std::sqrt(-2.0 * std::log(u1 > 1e-300 ? u1 : 1e-300)) * std::cos(6.283185307179586476925 * u2);
    }
};

extern "C" int icl_synthetic_blob(uint64_t seed, void *blob, int64_t bytes)
{
    if (!blob || bytes != icl_synthetic_blob_bytes()) return icl_fail(nullptr, ICL_ERR_ARG, "icl_synthetic_blob: need a %lld-byte buffer", (long long)icl_synthetic_blob_bytes());
    icl_blob_header h;
    default_header(h);
    memcpy(blob, &h, sizeof h);
    float *p = (float *)((char *)blob + sizeof h);
    icl_conv_rec t[ICL_RESNET50_NCONV];
    const int n = resnet50_topology(t);
    synth_rng g{seed};
    for (int i = 0; i < n; ++i) {
        const int64_t nw = (int64_t)t[i].cout * t[i].cin * t[i].k * t[i].k;
        const double sd = std::sqrt(2.0 / ((double)t[i].cin * t[i].k * t[i].k)); // He init
        for (int64_t e = 0; e < nw; ++e) *p++ = (float)(sd * g.normal());
        if (h.has_bias[i])
            for (int c = 0; c < t[i].cout; ++c) *p++ = (float)(0.01 * g.normal());
        for (int c = 0; c < t[i].cout; ++c) *p++ = (float)(0.5 + g.uni());      // gamma ~ U(0.5,1.5)
        for (int c = 0; c < t[i].cout; ++c) *p++ = (float)(0.1 * g.normal());   // beta
        for (int c = 0; c < t[i].cout; ++c) *p++ = (float)(0.1 * g.normal());   // running mean
        for (int c = 0; c < t[i].cout; ++c) *p++ = (float)(0.5 + g.uni());      // running var ~ U(0.5,1.5)
    }
    const double fsd = std::sqrt(1.0 / ICL_FEAT_DIM);
    for (int64_t e = 0; e < (int64_t)ICL_FC_OUT * ICL_FEAT_DIM; ++e) *p++ = (float)(fsd * g.normal());
    for (int e = 0; e < ICL_FC_OUT; ++e) *p++ = 0.0f;
    return ICL_OK;
}

static void model_destroy(icl_model *m)
{
    if (!m) return;
    for (auto &c : m->conv) {
        for (void *p : {c.w[0], c.w[1], c.w[2], (void *)c.scale, (void *)c.shift, c.wfused[0], c.wfused[1], c.wfused[2], (void *)c.shift_fused, c.wfold})
            if (p) (void)hipFree(p);
    }
    for (void *p : {(void *)m->fcw, (void *)m->fcb, m->zero, (void *)m->ones})
        if (p) (void)hipFree(p);
    for (int l = 0; l < ICL_MAX_LANES; ++l) {
        for (void *b : m->buf[l])
            if (b) (void)hipFree(b);
        if (m->pooled[l]) (void)hipFree(m->pooled[l]);
        if (m->xstream[l]) (void)hipStreamDestroy(m->xstream[l]);
        if (m->xjoin[l]) (void)hipEventDestroy(m->xjoin[l]);
    }
    delete m;
}

void icl_model_free(icl_ctx *ctx)
{
    model_destroy(ctx->model);
    ctx->model = nullptr;
}

// ---- the ICLW blob loader: parse a layer, pack it (resnet_pack.h), upload it ------------------------------------------------------------
// one convolution's tensors in the blob: W (OIHW), bias (null without), then the BatchNorm's gamma, beta, running mean and variance
struct blob_layer {
    const float *W, *bias, *gamma, *beta, *mean, *var;
};
// a cursor over the blob's floats (their count is checked against the topology before the first read)
struct blob_cursor {
    const float *p;
    const float *take(int64_t n) { return (p += n) - n; }
    blob_layer layer(const icl_conv_rec &r, bool has_bias) // (a braced list is evaluated left to right: the blob's order)
    {
        return blob_layer{take((int64_t)r.cout * r.cin * r.k * r.k), has_bias ? take(r.cout) : nullptr, take(r.cout), take(r.cout), take(r.cout), take(r.cout)};
    }
};
// a convolution as packed on the host: the fp32 weight rows in the kernels' layout and the folded BatchNorm
struct packed_conv {
    std::vector<float> w, scale, shift;
};

// One convolution: weights in every precision's storage, scale and shift, and the scale-folded bf16 copy of the fused kernels.
// Leaves the packed fp32 form in pk.
static int load_conv(icl_ctx *ctx, conv_layer &L, const icl_conv_rec &r, const blob_layer &b, float bn_eps, packed_conv &pk)
{
    const bool stem = r.role == 0;
    L.rec = r;
    L.K = stem ? STEM_K : r.cin * r.k * r.k;
    if (stem) pack_stem_rows(b.W, pk.w);
    else pack_ohwi(b.W, r.cout, r.cin, r.k, pk.w);
    pack_bn_fold(b.gamma, b.beta, b.mean, b.var, b.bias, bn_eps, r.cout, pk.scale, pk.shift);
    for (int prec : {ICL_PREC_FP32, ICL_PREC_BF16, ICL_PREC_BF16X3}) {
        if (stem && prec == ICL_PREC_BF16X3) continue; // (the BF16X3 stem runs in fp32: ICL_PREC_FP32 weights)
        ICL_TRY(upload_as(ctx, prec, &L.w[prec], pk.w.data(), pk.w.size()));
    }
    ICL_TRY(upload_as(ctx, ICL_PREC_FP32, (void **)&L.scale, pk.scale.data(), pk.scale.size()));
    ICL_TRY(upload_as(ctx, ICL_PREC_FP32, (void **)&L.shift, pk.shift.data(), pk.shift.size()));
    if (stem) { // stem2_pool_kernel
        std::vector<uint16_t> ws;
        pack_stem2(b.W, pk.scale.data(), ws);
        ICL_TRY(upload(ctx, &L.wfold, ws.data(), ws.size() * 2));
    }
    if (r.stage == 1 && r.role >= 1 && r.role <= 3) { // the fused stage-1 bottleneck takes its BN scales inside the weights
        std::vector<float> wf;
        pack_row_scale(pk.w.data(), pk.scale.data(), r.cout, L.K, wf);
        ICL_TRY(upload_as(ctx, ICL_PREC_BF16, &L.wfold, wf.data(), wf.size()));
    }
    return ICL_OK;
}

// A stage's downsample branch fused into block 0's last convolution L3: y = relu(W3'.t2 + Wds'.x_strided + (sh3 + sh_ds))
static int load_fused_ds(icl_ctx *ctx, conv_layer &L3, const packed_conv &c3, int k1, const packed_conv &ds, int k2)
{
    const int cout = L3.rec.cout;
    std::vector<float> w3, wds, wf, sh((size_t)cout);
    pack_row_scale(c3.w.data(), c3.scale.data(), cout, k1, w3);
    pack_row_scale(ds.w.data(), ds.scale.data(), cout, k2, wds);
    pack_row_concat(w3.data(), k1, wds.data(), k2, cout, wf);
    for (int co = 0; co < cout; ++co) sh[(size_t)co] = c3.shift[(size_t)co] + ds.shift[(size_t)co];
    for (int prec : {ICL_PREC_FP32, ICL_PREC_BF16, ICL_PREC_BF16X3}) ICL_TRY(upload_as(ctx, prec, &L3.wfused[prec], wf.data(), wf.size()));
    return upload_as(ctx, ICL_PREC_FP32, (void **)&L3.shift_fused, sh.data(), sh.size());
}

// the dense head, and the constant pages of the kernels
static int load_head(icl_ctx *ctx, icl_model *m, blob_cursor &cur)
{
    const std::vector<float> one(2048, 1.0f);
    ICL_TRY(upload_as(ctx, ICL_PREC_FP32, (void **)&m->ones, one.data(), one.size()));
    ICL_TRY(upload_as(ctx, ICL_PREC_FP32, (void **)&m->fcw, cur.take((int64_t)ICL_FC_OUT * ICL_FEAT_DIM), (size_t)ICL_FC_OUT * ICL_FEAT_DIM));
    ICL_TRY(upload_as(ctx, ICL_PREC_FP32, (void **)&m->fcb, cur.take(ICL_FC_OUT), (size_t)ICL_FC_OUT));
    ICL_HIP(ctx, hipMalloc(&m->zero, 256));
    ICL_HIP(ctx, hipMemset(m->zero, 0, 256));
    return ICL_OK;
}

extern "C" int icl_model_load_blob(icl_ctx *ctx, const void *blob, int64_t bytes)
{
    if (!ctx || !blob) return icl_fail(ctx, ICL_ERR_ARG, "icl_model_load_blob: bad argument");
    if (bytes < (int64_t)sizeof(icl_blob_header)) return icl_fail(ctx, ICL_ERR_IO, "weight blob too small");
    icl_blob_header h;
    memcpy(&h, blob, sizeof h);
    if (h.magic != ICL_BLOB_MAGIC || h.version != ICL_BLOB_VERSION || h.n_conv != ICL_RESNET50_NCONV)
        return icl_fail(ctx, ICL_ERR_IO, "not an ICLW v%u ResNet50 blob", ICL_BLOB_VERSION);
    if (bytes != (int64_t)sizeof h + 4 * blob_floats(h))
        return icl_fail(ctx, ICL_ERR_IO, "weight blob has %lld bytes, expected %lld", (long long)bytes, (long long)(sizeof h + 4 * blob_floats(h)));
    return no_throw(ctx, "icl_model_load_blob", [&]() -> int {
        std::lock_guard<std::mutex> lk(ctx->mu);
        icl_device_guard g(ctx->device);
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        icl_model_free(ctx);
        // built aside and installed after the last upload: a load that fails part-way leaves no model behind (ICL_ERR_NOMODEL later)
        std::unique_ptr<icl_model, void (*)(icl_model *)> own(new icl_model(), model_destroy);
        icl_model *m = own.get();
        icl_conv_rec t[ICL_RESNET50_NCONV];
        m->nconv = resnet50_topology(t);
        blob_cursor cur{(const float *)((const char *)blob + sizeof h)};
        packed_conv pk, src[4][2]; // src[stage - 1]: block 0's last convolution and its downsample layer, kept for the fusion below
        for (int i = 0; i < m->nconv; ++i) {
            const bool kept = t[i].block == 0 && t[i].role >= 3;
            ICL_TRY(load_conv(ctx, m->conv[i], t[i], cur.layer(t[i], h.has_bias[i] != 0), h.bn_eps, kept ? src[t[i].stage - 1][t[i].role - 3] : pk));
        }
        for (int i = 0; i < m->nconv; ++i) // canonical order: c1, c2, c3, ds
            if (t[i].block == 0 && t[i].role == 3) ICL_TRY(load_fused_ds(ctx, m->conv[i], src[t[i].stage - 1][0], t[i].cin, src[t[i].stage - 1][1], t[i + 1].cin));
        ICL_TRY(load_head(ctx, m, cur));
        ctx->model = own.release();
        return ICL_OK;
    });
}

extern "C" int icl_model_load_synthetic(icl_ctx *ctx, uint64_t seed)
{
    if (!ctx) return ICL_ERR_ARG;
    return no_throw(ctx, "icl_model_load_synthetic", [&]() -> int {
        const int64_t nb = icl_synthetic_blob_bytes();
        std::vector<char> blob((size_t)nb);
        ICL_TRY(icl_synthetic_blob(seed, blob.data(), nb));
        return icl_model_load_blob(ctx, blob.data(), nb);
    });
}

int icl_onnx_to_blob(icl_ctx *ctx, const char *path, std::vector<char> &blob); // onnx_reader.hip

extern "C" int icl_model_load_onnx(icl_ctx *ctx, const char *path)
{
    // LoadPretrainedModelONNX (embeddings.go:28-43): read the graph's initializers, validate the topology, upload.
    if (!ctx || !path) return icl_fail(ctx, ICL_ERR_ARG, "icl_model_load_onnx: bad argument");
    std::vector<char> blob;
    ICL_TRY(icl_onnx_to_blob(ctx, path, blob));
    return icl_model_load_blob(ctx, blob.data(), (int64_t)blob.size());
}

int icl_model_ensure_ws(icl_ctx *ctx, int batch, int prec, int lanes)
{
    icl_model *m = ctx->model;
    if (m->ws_batch >= batch && m->ws_prec == prec && m->ws_lanes >= lanes) return ICL_OK;
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    for (int l = 2; l < lanes; ++l)
        if (!m->xstream[l]) {
            ICL_HIP(ctx, hipStreamCreateWithFlags(&m->xstream[l], hipStreamNonBlocking));
            ICL_HIP(ctx, hipEventCreateWithFlags(&m->xjoin[l], hipEventDisableTiming));
        }
    for (int l = 0; l < ICL_MAX_LANES; ++l) {
        if (m->xstream[l]) ICL_HIP(ctx, hipStreamSynchronize(m->xstream[l]));
        for (auto &b : m->buf[l])
            if (b) {
                (void)hipFree(b);
                b = nullptr;
            }
        if (m->pooled[l]) (void)hipFree(m->pooled[l]);
        m->pooled[l] = nullptr;
    }
    m->ws_batch = 0;
    m->ws_lanes = 0;
    const size_t act = (size_t)batch * 802816 * prec_act_bytes(prec); // 112*112*64 == 56*56*256: the largest activation
    for (int l = 0; l < lanes; ++l) {
        for (auto &b : m->buf[l]) {
            hipError_t e = hipMalloc(&b, act);
            if (e != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "activation workspace (%zu B): %s", act, hipGetErrorString(e));
        }
        ICL_HIP(ctx, hipMalloc((void **)&m->pooled[l], (size_t)batch * ICL_FEAT_DIM * 4));
    }
    m->ws_batch = batch;
    m->ws_prec = prec;
    m->ws_lanes = lanes;
    return ICL_OK;
}
