// model.hip -- the ResNet50-v1 model of a context (host only): the topology, the synthetic weight generator, the ICLW blob loader
// that re-packs and uploads the weights in every layout the kernels of resnet.hip read, and the activation workspace.
//
// Replaces LoadPretrainedModelONNX (internal/embeddings/embeddings.go:28-43); the ONNX graph itself is read by onnx_reader.hip.
#include "icl_common.h"
#include "resnet_model.h"

#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

static int resnet50_topology(icl_conv_rec *out)
{
    static const int nblocks[4] = {3, 4, 6, 3};
    int n = 0;
    out[n++] = icl_conv_rec{3, 64, 7, 2, 3, 224, 112, 0, 0, 0};
    int h = 56, cin = 64;
    for (int s = 0; s < 4; ++s) {
        const int cout = 256 << s, mid = cout / 4;
        for (int b = 0; b < nblocks[s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1, ho = h / stride;
            out[n++] = icl_conv_rec{cin, mid, 1, stride, 0, h, ho, 1, s + 1, b};
            out[n++] = icl_conv_rec{mid, mid, 3, 1, 1, ho, ho, 2, s + 1, b};
            out[n++] = icl_conv_rec{mid, cout, 1, 1, 0, ho, ho, 3, s + 1, b};
            if (b == 0) out[n++] = icl_conv_rec{cin, cout, 1, stride, 0, h, ho, 4, s + 1, b};
            cin = cout;
            h = ho;
        }
    }
    return n;
}

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
        const float *p = (const float *)((const char *)blob + sizeof h);
        std::vector<float> wf;
        std::vector<uint16_t> wb;
        std::vector<float> sc, sh;
        std::vector<std::vector<float>> hw((size_t)m->nconv), hsc((size_t)m->nconv), hsh((size_t)m->nconv); // host copies for the fusion below
        for (int i = 0; i < m->nconv; ++i) {
            conv_layer &L = m->conv[i];
            L.rec = t[i];
            const int cin = t[i].cin, cout = t[i].cout, k = t[i].k;
            const float *W = p;
            p += (int64_t)cout * cin * k * k;
            const float *bias = nullptr;
            if (h.has_bias[i]) {
                bias = p;
                p += cout;
            }
            const float *gamma = p, *beta = p + cout, *mean = p + 2 * cout, *var = p + 3 * cout;
            p += 4 * (int64_t)cout;
            // re-pack OIHW -> [cout][kh][kw][cin] (stem: K padded 147 -> 160)
            L.cin_eff = (i == 0) ? STEM_K : cin;
            L.K = (i == 0) ? STEM_K : cin * k * k;
            wf.assign((size_t)cout * L.K, 0.0f);
            for (int co = 0; co < cout; ++co)
                for (int c = 0; c < cin; ++c)
                    for (int a = 0; a < k; ++a)
                        for (int b = 0; b < k; ++b) {
                            // stem: filter rows padded to 24 k-slots (stem_conv_kernel); others: [kh][kw][cin]
                            const size_t kk = (i == 0) ? (size_t)a * STEM_ROWK + (size_t)b * 3 + c : ((size_t)a * k + b) * cin + c;
                            wf[(size_t)co * L.K + kk] = W[(((size_t)co * cin + c) * k + a) * k + b];
                        }
            wb.resize(wf.size());
            for (size_t e = 0; e < wf.size(); ++e) wb[e] = host_bf16(wf[e]);
            ICL_TRY(upload(ctx, &L.w[ICL_PREC_FP32], wf.data(), wf.size() * 4));
            ICL_TRY(upload(ctx, &L.w[ICL_PREC_BF16], wb.data(), wb.size() * 2));
            if (i > 0) { // (the BF16X3 stem runs in fp32: ICL_PREC_FP32 weights)
                wb.resize(2 * wf.size());
                host_split32(wf.data(), wf.size(), wb.data());
                ICL_TRY(upload(ctx, &L.w[ICL_PREC_BF16X3], wb.data(), wb.size() * 2));
            }
            // BatchNormalization folded to y = x*scale + shift, conv bias folded into shift
            sc.resize(cout);
            sh.resize(cout);
            for (int c = 0; c < cout; ++c) {
                const double s = (double)gamma[c] / std::sqrt((double)var[c] + (double)h.bn_eps);
                sc[c] = (float)s;
                sh[c] = (float)((double)beta[c] - (double)mean[c] * s + (bias ? (double)bias[c] * s : 0.0));
            }
            ICL_TRY(upload(ctx, (void **)&L.scale, sc.data(), (size_t)cout * 4));
            ICL_TRY(upload(ctx, (void **)&L.shift, sh.data(), (size_t)cout * 4));
            if (i == 0) { // stem2_pool_kernel: [64][kh][8 kw slots][4 channel slots] = bf16(W * scale), zero in the padding
                std::vector<uint16_t> ws((size_t)64 * ST2_K, 0);
                for (int co = 0; co < 64; ++co)
                    for (int c = 0; c < 3; ++c)
                        for (int a = 0; a < 7; ++a)
                            for (int b = 0; b < 7; ++b)
                                ws[(size_t)co * ST2_K + (size_t)a * 32 + (size_t)b * 4 + c] = host_bf16(W[(((size_t)co * 3 + c) * 7 + a) * 7 + b] * sc[(size_t)co]);
                ICL_TRY(upload(ctx, &L.wfold, ws.data(), ws.size() * 2));
            }
            if (t[i].stage == 1 && t[i].role >= 1 && t[i].role <= 3) { // the fused stage-1 bottleneck takes its BN scales inside the weights
                for (size_t e = 0; e < wf.size(); ++e) wb[e] = host_bf16(wf[e] * sc[e / (size_t)L.K]);
                ICL_TRY(upload(ctx, &L.wfold, wb.data(), wb.size() * 2));
            }
            if (t[i].block == 0 && (t[i].role == 3 || t[i].role == 4)) {
                hw[(size_t)i] = wf;
                hsc[(size_t)i] = sc;
                hsh[(size_t)i] = sh;
            }
        }
        // fuse each stage's downsample branch into block 0's last conv: y = relu(W3'.t2 + Wds'.x_strided + (sh3 + sh_ds))
        for (int i = 0; i < m->nconv; ++i) {
            if (!(t[i].block == 0 && t[i].role == 3)) continue;
            const int ids = i + 1; // canonical order: c1, c2, c3, ds
            const int cout = t[i].cout, k1 = t[i].cin, k2 = t[ids].cin, kk = k1 + k2;
            wf.assign((size_t)cout * kk, 0.0f);
            sh.resize((size_t)cout);
            for (int co = 0; co < cout; ++co) {
                for (int c = 0; c < k1; ++c) wf[(size_t)co * kk + c] = hw[(size_t)i][(size_t)co * k1 + c] * hsc[(size_t)i][(size_t)co];
                for (int c = 0; c < k2; ++c) wf[(size_t)co * kk + k1 + c] = hw[(size_t)ids][(size_t)co * k2 + c] * hsc[(size_t)ids][(size_t)co];
                sh[(size_t)co] = hsh[(size_t)i][(size_t)co] + hsh[(size_t)ids][(size_t)co];
            }
            wb.resize(wf.size());
            for (size_t e = 0; e < wf.size(); ++e) wb[e] = host_bf16(wf[e]);
            conv_layer &L = m->conv[i];
            ICL_TRY(upload(ctx, &L.wfused[ICL_PREC_FP32], wf.data(), wf.size() * 4));
            ICL_TRY(upload(ctx, &L.wfused[ICL_PREC_BF16], wb.data(), wb.size() * 2));
            wb.resize(2 * wf.size());
            host_split32(wf.data(), wf.size(), wb.data());
            ICL_TRY(upload(ctx, &L.wfused[ICL_PREC_BF16X3], wb.data(), wb.size() * 2));
            ICL_TRY(upload(ctx, (void **)&L.shift_fused, sh.data(), (size_t)cout * 4));
        }
        {
            std::vector<float> one(2048, 1.0f);
            ICL_TRY(upload(ctx, (void **)&m->ones, one.data(), one.size() * 4));
        }
        ICL_TRY(upload(ctx, (void **)&m->fcw, p, (size_t)ICL_FC_OUT * ICL_FEAT_DIM * 4));
        p += (int64_t)ICL_FC_OUT * ICL_FEAT_DIM;
        ICL_TRY(upload(ctx, (void **)&m->fcb, p, (size_t)ICL_FC_OUT * 4));
        ICL_HIP(ctx, hipMalloc(&m->zero, 256));
        ICL_HIP(ctx, hipMemset(m->zero, 0, 256));
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
