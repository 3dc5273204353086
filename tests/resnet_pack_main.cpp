// resnet_pack_main.cpp -- every weight layout of imageclust_amd/csrc/resnet_pack.h against its index formula, written out here: a
// stand-alone host program (no GPU, no HIP) that tests/test_resnet_pack_cpu.py builds with the address and undefined-behaviour
// sanitizers and runs.  Inputs hold distinct values, so a transposed index cannot pass.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/resnet_pack.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);    \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, " [%s]\n", #cond);                 \
            exit(1);                                           \
        }                                                      \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u)
{
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// distinct, non-zero, of both signs, not representable in bf16
static std::vector<float> distinct(size_t n, float step = 0.001f)
{
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = ((i & 1) ? -1.0f : 1.0f) * (0.37f + step * (float)i);
    return v;
}

static void test_ohwi(int cout, int cin, int k)
{
    const std::vector<float> W = distinct((size_t)cout * cin * k * k);
    std::vector<float> out(7, -1.0f); // (a vector in use: the packer sizes it)
    pack_ohwi(W.data(), cout, cin, k, out);
    CHECK(out.size() == W.size(), "ohwi size %zu", out.size());
    for (int co = 0; co < cout; ++co)
        for (int a = 0; a < k; ++a)
            for (int b = 0; b < k; ++b)
                for (int c = 0; c < cin; ++c) {
                    const size_t o = (((size_t)co * k + a) * k + b) * cin + c, i = (((size_t)co * cin + c) * k + a) * k + b;
                    CHECK(bits(out[o]) == bits(W[i]), "ohwi cout %d cin %d k %d: [%d][%d][%d][%d]", cout, cin, k, co, a, b, c);
                }
    printf("ohwi cout %d cin %d k %d: %zu elements\n", cout, cin, k, out.size());
}

// the stem layouts, read from the output side: slot kk of a row -> (kh a, kw b, channel c) or padding
static void test_stem()
{
    const std::vector<float> W = distinct((size_t)64 * 3 * 7 * 7);
    std::vector<float> rows;
    pack_stem_rows(W.data(), rows);
    CHECK(STEM_K == 192 && STEM_ROWK == 24 && ST2_K == 224 && rows.size() == (size_t)64 * 192, "stem rows size %zu", rows.size());
    size_t nz = 0;
    for (int co = 0; co < 64; ++co)
        for (int kk = 0; kk < 192; ++kk) {
            const int a = kk / 24, r = kk % 24, b = r / 3, c = r % 3;
            const float got = rows[(size_t)co * 192 + kk];
            if (a < 7 && r < 21) CHECK(bits(got) == bits(W[(((size_t)co * 3 + c) * 7 + a) * 7 + b]), "stem rows [%d][%d]", co, kk);
            else CHECK(bits(got) == 0, "stem rows [%d][%d]: padding holds %g", co, kk, got);
            nz += got != 0.0f;
        }
    CHECK(nz == (size_t)64 * 147, "stem rows: %zu non-zeros", nz);
    printf("stem rows: %zu of %zu non-zero\n", nz, rows.size());

    std::vector<float> scale(64);
    for (int co = 0; co < 64; ++co) scale[co] = ((co & 1) ? -1.0f : 1.0f) * (0.5f + (float)co / 61.0f);
    std::vector<uint16_t> st2;
    pack_stem2(W.data(), scale.data(), st2);
    CHECK(st2.size() == (size_t)64 * 224, "stem2 size %zu", st2.size());
    nz = 0;
    for (int co = 0; co < 64; ++co)
        for (int kk = 0; kk < 224; ++kk) {
            const int a = kk / 32, r = kk % 32, b = r / 4, c = r % 4;
            const uint16_t got = st2[(size_t)co * 224 + kk];
            if (b < 7 && c < 3) CHECK(got == host_bf16(W[(((size_t)co * 3 + c) * 7 + a) * 7 + b] * scale[co]), "stem2 [%d][%d]", co, kk);
            else CHECK(got == 0, "stem2 [%d][%d]: padding holds 0x%04x", co, kk, got);
            nz += got != 0;
        }
    CHECK(nz == (size_t)64 * 147, "stem2: %zu non-zeros", nz);
    printf("stem2: %zu of %zu non-zero\n", nz, st2.size());
}

static void test_fold()
{
    const float gamma[4] = {1.25f, -0.75f, 0.5f, -1.5f}, beta[4] = {0.1f, -0.2f, 0.3f, 0.05f}, mean[4] = {0.7f, -0.4f, 0.02f, 1.3f},
                var[4] = {0.9f, 1.4f, 0.51f, 1e-4f}, bias[4] = {0.01f, -0.03f, 0.2f, -0.6f};
    int n = 0;
    for (const float eps : {1e-5f, 1e-3f})
        for (const float *bs : {(const float *)nullptr, bias}) {
            std::vector<float> sc, sh;
            pack_bn_fold(gamma, beta, mean, var, bs, eps, 4, sc, sh);
            CHECK(sc.size() == 4 && sh.size() == 4, "fold sizes");
            for (int c = 0; c < 4; ++c) {
                const double s = (double)gamma[c] / std::sqrt((double)var[c] + (double)eps);
                double t = (double)beta[c] - (double)mean[c] * s;
                if (bs) t = (double)beta[c] - (double)mean[c] * s + (double)bs[c] * s;
                CHECK(bits(sc[c]) == bits((float)s), "fold scale, channel %d eps %g bias %d: %.9g", c, eps, bs != nullptr, sc[c]);
                CHECK(bits(sh[c]) == bits((float)t), "fold shift, channel %d eps %g bias %d: %.9g", c, eps, bs != nullptr, sh[c]);
                CHECK((sc[c] < 0) == (gamma[c] < 0), "fold: the scale keeps gamma's sign");
                ++n;
            }
        }
    printf("fold: %d channels\n", n);
}

static void test_rows()
{
    const int rows = 3, K1 = 32, K2 = 64, K = K1 + K2;
    const std::vector<float> w1 = distinct((size_t)rows * K1), w2 = distinct((size_t)rows * K2, 0.0017f);
    const float s1[3] = {1.5f, -0.625f, 0.3f}, s2[3] = {-2.25f, 0.7f, 1.1f};
    for (int on1 = 0; on1 < 2; ++on1)
        for (int on2 = 0; on2 < 2; ++on2) { // scale on neither, on one (either), on both
            std::vector<float> a = w1, b = w2, out;
            if (on1) pack_row_scale(w1.data(), s1, rows, K1, a);
            if (on2) pack_row_scale(w2.data(), s2, rows, K2, b);
            CHECK(a.size() == w1.size() && b.size() == w2.size(), "row scale sizes");
            pack_row_concat(a.data(), K1, b.data(), K2, rows, out);
            CHECK(out.size() == (size_t)rows * K, "concat size %zu", out.size());
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < K; ++c) {
                    float want;
                    if (c < K1) want = on1 ? w1[(size_t)r * K1 + c] * s1[r] : w1[(size_t)r * K1 + c];
                    else want = on2 ? w2[(size_t)r * K2 + c - K1] * s2[r] : w2[(size_t)r * K2 + c - K1];
                    CHECK(bits(out[(size_t)r * K + c]) == bits(want), "rows [%d][%d] scale %d%d", r, c, on1, on2);
                }
        }
    printf("row scale + concat: %d x (%d | %d), 4 scale choices\n", rows, K1, K2);
}

static void test_storage()
{
    const size_t n = 64;
    std::vector<float> v = distinct(n, 0.0371f);
    // (value bits, its bf16): quiet NaN, a NaN whose payload sits in the low half only (must not become infinity), +0, -0, above
    // the half-way point (rounds up), a tie below an even bf16 (stays), a tie below an odd bf16 (goes up to the even one), -(tie)
    const uint32_t special[8][2] = {{0x7FC00000u, 0x7FC0}, {0x7F800001u, 0x7FC0}, {0x00000000u, 0x0000}, {0x80000000u, 0x8000},
                                    {0x3F80C000u, 0x3F81}, {0x3F808000u, 0x3F80}, {0x3F818000u, 0x3F82}, {0xBF818000u, 0xBF82}};
    for (int i = 0; i < 8; ++i) v[(size_t)5 * i + 1] = from_bits(special[i][0]); // spread over both 32-value chunks
    v[40] = 3.14159265f; // low part non-zero
    auto want_bf16 = [&](size_t i) -> uint16_t {
        for (int s = 0; s < 8; ++s)
            if ((size_t)5 * s + 1 == i) return (uint16_t)special[s][1];
        return host_bf16(v[i]);
    };
    auto same = [](float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); };
    std::vector<uint16_t> buf;
    std::vector<float> back(n);

    CHECK(pack_storage_bytes(PACK_FP32, n) == 256 && pack_storage_bytes(PACK_BF16, n) == 128 && pack_storage_bytes(PACK_BF16X3, n) == 256, "storage bytes");
    const void *p = pack_storage(PACK_FP32, v.data(), n, buf);
    CHECK(memcmp(p, v.data(), 4 * n) == 0, "fp32 storage is the values as they are");
    unpack_storage(PACK_FP32, p, n, back.data());
    CHECK(memcmp(back.data(), v.data(), 4 * n) == 0, "fp32 round trip");

    p = pack_storage(PACK_BF16, v.data(), n, buf);
    CHECK(p == buf.data() && buf.size() == n, "bf16 storage size %zu", buf.size());
    unpack_storage(PACK_BF16, p, n, back.data());
    for (size_t i = 0; i < n; ++i) {
        CHECK(buf[i] == want_bf16(i), "bf16 [%zu]: 0x%08x -> 0x%04x", i, bits(v[i]), buf[i]);
        CHECK(bits(back[i]) == (uint32_t)buf[i] << 16, "bf16 round trip [%zu]", i);
        CHECK(bits(back[i]) == bits(host_from_bf16(host_bf16(v[i]))), "bf16 round trip [%zu] by host_bf16 / host_from_bf16", i);
    }
    CHECK(std::fabs(v[3] - back[3]) <= std::fabs(v[3]) / 256, "bf16 is within half a unit of 8 bits");

    p = pack_storage(PACK_BF16X3, v.data(), n, buf);
    CHECK(p == buf.data() && buf.size() == 2 * n, "split storage size %zu", buf.size());
    unpack_storage(PACK_BF16X3, p, n, back.data());
    for (size_t i = 0; i < n; ++i) {
        const uint16_t hi = buf[(i / 32) * 64 + i % 32], lo = buf[(i / 32) * 64 + 32 + i % 32];
        const float fhi = from_bits((uint32_t)hi << 16), flo = from_bits((uint32_t)lo << 16);
        CHECK(hi == want_bf16(i), "split hi [%zu]: 0x%04x", i, hi);
        CHECK(lo == host_bf16(v[i] - fhi), "split lo [%zu]: 0x%04x", i, lo);
        CHECK(same(back[i], fhi + flo), "split then join [%zu] is hi + lo", i);
        if (!std::isnan(v[i])) CHECK(std::fabs(back[i] - v[i]) <= std::fabs(v[i]) / 65536, "split [%zu] keeps 16 bits", i);
    }
    CHECK(buf[64 + 32 + 8] != 0, "the low part of %g is non-zero", v[40]);
    printf("storage: fp32, bf16, split bf16 of %zu values\n", n);
}

int main()
{
    test_ohwi(3, 5, 3);
    test_ohwi(3, 5, 1);
    test_stem();
    test_fold();
    test_rows();
    test_storage();
    printf("ok\n");
    return 0;
}
