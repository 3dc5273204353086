// downsize_asan_main.cpp -- the host JPEG encoder and downsizer under AddressSanitizer + UBSan: a stand-alone program over jpeg_encode.hip
// and the host decoders (image_io.hip, jpeg_decode.hip, png_decode.hip compiled for the host alone), built and run by
// tests/test_downsize_asan_cpu.py.  No GPU, no Python.
//
//   encode W H Q SEED   a seeded noise / gradient image of W x H in a heap allocation of exactly W*H*3 bytes (one byte past it is the
//                       sanitizer's red zone) through icl_jpeg_encode_rgb into an allocation of exactly the size it reported; prints
//                       the size and an FNV-1a hash of the file
//   downsize MAX_BYTES MAX_DIM file...   every file through icl_downsize_image_file and, from an exact-size copy, icl_downsize_image_mem
//                       (outputs in exact-size allocations); both must agree; prints each result's code, size and hash
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/imageclust.h"

// what icl_core.hip gives the host code in the library
static thread_local std::string g_err;
int icl_fail(icl_ctx *, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
extern "C" const char *icl_last_error(icl_ctx *) { return g_err.c_str(); }

static uint64_t fnv(const uint8_t *p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static int encode(int w, int h, int q, uint64_t seed)
{
    const size_t n = (size_t)w * (size_t)h * 3;
    uint8_t *px = (uint8_t *)malloc(n);
    if (!px) abort();
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (size_t i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        px[i] = (seed & 1) ? (uint8_t)(s >> 56) : (uint8_t)((i / 3 % (size_t)w) * 255 / (size_t)w);
    }
    int64_t need = 0, got = 0;
    int rc = icl_jpeg_encode_rgb(px, w, h, q, nullptr, 0, &need);
    if (rc == ICL_OK) {
        if (need > icl_jpeg_encode_bound(w, h)) {
            fprintf(stderr, "%dx%d q%d: %lld bytes above the bound %lld\n", w, h, q, (long long)need, (long long)icl_jpeg_encode_bound(w, h));
            return 1;
        }
        uint8_t *out = (uint8_t *)malloc((size_t)need);
        if (!out) abort();
        rc = icl_jpeg_encode_rgb(px, w, h, q, out, need, &got);
        if (rc == ICL_OK) printf("encode %dx%d q%d: %lld bytes %016llx\n", w, h, q, (long long)got, (unsigned long long)fnv(out, (size_t)got));
        free(out);
    }
    free(px);
    if (rc != ICL_OK || got != need) {
        fprintf(stderr, "encode %dx%d q%d failed: %d %s\n", w, h, q, rc, g_err.c_str());
        return 1;
    }
    return 0;
}

template <class Call> static int run(const Call &call, std::vector<uint8_t> &file, int32_t info[6])
{
    int64_t need = 0, got = 0;
    int rc = call(nullptr, 0, &need, info);
    if (rc != ICL_OK) return rc;
    uint8_t *out = (uint8_t *)malloc(need ? (size_t)need : 1);
    if (!out) abort();
    rc = call(out, need, &got, info);
    if (rc == ICL_OK) file.assign(out, out + got);
    free(out);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "encode")) return encode(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), (uint64_t)atoll(argv[5]));
    if (argc < 5 || strcmp(argv[1], "downsize")) {
        fprintf(stderr, "usage: %s encode W H Q SEED | downsize MAX_BYTES MAX_DIM file...\n", argv[0]);
        return 2;
    }
    const int64_t max_bytes = atoll(argv[2]);
    const int32_t max_dim = atoi(argv[3]);
    for (int a = 4; a < argc; ++a) {
        std::vector<uint8_t> src, f1, f2;
        if (FILE *f = fopen(argv[a], "rb")) {
            uint8_t chunk[4096];
            for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) src.insert(src.end(), chunk, chunk + got);
            fclose(f);
        }
        uint8_t *own = (uint8_t *)malloc(src.empty() ? 1 : src.size()); // the memory twin reads an allocation of exactly the file's size
        if (!own) abort();
        if (!src.empty()) memcpy(own, src.data(), src.size());
        int32_t i1[6] = {0}, i2[6] = {0};
        const int r1 = run([&](uint8_t *o, int64_t c, int64_t *n, int32_t *i) { return icl_downsize_image_file(argv[a], max_bytes, max_dim, o, c, n, i); }, f1, i1);
        const int r2 = run([&](uint8_t *o, int64_t c, int64_t *n, int32_t *i) { return icl_downsize_image_mem(src.empty() ? nullptr : own, (int64_t)src.size(), max_bytes, max_dim, o, c, n, i); }, f2, i2);
        free(own);
        if (r1 != r2 || f1 != f2 || memcmp(i1, i2, sizeof i1)) {
            fprintf(stderr, "%s: the file call (%d, %zu bytes) and the memory call (%d, %zu bytes) differ\n", argv[a], r1, f1.size(), r2, f2.size());
            return 1;
        }
        printf("downsize %s: rc %d, %zu bytes %016llx, attempts %d\n", argv[a], r1, f1.size(), (unsigned long long)fnv(f1.data(), f1.size()), (int)i1[5]);
    }
    printf("ok\n");
    return 0;
}
