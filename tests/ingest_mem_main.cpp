// ingest_mem_main.cpp -- a memory source is never read past data[bytes - 1]: a stand-alone program over the host decoders (image_io.hip,
// jpeg_decode.hip, png_decode.hip compiled for the host alone), built and run under AddressSanitizer + UBSan by
// tests/test_ingest_mem_asan_cpu.py.  No GPU, no Python.
//
// For every file named on the command line: each prefix of its bytes, length 0 .. len, is copied into a fresh heap allocation of exactly
// that size and handed to icl_decode_image_mem (one byte past the allocation is the sanitizer's red zone); then 200 seeded single-byte
// mutations of the whole file, each again in an allocation of its own.  The whole file must decode; what the others return does not
// matter, only that every call comes back and the sanitizers stay silent.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/imageclust.h"

// what icl_core.hip gives the decoders in the library
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

static int decode_copy(const uint8_t *src, size_t n, int32_t *w, int32_t *h)
{
    uint8_t *own = (uint8_t *)malloc(n ? n : 1);
    if (!own) abort();
    if (n) memcpy(own, src, n);
    uint8_t *exact = n ? own : nullptr; // (length 0: no byte of the allocation belongs to the image)
    std::vector<uint8_t> rgb;
    int rc = icl_decode_image_mem(exact, (int64_t)n, nullptr, 0, w, h);
    if (rc == ICL_OK) {
        rgb.resize((size_t)*w * (size_t)*h * 3);
        rc = icl_decode_image_mem(exact, (int64_t)n, rgb.data(), (int64_t)rgb.size(), w, h);
    }
    free(own);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s image...\n", argv[0]);
        return 2;
    }
    for (int a = 1; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + got);
        fclose(f);
        int32_t w = 0, h = 0;
        if (file.empty() || decode_copy(file.data(), file.size(), &w, &h) != ICL_OK) {
            fprintf(stderr, "%s does not decode whole: %s\n", argv[a], g_err.c_str());
            return 1;
        }
        long ok = 0, empty = 0;
        for (size_t n = 0; n <= file.size(); ++n) {
            int32_t pw = 0, ph = 0;
            const int rc = decode_copy(file.data(), n, &pw, &ph);
            ok += rc == ICL_OK;
            empty += n == 0 && rc == ICL_ERR_IO && g_err.find("(in memory, 0 bytes). empty image buffer") != std::string::npos;
        }
        if (empty != 1) {
            fprintf(stderr, "%s: the empty prefix is not reported as an empty image buffer: %s\n", argv[a], g_err.c_str());
            return 1;
        }
        uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(a + 1);
        long mut_ok = 0;
        for (int k = 0; k < 200; ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> m(file);
            m[(size_t)((s >> 33) % m.size())] ^= (uint8_t)(1 + ((s >> 20) % 255));
            int32_t pw = 0, ph = 0;
            mut_ok += decode_copy(m.data(), m.size(), &pw, &ph) == ICL_OK;
        }
        printf("%s: %dx%d, %zu bytes: %ld of %zu prefixes and %ld of 200 mutations decode\n", argv[a], (int)w, (int)h, file.size(), ok, file.size() + 1, mut_ok);
    }
    printf("ok\n");
    return 0;
}
