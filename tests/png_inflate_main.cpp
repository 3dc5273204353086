// png_inflate_main.cpp -- the GPU PNG route's schedule (png_inflate.h, run as a host loop by png_decode.hip) stays inside its buffers: a
// stand-alone program over the host decoders compiled for the host alone, built and run under AddressSanitizer + UBSan by
// tests/test_png_gpu_schedule_asan_cpu.py.  No GPU, no Python.
//
// usage: png_inflate_main SWEEP file...   Every file goes through icl_png_raw_mem_host at stages 0, 1 and 2, from a heap allocation of
// exactly its size into one of exactly the size the call asked for (one byte past either is the sanitizer's red zone).  The first SWEEP
// files (one IDAT chunk each) are also swept: every prefix of the file; every prefix of the zlib stream, re-framed with correct CRCs so
// that it reaches the inflate loop; and 200 seeded single-byte mutations of the file, each with its CRCs recomputed.  What the calls return
// does not matter beyond "no error code"; the sanitizers must stay silent.
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

static uint32_t crc32_of(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return c ^ 0xffffffffu;
}
static uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static void put32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}
// every chunk whose length field still fits gets the CRC of what it now holds
static void fix_crcs(std::vector<uint8_t> &f)
{
    size_t pos = 8;
    while (pos + 12 <= f.size()) {
        const uint32_t n = be32(f.data() + pos);
        if ((size_t)n > f.size() - pos - 12) break;
        put32(f.data() + pos + 8 + n, crc32_of(f.data() + pos + 4, 4 + (size_t)n));
        pos += 12 + (size_t)n;
    }
}
// where the (first) IDAT chunk starts and how long its body is; false: none
static bool find_idat(const std::vector<uint8_t> &f, size_t &at, uint32_t &n)
{
    size_t pos = 8;
    while (pos + 12 <= f.size()) {
        n = be32(f.data() + pos);
        if ((size_t)n > f.size() - pos - 12) return false;
        if (!memcmp(f.data() + pos + 4, "IDAT", 4)) {
            at = pos;
            return true;
        }
        pos += 12 + (size_t)n;
    }
    return false;
}

static long g_calls = 0, g_accepted = 0;

// stages 0, 1, 2 of one image held in an exact allocation; returns the state of stage 1, or -2 on an error code
static int run_exact(const uint8_t *src, size_t n)
{
    uint8_t *own = (uint8_t *)malloc(n ? n : 1);
    if (!own) abort();
    if (n) memcpy(own, src, n);
    int state1 = -2;
    for (int stage = 0; stage < 3; ++stage) {
        int64_t need = 0;
        int32_t info[12];
        if (icl_png_raw_mem_host(own, (int64_t)n, stage, nullptr, 0, &need, info) != ICL_OK) {
            free(own);
            return -2;
        }
        uint8_t *out = (uint8_t *)malloc(need ? (size_t)need : 1);
        if (!out) abort();
        const int rc = icl_png_raw_mem_host(own, (int64_t)n, stage, out, need, &need, info);
        free(out);
        if (rc != ICL_OK) {
            free(own);
            return -2;
        }
        ++g_calls;
        g_accepted += info[0] == 1;
        if (stage == 1) state1 = info[0];
    }
    free(own);
    return state1;
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s SWEEP file...\n", argv[0]);
        return 2;
    }
    const int sweep = atoi(argv[1]);
    for (int a = 2; a < argc; ++a) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<uint8_t> file;
        uint8_t chunk[4096];
        for (size_t got; (got = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + got);
        fclose(f);
        const int whole = run_exact(file.data(), file.size());
        if (whole == -2) {
            fprintf(stderr, "%s: %s\n", argv[a], g_err.c_str());
            return 1;
        }
        if (a - 2 >= sweep) {
            printf("%s: state %d\n", argv[a], whole);
            continue;
        }
        size_t at = 0;
        uint32_t zn = 0;
        if (whole != 1 || !find_idat(file, at, zn)) {
            fprintf(stderr, "%s: a swept file must be accepted whole and hold an IDAT chunk\n", argv[a]);
            return 1;
        }
        long bad = 0;
        for (size_t n = 0; n <= file.size(); ++n) bad += run_exact(file.data(), n) == -2;
        for (uint32_t k = 0; k <= zn; ++k) { // the zlib stream cut to k bytes, in a well-formed file
            std::vector<uint8_t> m(file.begin(), file.begin() + (long)at);
            m.resize(at + 12 + k);
            put32(m.data() + at, k);
            memcpy(m.data() + at + 4, "IDAT", 4);
            memcpy(m.data() + at + 8, file.data() + at + 8, k);
            const uint8_t iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
            m.insert(m.end(), iend, iend + 12);
            fix_crcs(m);
            bad += run_exact(m.data(), m.size()) == -2;
        }
        uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(a + 1);
        long mut_ok = 0;
        for (int k = 0; k < 200; ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            std::vector<uint8_t> m(file);
            m[(size_t)((s >> 33) % m.size())] ^= (uint8_t)(1 + ((s >> 20) % 255));
            fix_crcs(m);
            const int st = run_exact(m.data(), m.size());
            bad += st == -2;
            mut_ok += st == 1;
        }
        if (bad) {
            fprintf(stderr, "%s: %ld calls returned an error code: %s\n", argv[a], bad, g_err.c_str());
            return 1;
        }
        printf("%s: swept, %zu bytes, stream %u bytes, %ld of 200 mutations accepted\n", argv[a], file.size(), zn, mut_ok);
    }
    printf("calls %ld accepted %ld\nok\n", g_calls, g_accepted);
    return 0;
}
