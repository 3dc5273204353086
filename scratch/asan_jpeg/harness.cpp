// CPU AddressSanitizer harness for the host-only JPEG decoder (sanitizers run on the CPU build only).
#include <cstdio>
#include <cstdint>
#include <vector>
struct icl_ctx;
// stage A (parse + entropy decode) then stage B (IDCT, upsampling, colour) of jpeg_decode.hip
int icl_jpeg_decode(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, std::vector<uint8_t> &rgb, int &W, int &H, int &orient);
// stage A0 + the GPU entropy decoder's schedule as a host loop (jpeg_entropy.h): the same damaged files go through it
int icl_jpeg_entropy_host_check(const uint8_t *data, size_t len, const char *path);
int main(int argc, char **argv)
{
    int ok = 0, bad = 0, acc = 0;
    for (int i = 1; i < argc; ++i) {
        FILE *f = fopen(argv[i], "rb");
        if (!f) continue;
        std::vector<uint8_t> d;
        int c;
        while ((c = fgetc(f)) != EOF) d.push_back((uint8_t)c);
        fclose(f);
        std::vector<uint8_t> rgb;
        int w, h, orient;
        (icl_jpeg_decode(nullptr, d.data(), d.size(), argv[i], rgb, w, h, orient) == 0 ? ok : bad)++;
        acc += icl_jpeg_entropy_host_check(d.data(), d.size(), argv[i]) == 1;
    }
    printf("decoded %d, rejected %d; subsequence decoder accepted %d\n", ok, bad, acc);
}
