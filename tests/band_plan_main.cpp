// band_plan_main.cpp -- the column-split decision of the band walk (imageclust_amd/csrc/band_plan.h), which icl_nearest and
// icl_cluster_fit share: a stand-alone host program (no GPU, no HIP) that tests/test_band_plan_cpu.py builds with the address and
// undefined-behaviour sanitizers and runs.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/band_plan.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);    \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, " [%s]\n", #cond);                 \
            exit(1);                                           \
        }                                                      \
    } while (0)

static int64_t lo(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t hi(int64_t a, int64_t b) { return a > b ? a : b; }

int main()
{
    const int forced[] = {1, 2, 3, 6, 7, 1023, 1024, 1025, 100000, INT_MAX};
    const int cus[] = {1, 256};
    long long checked = 0;
    std::vector<int64_t> tiles = {1023, 1024, 1025, 2000}; // the cap's edge, then 0 .. 9 and every 37th up to 2000
    for (int64_t t = 0; t <= 2000; t += t < 10 ? 1 : 37) tiles.push_back(t);
    for (int64_t nbands = 1; nbands <= 600; ++nbands)
        for (int64_t ntiles : tiles) {
            const int64_t cap = hi(1, lo(ntiles, 1024));
            for (int cu : cus) {
                for (int f : forced) { // a forced count holds up to one tile per split, whatever the device
                    const int s = band_splits(f, cu, nbands, ntiles);
                    CHECK(s == lo(f, cap), "forced %d, %lld bands, %lld tiles: %d", f, (long long)nbands, (long long)ntiles, s);
                    CHECK(s >= 1 && s <= hi(1, ntiles), "forced %d, %lld tiles: %d is outside [1, max(1, tiles)]", f, (long long)ntiles, s);
                }
                const int s = band_splits(0, cu, nbands, ntiles); // the engine decides: about two workgroups per CU in one round
                const int64_t want = nbands >= 2 * cu ? 1 : hi(1, lo(2 * cu / nbands, cap));
                CHECK(s == want, "auto, %d CUs, %lld bands, %lld tiles: %d, not %lld", cu, (long long)nbands, (long long)ntiles, s, (long long)want);
                CHECK(s >= 1 && s <= hi(1, ntiles), "auto, %lld tiles: %d is outside [1, max(1, tiles)]", (long long)ntiles, s);
                checked += 11;
            }
        }
    printf("forced: min(f, max(1, min(tiles, 1024)))\n");
    printf("auto: 1 from 2 x CUs bands on, else max(1, min(2 x CUs / bands, cap))\n");
    // a device that reports no CU counts as one; the shape of SPLIT_CASE in tests/fit_cases.py (one band, six tiles) on 256 CUs
    CHECK(band_splits(0, 0, 1, 6) == 2 && band_splits(0, -3, 2, 6) == 1, "a CU count below 1 is read as 1");
    CHECK(band_splits(0, 256, 1, 6) == 6 && band_splits(7, 256, 1, 6) == 6 && band_splits(3, 256, 1, 6) == 3, "one band, six tiles");
    printf("range: every result in [1, max(1, tiles)] (%lld decisions)\n", checked);
    printf("ok\n");
    return 0;
}
