// fold_plan_main.cpp -- the host rules of imageclust_amd/csrc/fold_plan.h (what icl_fold_centroids refuses, the groups' item totals, the
// launch geometry): a stand-alone host program (no GPU, no HIP) that tests/test_fold_centroids_cpu.py builds with the address and
// undefined-behaviour sanitizers and runs.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/fold_plan.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static bool says(const char *why, const char *part) { return why && strstr(why, part); }

// every column of every group has exactly one owner, inside the matrix; no workgroup is wider than its launch bound
static void check_geometry(int64_t K, int32_t d, bool aligned, int cus)
{
    const fold_geom g = fold_geometry(K, d, aligned, cus);
    CHECK(g.vec == (aligned && d % 4 == 0) && g.per == (g.vec ? 4 : 1), "K %lld d %d: form", (long long)K, d);
    CHECK(g.threads >= FOLD_WAVE && g.threads <= FOLD_THREADS && g.threads % FOLD_WAVE == 0, "K %lld d %d: %d threads", (long long)K, d, g.threads);
    CHECK(g.cols == g.threads * g.per, "K %lld d %d: cols", (long long)K, d);
    CHECK(g.chunks >= 1 && g.chunks * g.cols >= d && (g.chunks - 1) * g.cols < d, "K %lld d %d: %lld chunks of %d", (long long)K, d, (long long)g.chunks, g.cols);
    CHECK(g.blocks == K * g.chunks && g.grid <= g.blocks && g.grid * g.threads <= 0xffffffffLL && (K == 0 || g.grid >= 1), "K %lld d %d: grid", (long long)K, d);
    std::vector<int> owners((size_t)d, 0);
    for (int64_t ch = 0; ch < g.chunks; ++ch)
        for (int t = 0; t < g.threads; ++t) {
            const int64_t col = (ch * g.threads + t) * g.per; // fold_kernel's column of thread t in chunk ch
            if (col >= d) continue;
            CHECK(col + g.per <= d, "K %lld d %d: thread %d of chunk %lld crosses the row's end", (long long)K, d, t, (long long)ch);
            for (int e = 0; e < g.per; ++e) owners[(size_t)(col + e)]++;
        }
    for (int32_t k = 0; k < d; ++k) CHECK(owners[(size_t)k] == 1, "K %lld d %d: column %d has %d owners", (long long)K, d, k, owners[(size_t)k]);
}

// with arguments "K d aligned compute_units": the geometry of that call, for tests/fold_cases.geometry to be held against
int main(int argc, char **argv)
{
    if (argc == 5) {
        const fold_geom g = fold_geometry(atoll(argv[1]), atoi(argv[2]), atoi(argv[3]) != 0, atoi(argv[4]));
        printf("%d %d %lld %lld\n", g.vec, g.threads, (long long)g.chunks, (long long)g.grid);
        return 0;
    }
    const float E[12] = {0};
    float C[8];
    const int64_t rp[4] = {0, 2, 2, 5};
    const int32_t mb[5] = {0, 3, 3, 1, 2};
    const int32_t sz[4] = {1, 2, 3, 4};
    int64_t rows = -1, longest = -1;

    // 1. an accepted call, its totals and figures
    CHECK(!fold_bad_arg(E, sz, 4, 3, rp, mb, 3, C, &rows, &longest) && rows == 5 && longest == 3, "accepted call: rows %lld longest %lld", (long long)rows, (long long)longest);
    CHECK(!fold_bad_arg(E, nullptr, 4, 3, rp, mb, 3, C), "accepted call without sizes");
    int32_t tot[3] = {-1, -1, -1};
    fold_totals(sz, rp, mb, 3, tot);
    CHECK(tot[0] == 5 && tot[1] == 0 && tot[2] == 9, "totals %d %d %d", tot[0], tot[1], tot[2]);
    fold_totals(nullptr, rp, mb, 3, tot);
    CHECK(tot[0] == 2 && tot[1] == 0 && tot[2] == 3, "unsized totals %d %d %d", tot[0], tot[1], tot[2]);
    CHECK(!fold_bad_arg(nullptr, nullptr, 0, 1, nullptr, nullptr, 0, nullptr, &rows, &longest) && rows == 0 && longest == 0, "K == 0 needs no array");
    const int64_t rp0[3] = {0, 0, 0};
    CHECK(!fold_bad_arg(nullptr, nullptr, 0, 3, rp0, nullptr, 2, C, &rows), "empty groups need neither E nor member");
    printf("accepted calls: 4\n");

    // 2. every refusal
    int refusals = 0;
#define REFUSED(part, ...)                                                             \
    do {                                                                               \
        CHECK(says(fold_bad_arg(__VA_ARGS__), part), "not refused as \"%s\"", part);   \
        ++refusals;                                                                    \
    } while (0)
    REFUSED("negative", E, sz, -1, 3, rp, mb, 3, C);
    REFUSED("negative", E, sz, 4, 3, rp, mb, -1, C);
    REFUSED("2^31", E, sz, 4, 3, rp, mb, 1LL << 31, C);
    REFUSED("d must", E, sz, 4, 0, rp, mb, 3, C);
    REFUSED("null", E, sz, 4, 3, nullptr, mb, 3, C);
    REFUSED("null", E, sz, 4, 3, rp, mb, 3, nullptr);
    REFUSED("null", E, sz, 4, 3, rp, nullptr, 3, C);
    REFUSED("null", nullptr, sz, 4, 3, rp, mb, 3, C);
    const int64_t rp1[4] = {1, 2, 2, 5}, rpd[4] = {0, 3, 2, 5};
    REFUSED("row_ptr[0]", E, sz, 4, 3, rp1, mb, 3, C);
    REFUSED("decreases", E, sz, 4, 3, rpd, mb, 3, C);
    const int32_t mlo[5] = {0, 3, -1, 1, 2}, mhi[5] = {0, 3, 3, 1, 4};
    REFUSED("member", E, sz, 4, 3, rp, mlo, 3, C);
    REFUSED("member", E, sz, 4, 3, rp, mhi, 3, C);
    REFUSED("member", E, sz, 0, 3, rp, mb, 3, C);
    const int32_t s0[4] = {1, 0, 3, 4}, sneg[4] = {1, 2, 3, -4};
    REFUSED("size", E, s0, 4, 3, rp, mb, 3, C);
    REFUSED("size", E, sneg, 4, 3, rp, mb, 3, C);
    const int32_t shuge[4] = {INT32_MAX, 1, 1, INT32_MAX}; // group 0: rows 0 and 3
    REFUSED("INT32_MAX", E, shuge, 4, 3, rp, mb, 3, C);
    const int32_t sedge[4] = {INT32_MAX - 1, 1, 1, 1};
    CHECK(!fold_bad_arg(E, sedge, 4, 3, rp, mb, 3, C), "a total of exactly INT32_MAX is accepted");
    printf("refusals: %d\n", refusals);

    // 3. the geometry over the shapes the GPU tests run and a sweep around them
    const int32_t widths[] = {1, 3, 4, 8, 255, 256, 257, 1023, 1024, 1025, 1037, 2048, 2052, 4096, 5000};
    const int64_t counts[] = {0, 1, 2, 22, 300, 1024, 11000, 70000};
    int shapes = 0;
    for (int32_t d : widths)
        for (int64_t K : counts)
            for (int aligned = 0; aligned < 2; ++aligned)
                for (int cus : {0, 1, 256, 304}) {
                    check_geometry(K, d, aligned != 0, cus);
                    ++shapes;
                }
    // few groups narrow the workgroups, many keep them wide; a misaligned pointer or an odd width takes the scalar form
    const fold_geom one = fold_geometry(1, 2048, true, 256), lib = fold_geometry(11000, 2048, true, 256), odd = fold_geometry(22, 8, false, 256);
    CHECK(one.vec && one.threads == FOLD_WAVE && one.chunks == 8, "one long group: %d threads, %lld chunks", one.threads, (long long)one.chunks);
    CHECK(lib.vec && lib.threads == FOLD_THREADS && lib.chunks == 2 && lib.grid == 22000, "library shape: %d threads, %lld chunks", lib.threads, (long long)lib.chunks);
    CHECK(!odd.vec && odd.per == 1 && odd.chunks == 1, "misaligned: scalar form");
    CHECK(!fold_geometry(22, 1037, true, 256).vec && fold_geometry(22, 1037, true, 256).chunks > 1, "odd width: scalar form, several chunks");
    CHECK(fold_geometry(70000, 3, true, 256).grid == 70000, "70 000 groups: one workgroup each");
    // the shapes the GPU tests run with several waves per workgroup (256 compute units): four waves in both forms, with dead tail lanes
    // at d = 2052 and d = 1037, and two waves
    CHECK(fold_geometry(1100, 2048, true, 256).threads == 256 && fold_geometry(1100, 2052, true, 256).threads == 256, "K 1100: 256 threads, 16-byte form");
    CHECK(fold_geometry(1100, 2052, true, 256).chunks == 3 && fold_geometry(1100, 1037, true, 256).chunks == 5, "K 1100: chunks with a dead tail");
    CHECK(fold_geometry(1100, 1037, true, 256).threads == 256 && fold_geometry(1100, 2048, false, 256).threads == 256, "K 1100: 256 threads, scalar form");
    CHECK(fold_geometry(300, 2048, true, 256).threads == 128 && fold_geometry(300, 2052, true, 256).threads == 128, "K 300: 128 threads");
    // more blocks than one launch may hold threads for: the grid is cut and the workgroups walk
    const fold_geom huge = fold_geometry((1LL << 31) - 1, 5000, false, 256);
    CHECK(huge.blocks > huge.grid && huge.grid == 0xffffffffLL / huge.threads, "grid cut at 2^32 threads");
    printf("geometry: %d shapes\n", shapes);
    printf("ok\n");
    return 0;
}
