// dist_tile_main.cpp -- the tile decode and tile count of imageclust_amd/csrc/dist_tile.h, which every distance kernel and its launcher
// share: a stand-alone host program (no GPU, no HIP) that tests/test_dist_tile_cpu.py builds with the address and
// undefined-behaviour sanitizers and runs.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/dist_tile.h"

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

static int64_t pairs_of(int64_t tr_lo, int64_t tr_hi) // |{(ti, tj): tr_lo <= ti < tr_hi, 0 <= tj <= ti}|, counted row by row
{
    int64_t n = 0;
    for (int64_t ti = tr_lo; ti < tr_hi; ++ti) n += ti + 1;
    return n;
}

// The decode maps [0, count) ONTO the launch's tiles, each exactly once; the host count is the number of tiles.
static int64_t check_bijection(int64_t tr_lo, int64_t tr_hi)
{
    const int64_t count = tri_tile_count(tr_lo, tr_hi), first = tr_lo * (tr_lo + 1) / 2;
    CHECK(count == pairs_of(tr_lo, tr_hi), "count of [%lld, %lld): %lld", (long long)tr_lo, (long long)tr_hi, (long long)count);
    std::vector<unsigned char> seen((size_t)count, 0);
    for (int64_t b = 0; b < count; ++b) {
        int ti = -1, tj = -1;
        tri_band_decode(b, tr_lo, tr_hi, ti, tj);
        CHECK(ti >= tr_lo && ti < tr_hi && tj >= 0 && tj <= ti, "[%lld, %lld) id %lld -> (%d, %d) outside the launch", (long long)tr_lo,
              (long long)tr_hi, (long long)b, ti, tj);
        const int64_t at = (int64_t)ti * (ti + 1) / 2 + tj - first; // row-major rank inside the launch: < count for a tile in range
        CHECK(!seen[(size_t)at], "[%lld, %lld) id %lld -> (%d, %d) a second time", (long long)tr_lo, (long long)tr_hi, (long long)b, ti, tj);
        seen[(size_t)at] = 1;
    }
    return count; // count distinct tiles in a set of count: onto
}

struct tile {
    int ti, tj;
};
// The order decides which tiles run together, so which operand panels an XCD's L2 holds: it must not move.  Tables: the decode of
// ward_dist_exact_kernel before the three copies became one, run on the host.
static const tile ORDER_0_10[] = {
    {0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}, {6, 0}, {7, 0}, {1, 1}, {2, 1}, {2, 2}, {3, 1},
    {3, 2}, {3, 3}, {4, 1}, {4, 2}, {4, 3}, {4, 4}, {5, 1}, {5, 2}, {5, 3}, {5, 4}, {5, 5}, {6, 1},
    {6, 2}, {6, 3}, {6, 4}, {6, 5}, {6, 6}, {7, 1}, {7, 2}, {7, 3}, {7, 4}, {7, 5}, {7, 6}, {7, 7},
    {8, 0}, {9, 0}, {8, 1}, {9, 1}, {8, 2}, {9, 2}, {8, 3}, {9, 3}, {8, 4}, {9, 4}, {8, 5}, {9, 5},
    {8, 6}, {9, 6}, {8, 7}, {9, 7}, {8, 8}, {9, 8}, {9, 9},
};
static const tile ORDER_3_12[] = {
    {3, 0}, {4, 0}, {5, 0}, {6, 0}, {7, 0}, {8, 0}, {9, 0}, {10, 0}, {3, 1}, {4, 1}, {5, 1}, {6, 1},
    {7, 1}, {8, 1}, {9, 1}, {10, 1}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {7, 2}, {8, 2}, {9, 2}, {10, 2},
    {3, 3}, {4, 3}, {5, 3}, {6, 3}, {7, 3}, {8, 3}, {9, 3}, {10, 3}, {4, 4}, {5, 4}, {5, 5}, {6, 4},
    {6, 5}, {6, 6}, {7, 4}, {7, 5}, {7, 6}, {7, 7}, {8, 4}, {8, 5}, {8, 6}, {8, 7}, {8, 8}, {9, 4},
    {9, 5}, {9, 6}, {9, 7}, {9, 8}, {9, 9}, {10, 4}, {10, 5}, {10, 6}, {10, 7}, {10, 8}, {10, 9}, {10, 10},
    {11, 0}, {11, 1}, {11, 2}, {11, 3}, {11, 4}, {11, 5}, {11, 6}, {11, 7}, {11, 8}, {11, 9}, {11, 10}, {11, 11},
};

template <size_t N> static void check_order(int64_t tr_lo, int64_t tr_hi, const tile (&want)[N])
{
    CHECK(tri_tile_count(tr_lo, tr_hi) == (int64_t)N, "table of [%lld, %lld) has %zu entries", (long long)tr_lo, (long long)tr_hi, N);
    for (size_t b = 0; b < N; ++b) {
        int ti = -1, tj = -1;
        tri_band_decode((int64_t)b, tr_lo, tr_hi, ti, tj);
        CHECK(ti == want[b].ti && tj == want[b].tj, "[%lld, %lld) id %zu -> (%d, %d), the table says (%d, %d)", (long long)tr_lo, (long long)tr_hi,
              b, ti, tj, want[b].ti, want[b].tj);
    }
}

int main()
{
    int64_t tiles = 0;
    const int64_t lows[] = {0, 1, 7, 8, 9, 13, 100};
    for (int64_t tr_lo : lows)
        for (int64_t span = 1; span <= 41; ++span) tiles += check_bijection(tr_lo, tr_lo + span);
    printf("small launches: 7 x 41 bijections, %lld tiles\n", (long long)tiles);

    tiles = check_bijection(0, 782) + check_bijection(0, 1954) + check_bijection(500, 782);
    printf("large launches: (0, 782), (0, 1954), (500, 782) bijections, %lld tiles\n", (long long)tiles);

    { // the largest triangle whose count fits a grid: its last ids decode into range (the sqrt guess is furthest from exact here)
        const int64_t T = 65535, count = tri_tile_count(0, T);
        CHECK(count == T * (T + 1) / 2 && count <= 0x7fffffffLL, "count of (0, 65535): %lld", (long long)count);
        for (int64_t b = count - 100000; b < count; ++b) {
            int ti = -1, tj = -1;
            tri_band_decode(b, 0, T, ti, tj);
            CHECK(ti >= 0 && ti < T && tj >= 0 && tj <= ti, "(0, 65535) id %lld -> (%d, %d)", (long long)b, ti, tj);
            tri_decode32(b, ti, tj);
            CHECK(tj >= 0 && tj <= ti && (int64_t)ti * (ti + 1) / 2 + tj == b, "row-major id %lld -> (%d, %d)", (long long)b, ti, tj);
        }
        for (int64_t b = 0; b < 100000; ++b) {
            int ti = -1, tj = -1;
            tri_decode32(b, ti, tj);
            CHECK(tj >= 0 && tj <= ti && (int64_t)ti * (ti + 1) / 2 + tj == b, "row-major id %lld -> (%d, %d)", (long long)b, ti, tj);
        }
        CHECK(tri_tile_count(0, 65536) == -1 && tri_tile_count(1, 65536) == -1, "a count past 2^31 - 1 must be refused");
        CHECK(tri_tile_count(5, 5) == 0, "an empty launch has no tiles");
        printf("grid limit: last 100000 ids of (0, 65535) in range, the row-major decode inverts its rank, larger counts refused\n");
    }

    check_order(0, 10, ORDER_0_10);
    check_order(3, 12, ORDER_3_12);
    printf("tile order: (0, 10) and (3, 12) as recorded\n");
    printf("ok\n");
    return 0;
}
