// ws_layout_main.cpp -- icl_ws_layout (imageclust_amd/csrc/icl_ws_layout.h), the bump layout every grow-only workspace of the library
// places its pieces with: a stand-alone host program (no GPU, no HIP) that tests/test_ws_layout_cpu.py builds with the address and
// undefined-behaviour sanitizers and runs.  Prints one line per rule and a final "ok".
//
// The expected offsets and totals of the three shapes are literals, worked out by hand from the expressions the units used before
// they shared this type (up16(b) = (b + 15) & ~15 and hand-summed offsets in pairs.hip and nearest.hip; (b + 255) / 256 * 256 pieces
// in requests.hip): the workspace sizes icl_last_pairs_stats / icl_last_nearest_stats report must not move.
#include "../imageclust_amd/csrc/icl_ws_layout.h"

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

// take() returns aligned offsets, each advancing by the size rounded up; a piece of 0 bytes takes no room
static void check_steps(size_t align)
{
    const size_t sizes[] = {1, align - 1, align, align + 1, 0, 3 * align, 0, 0, 7, 1000003, 0, 5 * align + 2};
    icl_ws_layout L(align);
    CHECK(L.total == 0, "a fresh layout holds %zu bytes", L.total);
    size_t expect = 0;
    for (size_t b : sizes) {
        const size_t at = L.take(b), rounded = (b + align - 1) / align * align;
        CHECK(at == expect, "align %zu: a piece of %zu bytes lies at %zu, not %zu", align, b, at, expect);
        CHECK(at % align == 0, "align %zu: offset %zu", align, at);
        CHECK(rounded >= b && rounded < b + align && rounded % align == 0, "align %zu: %zu rounds to %zu", align, b, rounded);
        expect += rounded;
        CHECK(L.total == expect, "align %zu: total %zu after a piece of %zu bytes, not %zu", align, L.total, b, expect);
        if (b == 0) CHECK(L.total == at, "align %zu: an empty piece took %zu bytes", align, L.total - at);
    }
}

static void check_shape(const char *name, size_t align, const std::vector<size_t> &pieces, const std::vector<size_t> &offsets, size_t total)
{
    icl_ws_layout L(align);
    for (size_t i = 0; i < pieces.size(); ++i) {
        const size_t at = L.take(pieces[i]);
        CHECK(at == offsets[i], "%s: piece %zu (%zu bytes) lies at %zu, not %zu", name, i, pieces[i], at, offsets[i]);
    }
    CHECK(L.total == total, "%s: %zu bytes in all, not %zu", name, L.total, total);
}

int main()
{
    check_steps(16);
    check_steps(256);
    printf("steps: aligned offsets, rounded sizes, empty pieces take no room (alignments 16 and 256)\n");

    // icl_pairs_within, n = 129 with sizes: T = 2 tile rows, 3 tiles.  [size 516] [row_count 516] [totals 16] [hit 3] [row_ptr 1040] [tile rows 8]
    //   up16: 528 + 528 + 16 + 16 + 1040 + 16 = 2144; the memset over row_count | totals | hit covers 528 .. 1088
    check_shape("pairs n=129", 16, {516, 516, 16, 3, 1040, 8}, {0, 528, 1056, 1072, 1088, 2128}, 2144);
    // ... and without sizes: the first piece is empty and everything moves down by 528
    check_shape("pairs n=129, no sizes", 16, {0, 516, 16, 3, 1040, 8}, {0, 0, 528, 544, 560, 1600}, 1616);
    // icl_nearest, nq = 130, n = 257, k = 64, two splits, q_size / e_size / exclude given:
    //   [q_size 520] [e_size 1028] [exclude 520] then two partial lists of 2 * 130 * 64 * 4 = 66560 bytes: 528 + 1040 + 528 + 2 * 66560 = 135216
    check_shape("nearest nq=130 n=257 k=64 splits=2", 16, {520, 1028, 520, 66560, 66560}, {0, 528, 1568, 2096, 68656}, 135216);
    // ... one split and no metadata: no workspace at all
    check_shape("nearest, nothing to hold", 16, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}, 0);
    // icl_cluster_requests, one request of 3 images, head = 1000, a label set of 7 (d = 1007), 5 label entries in all:
    //   [E 3 * 1007 * 4 = 12084] [dense rows 3 * 1000 * 4 = 12000] [image table 3 * 16] [label_off 4 * 8] [label_idx 5 * 4]
    //   in 256-byte pieces: 12288 + 12032 + 256 + 256 + 256 = 25088
    check_shape("requests rows=3 head=1000 labels=5", 256, {12084, 12000, 48, 32, 20}, {0, 12288, 24320, 24576, 24832}, 25088);
    printf("shapes: the offsets and totals of the earlier expressions (pairs, nearest, requests)\n");
    printf("ok\n");
    return 0;
}
