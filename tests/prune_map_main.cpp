// prune_map_main.cpp -- the output-pixel map and the prune rule of the forward pass (imageclust_amd/csrc/prune_map.h): a stand-alone host
// program (no GPU, no HIP) that tests/test_prune_map_cpu.py builds with the address and undefined-behaviour sanitizers and runs.  The map
// is checked against the obvious triple loop over (b, oy, ox), tile by tile as conv_wr_kernel walks it (64-pixel tiles, M not a multiple
// of the tile, odd heights); the rule against the records of ResNet50-v1 and against records that must not be pruned.  Prints one line per
// group and a final "ok".
#include "../imageclust_amd/csrc/prune_map.h"

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

static icl_conv_rec rec(int cin, int cout, int k, int stride, int pad, int hin, int role, int stage, int block)
{
    icl_conv_rec r = {cin, cout, k, stride, pad, hin, (hin + 2 * pad - k) / stride + 1, role, stage, block};
    return r;
}

int main()
{
    // ---- the map: every compact pixel, in the kernel's tile order, against the triple loop
    long long pixels = 0;
    const int heights[] = {1, 2, 3, 7, 8, 10, 13, 14, 15, 28, 56};
    for (int s = 1; s <= 3; ++s)
        for (int H : heights)
            for (int W : {H, H + 1})
                for (int B : {1, 3, 5}) {
                    const prune_map pm = prune_map_make(s, H, W);
                    CHECK(pm.Ho == (H + s - 1) / s && pm.Wo == (W + s - 1) / s, "extent of %d x %d at stride %d: %d x %d", H, W, s, pm.Ho, pm.Wo);
                    CHECK((H + 2 - 3) / s + 1 == pm.Ho, "a 3x3 / pad 1 / stride %d convolution over %d rows gives other rows than the map: %d", s, H, pm.Ho);
                    std::vector<int64_t> want;
                    for (int b = 0; b < B; ++b)
                        for (int oy = 0; oy < pm.Ho; ++oy)
                            for (int ox = 0; ox < pm.Wo; ++ox) want.push_back(((int64_t)b * H + s * oy) * W + s * ox);
                    const int64_t M = (int64_t)B * pm.Ho * pm.Wo;
                    CHECK((int64_t)want.size() == M, "M");
                    std::vector<char> hit((size_t)B * H * W, 0);
                    const int PT = 64, ntiles = (int)((M + PT - 1) / PT);
                    for (int tile = 0; tile < ntiles; ++tile)
                        for (int r = 0; r < PT; ++r) { // rows beyond M are the kernel's out-of-range lanes: never mapped
                            const int64_t m = (int64_t)tile * PT + r;
                            if (m >= M) continue;
                            const int64_t p = prune_map_pixel(pm, (unsigned)m);
                            CHECK(p == want[(size_t)m], "s %d, %d x %d, B %d: pixel %lld maps to %lld, not %lld", s, H, W, B, (long long)m, (long long)p, (long long)want[(size_t)m]);
                            CHECK(p >= 0 && p < (int64_t)B * H * W && !hit[(size_t)p], "pixel %lld: %lld is outside the tensor or taken", (long long)m, (long long)p);
                            hit[(size_t)p] = 1;
                            ++pixels;
                        }
                    for (int b = 0; b < B; ++b) // exactly the pixels whose row and column are multiples of s
                        for (int y = 0; y < H; ++y)
                            for (int x = 0; x < W; ++x)
                                CHECK(hit[((size_t)b * H + y) * W + x] == (y % s == 0 && x % s == 0), "s %d, %d x %d: pixel (%d, %d, %d)", s, H, W, b, y, x);
                }
    printf("map: %lld compact pixels equal the triple loop, each full pixel hit once iff both coordinates are multiples of s\n", pixels);

    // ---- the rule on ResNet50-v1: the last identity block of stages 1-3 stands in front of a strided block 0
    const int widths[5] = {0, 64, 128, 256, 512}, heights_of[5] = {0, 56, 28, 14, 7}, nblocks[5] = {0, 3, 4, 6, 3};
    int pruned = 0, asked = 0;
    for (int st = 1; st <= 4; ++st)
        for (int blk = 0; blk < nblocks[st]; ++blk) {
            const int mid = widths[st], h = heights_of[st];
            const icl_conv_rec c2 = rec(mid, mid, 3, 1, 1, h, 2, st, blk), c3 = rec(mid, 4 * mid, 1, 1, 0, h, 3, st, blk);
            const bool last = blk == nblocks[st] - 1;
            icl_conv_rec n1, nd;
            if (last && st < 4) {
                n1 = rec(4 * mid, 2 * mid, 1, 2, 0, h, 1, st + 1, 0);
                nd = rec(4 * mid, 8 * mid, 1, 2, 0, h, 4, st + 1, 0);
            } else { // the next block of the same stage: what stands three records further is its c1's successor, not a downsample
                n1 = rec(4 * mid, mid, 1, 1, 0, h, 1, st, blk + 1);
                nd = rec(mid, mid, 3, 1, 1, h, 2, st, blk + 1);
            }
            const bool stage4_end = last && st == 4;
            const int s = stage4_end ? prune_stride(c2, c3, nullptr, nullptr) : prune_stride(c2, c3, &n1, &nd);
            const int want = (last && st < 4 && blk > 0) ? 2 : 0;
            CHECK(s == want, "stage %d block %d: stride %d, not %d", st, blk, s, want);
            pruned += s > 0;
            ++asked;
        }
    CHECK(pruned == 3 && asked == 16, "%d of %d blocks", pruned, asked);
    printf("rule: the last block of stages 1, 2 and 3 at stride 2, none of the other 13\n");

    // ---- ... and what must not be pruned: each condition of the rule, one at a time
    const icl_conv_rec c2 = rec(128, 128, 3, 1, 1, 28, 2, 2, 3), c3 = rec(128, 512, 1, 1, 0, 28, 3, 2, 3);
    const icl_conv_rec n1 = rec(512, 256, 1, 2, 0, 28, 1, 3, 0), nd = rec(512, 1024, 1, 2, 0, 28, 4, 3, 0);
    CHECK(prune_stride(c2, c3, &n1, &nd) == 2, "the base case");
    struct { const char *what; icl_conv_rec a2, a3, b1, bd; } bad[] = {
        {"a c1 of stride 1 (ResNet v1.5 keeps the stride on c2)", c2, c3, rec(512, 256, 1, 1, 0, 28, 1, 3, 0), nd},
        {"c1 and the downsample at different strides", c2, c3, n1, rec(512, 1024, 1, 3, 0, 28, 4, 3, 0)},
        {"a 3x3 downsample", c2, c3, n1, rec(512, 1024, 3, 2, 1, 28, 4, 3, 0)},
        {"a padded c1", c2, c3, rec(512, 256, 1, 2, 1, 28, 1, 3, 0), nd},
        {"a reader of another tensor", c2, c3, rec(512, 256, 1, 2, 0, 14, 1, 3, 0), nd},
        {"a block 0 in front (its c3 runs in the dual-operand launch)", c2, rec(128, 512, 1, 1, 0, 28, 3, 2, 0), n1, nd},
        {"a 1x1 c2", rec(128, 128, 1, 1, 0, 28, 2, 2, 3), c3, n1, nd},
        {"a strided c2", rec(128, 128, 3, 2, 1, 56, 2, 2, 3), c3, n1, nd},
        {"an unpadded c2", rec(128, 128, 3, 1, 0, 30, 2, 2, 3), c3, n1, nd},
        {"a successor that is no block 0", c2, c3, rec(512, 256, 1, 2, 0, 28, 1, 3, 1), nd},
        {"a successor without a downsample record", c2, c3, n1, rec(256, 256, 3, 1, 1, 14, 2, 3, 0)},
    };
    for (const auto &t : bad) CHECK(prune_stride(t.a2, t.a3, &t.b1, &t.bd) == 0, "%s is pruned", t.what);
    CHECK(prune_stride(c2, c3, &n1, nullptr) == 0 && prune_stride(c2, c3, nullptr, &nd) == 0, "a missing record");
    printf("refused: %d records that break one condition each\n", (int)(sizeof bad / sizeof bad[0]));
    printf("ok\n");
    return 0;
}
