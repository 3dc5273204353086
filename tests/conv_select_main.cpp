// conv_select_main.cpp -- the kernel choice and the forward plan (imageclust_amd/csrc/conv_select.h): a stand-alone host program (no GPU, no
// HIP) that tests/test_conv_select_cpu.py builds with the address and undefined-behaviour sanitizers and runs.  It prints what the header
// decides; the Python side compares that with its own restatement of the rule (tests/conv_exact.py: route, wr_rule) and with a recorded
// launch listing.  The kernel names are formatted here: the header holds no strings.
//   topo                                  the records of ResNet50-v1, one per line
//   choose FILE                           FILE: lines "prec B H cin cout k stride pad res p8 split ncu" -> one choice per line
//   plan prec B ncu dense tap fuse prune p8 split stem_per_cu [stem_max_blocks]   -> one step per line, then "out <buffer> <H> <C> pruned <n>"
//   refuse                                conv_same_arithmetic on choices that differ in one parameter each
#include "../imageclust_amd/csrc/conv_select.h"
#include "../imageclust_amd/csrc/prune_map.h"
#include "../imageclust_amd/csrc/resnet50_topology.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);    \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, " [%s]\n", #cond);                 \
            exit(1);                                           \
        }                                                      \
    } while (0)

static conv_opts opts(int p8, int split, int ncu)
{
    conv_opts o = {p8, 1, split, 2048, 1, 64, ncu}; // the context's defaults: conv_wr on, split from K = 2048, ICL_CONV_MODE 1, 64-pixel tiles at K = 256
    return o;
}

static std::string kernel_name(const conv_choice &c)
{
    char b[160];
    const char *tf[2] = {"false", "true"};
    switch (c.family) {
    case CONV_WR: snprintf(b, sizeof b, "conv_wr_kernel<%d, %d, %d, %s, %s>", c.wr_k, c.wr_ns, c.wr_mt, tf[c.res], tf[c.mapped]); break;
    case CONV_P8: snprintf(b, sizeof b, "conv_p8_kernel<%d, %d, %s, %s, %s, %s>", c.layout == 1 ? 2 : 4, c.layout == 1 ? 4 : 2, tf[c.taps], tf[c.dual], tf[c.split], tf[c.x3]); break;
    case CONV_HALO: snprintf(b, sizeof b, "conv3x3_halo_kernel<%d, %d>", c.bn, c.ring); break;
    case CONV_IGEMM: snprintf(b, sizeof b, "conv_igemm_kernel<%d, %s, %s>", c.bn, tf[c.dual], tf[c.early]); break;
    default: snprintf(b, sizeof b, "unsupported");
    }
    return b;
}

static void print_choice(const conv_choice &c)
{
    const char *fam[5] = {"unsupported", "wr", "p8", "halo", "igemm"};
    printf("family=%s K=%d ns=%d mt=%d res=%d mapped=%d slices=%d workers=%d layout=%d taps=%d dual=%d split=%d x3=%d bn=%d npw=%d ring=%d stages=%d early=%d "
           "gx=%d gy=%d blocks=%u threads=%u lds=%zu counter=%d\n",
           fam[c.family], c.wr_k, c.wr_ns, c.wr_mt, (int)c.res, (int)c.mapped, c.slices, c.workers, c.layout, (int)c.taps, (int)c.dual, (int)c.split, (int)c.x3, c.bn, c.npw,
           c.ring, c.stages, (int)c.early, c.gx, c.gy, c.blocks, c.threads, c.lds, c.counter);
}

static int choose(const char *path)
{
    FILE *f = fopen(path, "r");
    CHECK(f, "cannot open %s", path);
    int prec, B, H, cin, cout, k, stride, pad, res, p8, split, ncu, n = 0;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d", &prec, &B, &H, &cin, &cout, &k, &stride, &pad, &res, &p8, &split, &ncu) == 12) {
        const conv_args a = conv_plain(nullptr, nullptr, nullptr, res ? (const void *)&res : nullptr, nullptr, nullptr, nullptr, B, H, cin, cout, k, stride, pad, 1);
        const conv_choice c = conv_select(prec, a, opts(p8, split, ncu));
        CHECK(c.family != CONV_UNSUPPORTED, "case %d is unsupported: %s", n, c.why);
        // what every launch must satisfy, whatever the family: the grid covers the tiles, the LDS fits a workgroup's 160 KiB
        CHECK(c.blocks >= 1 && c.lds <= 160 * 1024 && (c.threads == 256 || c.threads == 512), "case %d: launch", n);
        if (c.family != CONV_WR) CHECK((int64_t)c.gx * c.gy == (int64_t)c.blocks && c.gy >= 1, "case %d: %d x %d tiles, %u workgroups", n, c.gx, c.gy, c.blocks);
        print_choice(c);
        ++n;
    }
    fclose(f);
    return 0;
}

static int plan(char **v, int stem_max_blocks)
{
    const int prec = atoi(v[0]), B = atoi(v[1]), ncu = atoi(v[2]), dense = atoi(v[3]), tap = atoi(v[4]);
    fwd_opts o = {opts(atoi(v[7]), atoi(v[8]), ncu), atoi(v[5]), atoi(v[6]), atoi(v[9])};
    o.stem_max_blocks = stem_max_blocks;
    icl_conv_rec recs[ICL_RESNET50_NCONV];
    const int n = resnet50_topology(recs);
    const fwd_plan p = forward_make_plan(recs, n, prec, B, dense != 0, tap, o);
    CHECK(!p.err, "plan: %s (convolution %d)", p.err, p.err_layer);
    for (const fwd_step &s : p.steps) {
        const icl_conv_rec &r = recs[s.layer];
        char layer[32];
        std::string kernel;
        switch (s.kind) {
        case FWD_STEM2_POOL: snprintf(layer, sizeof layer, "stem"); kernel = "stem2_pool_kernel"; break;
        case FWD_STEM_POOL: snprintf(layer, sizeof layer, "stem"); kernel = "stem_pool_kernel"; break;
        case FWD_STEM: snprintf(layer, sizeof layer, "stem"); kernel = "stem_conv_kernel"; break;
        case FWD_MAXPOOL: snprintf(layer, sizeof layer, "maxpool"); kernel = "maxpool_kernel"; break;
        case FWD_BNECK56: snprintf(layer, sizeof layer, "s%d.b%d", r.stage, r.block); kernel = s.ds ? "bneck56_kernel<true>" : "bneck56_kernel<false>"; break;
        case FWD_CONV: snprintf(layer, sizeof layer, "s%d.b%d.c%d", r.stage, r.block, r.role); kernel = kernel_name(s.c); break;
        case FWD_AVGPOOL: snprintf(layer, sizeof layer, "avgpool"); kernel = "avgpool_kernel"; break;
        default: snprintf(layer, sizeof layer, "fc"); kernel = "fc_kernel";
        }
        for (int b : {s.x, s.y, s.r, s.x2}) CHECK(b >= FWD_NONE && b <= FWD_Y, "buffer %d", b);
        CHECK(s.y == FWD_NONE || (s.y != s.x && s.y != s.r && s.y != s.x2), "%s writes a buffer it reads", layer);
        printf("%s|%llu|%s|pruned=%d|x=%d y=%d r=%d x2=%d\n", layer, (unsigned long long)s.blocks * s.threads, kernel.c_str(), (int)s.pruned, s.x, s.y, s.r, s.x2);
    }
    printf("out %d %d %d pruned %d\n", p.out, p.H, p.C, p.pruned);
    return 0;
}

// plan_pruned_block's check: a pruned launch whose choice differs from the unpruned layer's in ONE parameter that fixes the K order is refused
static int refuse()
{
    const conv_opts o = opts(1, 0, 256);
    // stage 3's last block at B = 256: c2 3x3 256 -> 256 at 14 x 14 and at stride 2; c3 256 -> 1024 plain and mapped
    const conv_args u2 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 256, 14, 256, 256, 3, 1, 1, 1);
    const conv_args p2 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 256, 14, 256, 256, 3, 2, 1, 1);
    conv_args u3 = conv_plain(nullptr, nullptr, nullptr, &o, nullptr, nullptr, nullptr, 256, 14, 256, 1024, 1, 1, 0, 1), p3 = u3;
    p3 = conv_plain(nullptr, nullptr, nullptr, &o, nullptr, nullptr, nullptr, 256, 7, 256, 1024, 1, 1, 0, 1);
    p3.omap = prune_map_make(2, 14, 14);
    const conv_choice cu2 = conv_select(CONV_PREC_BF16, u2, o), cp2 = conv_select(CONV_PREC_BF16, p2, o);
    const conv_choice cu3 = conv_select(CONV_PREC_BF16, u3, o), cp3 = conv_select(CONV_PREC_BF16, p3, o);
    CHECK(cu2.family == CONV_P8 && cu3.family == CONV_WR && cp3.mapped && !cu3.mapped, "the base case's families");
    CHECK(conv_same_arithmetic(cu2, cp2) && conv_same_arithmetic(cu3, cp3), "the base case is refused");
    CHECK(cu2.blocks != cp2.blocks, "the grid differs and does not matter");
    conv_choice t = cp2;
    t.family = CONV_HALO;
    CHECK(!conv_same_arithmetic(cu2, t), "another family");
    t = cp2;
    t.split = !t.split;
    CHECK(!conv_same_arithmetic(cu2, t), "split wanted on one side");
    t = cp2;
    t.layout = 2;
    CHECK(!conv_same_arithmetic(cu2, t), "another p8 layout");
    t = cp3;
    t.wr_mt = 2;
    CHECK(!conv_same_arithmetic(cu3, t), "another tile height");
    conv_choice none = {};
    CHECK(!conv_same_arithmetic(none, none), "two unsupported launches");
    // ... and through the rule itself: under ICL_CONV_SPLIT with a minimum K of 2304 the 14 x 14 layer is not split and its 7 x 7 sample is
    conv_opts so = opts(1, 1, 256);
    so.sk_min_k = 2304;
    CHECK(!conv_same_arithmetic(conv_select(CONV_PREC_BF16, u2, so), conv_select(CONV_PREC_BF16, p2, so)), "split on the pruned side only");
    icl_conv_rec recs[ICL_RESNET50_NCONV];
    const int n = resnet50_topology(recs);
    conv_args q2, q3;
    int ci = 0;
    for (int i = 0; i < n; ++i)
        if (recs[i].stage == 3 && recs[i].block == 5 && recs[i].role == 2) ci = i;
    CHECK(plan_pruned_block(recs[ci], recs[ci + 1], 2, 256, o, &q2, &q3), "stage 3's last block");
    CHECK(!plan_pruned_block(recs[ci], recs[ci + 1], 2, 256, so, &q2, &q3), "... with the split form on one side");
    conv_opts off = o;
    off.wr = 0;
    CHECK(!plan_pruned_block(recs[ci], recs[ci + 1], 2, 256, off, &q2, &q3), "... without the kernel that writes through a map");
    CHECK(!plan_pruned_block(recs[ci], recs[ci + 1], 1, 256, o, &q2, &q3), "stride 1");
    printf("refused: family, split, layout, tile height, unsupported; split on one side; no mapped kernel; stride 1\nok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "topo")) {
        icl_conv_rec t[ICL_RESNET50_NCONV];
        const int n = resnet50_topology(t);
        CHECK(n == ICL_RESNET50_NCONV, "%d records", n);
        for (int i = 0; i < n; ++i) printf("%d %d %d %d %d %d %d %d %d %d\n", t[i].cin, t[i].cout, t[i].k, t[i].stride, t[i].pad, t[i].hin, t[i].hout, t[i].role, t[i].stage, t[i].block);
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "choose")) return choose(argv[2]);
    if ((argc == 12 || argc == 13) && !strcmp(argv[1], "plan")) return plan(argv + 2, argc == 13 ? atoi(argv[12]) : 0);
    if (argc == 2 && !strcmp(argv[1], "refuse")) return refuse();
    fprintf(stderr, "usage: see the head of conv_select_main.cpp\n");
    return 2;
}
