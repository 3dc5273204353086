// bneck56_needed_main.cpp -- which pixels the pruned fused stage-1 bottleneck (bneck56_kernel<false, 2>, imageclust_amd/csrc/resnet_fused.h)
// stores: a stand-alone host program (no GPU, no HIP) that tests/test_bneck56_needed_cpu.py builds with the address and undefined-behaviour
// sanitizers and runs.  It walks runs of 1 to 4 stacked images in the kernel's 4-row steps with the kernel's own cursor and rules
// (bn56_row, bn56_step_rows, bn56_quarter_row, bn56_col_needed: prune_map.h), strip by strip and store lane by store lane, and checks
// against the obvious triple loop that exactly the pixels (2 oy, 2 ox) are stored, each once, and that the front waves' two rows of a step
// contain every row its quarters store.  Prints one line per group and a final "ok".
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

static const int ROWS = 4, COLS = 14, SUB = 2; // BN56_ROWS, BN56_COLS, the reader's stride

int main()
{
    long long stored = 0, steps = 0, idle_quarters = 0, one_row_steps = 0;
    const int heights[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 56}, widths[] = {1, 13, 14, 15, 29, 56};
    for (int H : heights)
        for (int W : widths)
            for (int n = 1; n <= 4; ++n)      // images of the run
                for (int b0 : {0, 3}) {       // the run's first image inside a batch of b0 + n + 1
                    const int B = b0 + n + 1, b1 = b0 + n, VH = H + 1;
                    const int nstrips = (W + COLS - 1) / COLS, nsteps = (n * VH + ROWS - 1) / ROWS;
                    std::vector<int> hit((size_t)B * H * W, 0);
                    for (int strip = 0; strip < nstrips; ++strip) {
                        const int c0 = strip * COLS;
                        CHECK(c0 % SUB == 0, "strip %d starts at an odd column", strip);
                        bn56_row out = {b0 - 1, H, b0 * H}; // the back waves' cursor: the padding row above the run
                        bn56_row o2 = out;                  // the front waves' cursor of the same row
                        for (int j = 0; j < nsteps; ++j) {
                            const bn56_rows2 nr = bn56_step_rows(o2, H, VH, SUB);
                            CHECK(nr.a >= 0 && nr.a < ROWS && nr.b >= 0 && nr.b < ROWS && nr.a != nr.b, "step %d: rows %d, %d", j, nr.a, nr.b);
                            int in_step = 0;
                            for (int qd = 0; qd < 2; ++qd) { // the quarters: rows {0, 1} and {2, 3} of the step
                                bn56_row t = out;
                                const int mm = bn56_quarter_row(t, b0, b1, H, VH, SUB);
                                if (mm >= 0) {
                                    const int m = 2 * qd + mm;
                                    CHECK(m == nr.a || m == nr.b, "H %d, n %d, step %d: row %d is stored but conv2 computes rows %d, %d", H, n, j, m, nr.a, nr.b);
                                    if (mm) t.step(VH);
                                    CHECK(t.b >= b0 && t.b < b1 && t.r < H && t.p == t.b * H + t.r, "row (%d, %d) at physical row %d", t.b, t.r, t.p);
                                    for (int lcol = 0; lcol < 8; ++lcol) { // the store instruction: 8 lanes per pixel, strip column 2 * lcol
                                        const int c = SUB * lcol;
                                        if (!(c < COLS && bn56_col_needed(c0 + c, W, SUB))) continue;
                                        ++hit[((size_t)t.p) * W + c0 + c];
                                        ++stored;
                                    }
                                    ++in_step;
                                } else {
                                    ++idle_quarters;
                                }
                                out.step(VH);
                                out.step(VH);
                            }
                            one_row_steps += in_step == 1;
                            for (int i = 0; i < ROWS; ++i) o2.step(VH);
                            CHECK(o2.b == out.b && o2.r == out.r && o2.p == out.p, "the two cursors part");
                            ++steps;
                        }
                    }
                    for (int b = 0; b < B; ++b) // the triple loop: inside the run exactly the pixels (2 oy, 2 ox), each once; nothing outside it
                        for (int y = 0; y < H; ++y)
                            for (int x = 0; x < W; ++x) {
                                const int want = (b >= b0 && b < b1 && y % SUB == 0 && x % SUB == 0) ? 1 : 0;
                                CHECK(hit[((size_t)b * H + y) * W + x] == want, "H %d W %d, run [%d, %d): pixel (%d, %d, %d) stored %d times, not %d", H, W, b0, b1, b,
                                      y, x, hit[((size_t)b * H + y) * W + x], want);
                            }
                }
    CHECK(idle_quarters > 0 && one_row_steps > 0, "no step with fewer than two stored rows was walked");
    printf("walk: %lld steps, %lld pixels stored, each (2 oy, 2 ox) once and nothing else; %lld quarters store no row\n", steps, stored, idle_quarters);

    // ---- the rules alone
    for (int H = 1; H <= 9; ++H)
        for (int r = 0; r <= H; ++r) CHECK(bn56_row_needed(r, H, SUB) == (r < H && r % 2 == 0), "row %d of %d", r, H);
    for (int W : widths)
        for (int c = 0; c < W + 3; ++c) CHECK(bn56_col_needed(c, W, SUB) == (c < W && c % 2 == 0), "column %d of %d", c, W);
    printf("rules: even rows and columns inside the image, never the padding row\n");
    printf("ok\n");
    return 0;
}
