// prune_map.h -- the forward pass computes only the pixels the next stage's stride reads ("dead pixels"): the rule that
// says which bottleneck may be pruned, and the map from a pixel of the compact [B][Ho][Wo] tensor the pruned c2 / c3 work on to its place
// in the full-size [B][H][W] tensor the residual is read from and the output is written to.  Plain C++ with no HIP in it:
// tests/prune_map_main.cpp compiles it with the host compiler alone and checks the map against the obvious triple loop; conv_wr_kernel
// calls prune_map_pixel for its residual loads and its stores, so the place of a pixel is stated once.
#pragma once
#include <cstdint>

#include "../../include/icl_model_format.h"

#ifdef __HIPCC__
#define PRUNE_HD __host__ __device__
#define PRUNE_FI __host__ __device__ __forceinline__
#else
#define PRUNE_HD
#define PRUNE_FI inline
#endif

// Output-pixel map of a convolution launch: compact pixel (b, oy, ox) of [B][Ho][Wo] lives at pixel (b, sub * oy, sub * ox) of [B][H][W].
// sub == 0: no map (the output is the compact tensor itself).
struct prune_map {
    int sub, H, W, Ho, Wo;
};

// extent of a k = 1, pad = 0, stride = s convolution's output over h input pixels: the pixels 0, s, 2 s, ... < h
PRUNE_HD inline int prune_extent(int h, int s) { return (h - 1) / s + 1; }

inline prune_map prune_map_make(int sub, int H, int W)
{
    prune_map pm = {sub, H, W, prune_extent(H, sub), prune_extent(W, sub)};
    return pm;
}

// compact pixel index m (< B * Ho * Wo) -> pixel index in the full tensor
PRUNE_HD inline int64_t prune_map_pixel(const prune_map &pm, unsigned m)
{
    const unsigned t = m / (unsigned)pm.Wo, ox = m - t * (unsigned)pm.Wo;
    const unsigned b = t / (unsigned)pm.Ho, oy = t - b * (unsigned)pm.Ho;
    return ((int64_t)b * pm.H + (int64_t)pm.sub * oy) * pm.W + (int64_t)pm.sub * ox;
}

// The rule: a bottleneck's output is read only at the pixels (s * oy, s * ox) when the block that follows it in the same pass is a block 0
// whose c1 and downsample records are both 1 x 1, pad 0, with one stride s > 1 over this block's output.  c3: the last convolution of the
// block in question; next_c1 / next_ds: the records of the block after it (next_ds == nullptr: it has no downsample branch).  Returns s,
// or 0 (every pixel is needed).  Only an identity block is pruned (its c2 is 3 x 3 / stride 1 / pad 1, so that sampling it at stride s is
// the 3 x 3 / stride s / pad 1 convolution; its c3 is 1 x 1 / stride 1).
inline int prune_stride(const icl_conv_rec &c2, const icl_conv_rec &c3, const icl_conv_rec *next_c1, const icl_conv_rec *next_ds)
{
    if (!next_c1 || !next_ds || next_c1->role != 1 || next_ds->role != 4 || next_c1->block != 0) return 0;
    const int s = next_c1->stride;
    if (s <= 1 || next_ds->stride != s || next_c1->k != 1 || next_ds->k != 1 || next_c1->pad != 0 || next_ds->pad != 0) return 0;
    if (next_c1->hin != c3.hout || next_ds->hin != c3.hout || next_c1->cin != c3.cout || next_ds->cin != c3.cout) return 0;
    if (c3.role != 3 || c3.block == 0 || c3.k != 1 || c3.stride != 1 || c3.pad != 0) return 0;
    if (c2.role != 2 || c2.k != 3 || c2.stride != 1 || c2.pad != 1 || c2.hout != c3.hin || c2.hin != c2.hout) return 0;
    // 3 x 3 / pad 1 / stride s and 1 x 1 / pad 0 / stride s give the same extent: (h + 2 - 3) / s + 1 == (h - 1) / s + 1
    return s;
}

// ------------------------------------------------------------------------------------------------------------
// The same rule inside the fused stage-1 bottleneck (bneck56_kernel<false, 2>, resnet_fused.h): the kernel walks a strip of a RUN of images
// stacked with one padding row between them (VH = H + 1 virtual rows per image, row H = padding) in steps of 4 virtual rows, so which rows
// of a step are read by the strided reader follows from the row cursor alone -- never from the step index: the parity of a virtual row
// flips from one image of a run to the next.  tests/bneck56_needed_main.cpp walks these functions on the host against the triple loop.
// ------------------------------------------------------------------------------------------------------------
// (image, row) of a virtual row cursor, advanced without divisions (VH = H + 1 rows per image, row H = padding)
struct bn56_row {
    int b, r, p; // image, row inside the image (H = the padding row), physical row b * H + r of the tensor
    PRUNE_FI void step(int VH)
    {
        ++p;
        if (++r == VH) {
            r = 0;
            ++b;
            --p; // the padding row is not in memory
        }
    }
};
// row r of an image of H rows (r == H: the padding row) / column c of its W columns is read by a 1 x 1, pad 0, stride sub reader
PRUNE_FI bool bn56_row_needed(int r, int H, int sub) { return r < H && r % sub == 0; }
PRUNE_FI bool bn56_col_needed(int c, int W, int sub) { return c < W && c % sub == 0; }
// Front waves, sub >= 2: the needed rows among the 4 virtual rows from t on, as row indices 0..3 of the step.  Two rows that follow each
// other are never both needed (inside an image their parities differ, the padding row is never needed), so there are at most two: {a, b},
// a < b when both are needed.  With fewer, the spare index names another, unneeded row of the step (a != b always): conv2 computes two
// rows per step without a branch, and what it leaves in an unneeded row of t2 nobody reads.
struct bn56_rows2 {
    int a, b;
};
PRUNE_FI bn56_rows2 bn56_step_rows(bn56_row t, int H, int VH, int sub)
{
    int a = -1, b = -1;
    for (int m = 0; m < 4; ++m) {
        if (bn56_row_needed(t.r, H, sub)) {
            if (a < 0) a = m;
            else b = m;
        }
        t.step(VH);
    }
    if (a < 0) a = 0;
    if (b < 0) b = a ^ 2;
    return bn56_rows2{a, b};
}
// Back waves: which of a quarter's two rows (t0 and the row behind it) is stored -- needed, and a row of the run's images [b0, b1):
// 0, 1, or -1 (neither: the quarter does nothing).
PRUNE_FI int bn56_quarter_row(bn56_row t0, int b0, int b1, int H, int VH, int sub)
{
    if (t0.b >= b0 && t0.b < b1 && bn56_row_needed(t0.r, H, sub)) return 0;
    t0.step(VH);
    if (t0.b >= b0 && t0.b < b1 && bn56_row_needed(t0.r, H, sub)) return 1;
    return -1;
}
