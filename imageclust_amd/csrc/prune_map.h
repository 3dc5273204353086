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
#else
#define PRUNE_HD
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
