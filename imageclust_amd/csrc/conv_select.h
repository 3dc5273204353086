// conv_select.h -- which kernel a convolution of the forward pass takes, and with which launch: the rule, stated once.  Plain C++ with no HIP
// in it (as prune_map.h): resnet.hip's launch_conv_t is conv_select followed by one switch over the family, the launchers of conv_wr.h,
// conv_p8.h and resnet.hip take the choice and derive nothing again, the pruned block of the forward pass compares two choices
// (conv_same_arithmetic) and names no kernel, and tests/conv_select_main.cpp compiles this header with the host compiler alone.
//
// Order of precedence: conv_wr_kernel (bf16, the HBM-bound 1x1 layers) -> conv_p8_kernel (bf16 and split bf16, the K-heavy layers) ->
// conv3x3_halo_kernel (3x3 / stride 1 / pad 1 with Cin >= 128) -> conv_igemm_kernel.  Only conv_wr_kernel writes through an output-pixel map.
#pragma once
#include <cstddef>
#include <cstdint>

#include "prune_map.h"

struct conv_args {
    const void *X;      // [B][H][W][Cin]
    const void *Wt;     // [Cout][KH][KW][Cin]
    void *Y;            // [B][Ho][Wo][Cout]
    const void *R;      // residual, same shape as Y, or nullptr
    const float *scale; // [Cout] folded BN scale
    const float *shift; // [Cout] folded BN shift (+ conv bias)
    const void *zero;   // >= 16 zero bytes: the source of padded taps / rows beyond M for the LDS-DMA loads
    int B, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, relu;
    int64_t M;          // B*Ho*Wo
    int K;              // KH*KW*Cin
    int gx, gy;         // tiles along M and along Cout
    // optional second operand (DUAL kernels): a 1x1 / stride2 convolution over X2 accumulated into the SAME tile, i.e.
    // the K axis is [KH*KW*Cin of X | Cin2 of X2].  Used to fuse a bottleneck's downsample branch into its last conv.
    const void *X2;     // [B][H2][W2][Cin2]
    int H2, W2, Cin2, stride2;
    // split form of conv_p8_kernel (conv_p8.h): partner sums, one flag per tile, the value the flags are raised to by this launch
    void *sk_part;
    int *sk_flag;
    int sk_epoch;
    // optional output-pixel map (conv_wr_kernel's MAP form only; omap.sub == 0: none): X is the compact [B][Ho][Wo][Cin] tensor, R and Y are
    // full-size [B][omap.H][omap.W][Cout] tensors in which output pixel (b, oy, ox) is pixel (b, sub * oy, sub * ox) -- prune_map.h
    prune_map omap;
};

#define CONV_PREC_FP32 0  /* == ICL_PREC_FP32, _BF16, _BF16X3 (imageclust.h; resnet.hip asserts it) */
#define CONV_PREC_BF16 1
#define CONV_PREC_BF16X3 2
#define CONV_TILE_M 128   /* == CV_BM: pixels per tile of the 128 x BN kernels */
#define CONV_ROW_BYTES 128 /* == CV_ROWB: bytes of one k-step of one tile row in LDS */
#define HALO_MAXP 12 /* halo pieces (8 pixels x 128 B) a wave fetches per channel chunk: tiles of up to 384 halo pixels */
#ifndef P8_AUTO_MIN_NT
#define P8_AUTO_MIN_NT 4 /* ICL_CONV_P8_AUTO: layers with K >= 256 (measured with two passes in flight) */
#endif

// Everything the choice reads that is not the shape (resnet.hip's conv_opts_of fills it from the context and the environment).
struct conv_opts {
    int p8;        // ICL_CONV_P8_OFF / _AUTO / _ALL (icl_set_conv_options)
    int wr;        // the streaming 1x1 kernel is on (ICL_CONV_WR)
    int sk;        // the split form of conv_p8_kernel is wanted (ICL_CONV_SPLIT)
    int sk_min_k;  // ... for layers with at least this K
    int conv_mode; // ICL_CONV_MODE: 0 plain two-stage loop, 1 default, 2 no halo kernel for the 3x3 layers
    int wr_pt256;  // ICL_WR_PT256: pixels per tile of conv_wr_kernel's K = 256 layers, 64 or 32
    int ncu;       // compute units of the device
};

enum conv_family { CONV_UNSUPPORTED = 0, CONV_WR, CONV_P8, CONV_HALO, CONV_IGEMM };

// The kernel family, what names the instantiation, and the launch.  Fields of another family than `family` are zero.
struct conv_choice {
    int family;
    const char *why; // CONV_UNSUPPORTED: the message
    // conv_wr_kernel<K, NS, MT, RES, MAP>: slices x workers workgroups
    int wr_k, wr_ns, wr_mt, slices, workers;
    bool res, mapped;
    // conv_p8_kernel<MW, NWV, TAPS, DUAL, SPLIT, X3>: layout 1 = 2 x 4 waves (256 x 256 tile), 2 = 4 x 2 waves (512 x 128); split: WANTED -- the
    // launcher falls back to one workgroup per tile when the scratch of the split form cannot be had
    int layout;
    bool taps, split, x3;
    // conv3x3_halo_kernel<T, BN, ring>(npw); conv_igemm_kernel<T, BN, DUAL, 2, EARLY> with `stages` stages of LDS
    int bn, npw, ring, stages;
    bool dual, early; // dual: also conv_p8_kernel's
    // the launch
    int gx, gy;        // tiles along M and along Cout (conv_args::gx, gy)
    unsigned blocks, threads; // workgroups (the split form launches 2 * blocks) and their size
    size_t lds;        // dynamic LDS bytes
    int counter;       // the launch counter it bumps: 0 conv_wr_kernel / conv_p8_kernel, 1 the 128 x BN kernels (icl_conv_stats)
};

static inline int64_t conv_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the kernels' view of the arguments: BF16X3 is given in real channels, the kernels see the split layout as bf16 tensors of twice the channels
// (Cin, Cin2 and K doubled; Cout -- the rows of the weights and of the accumulator tile -- unchanged)
static inline conv_args conv_kernel_view(int prec, conv_args a)
{
    if (prec == CONV_PREC_BF16X3) {
        a.Cin *= 2;
        a.Cin2 *= 2;
        a.K *= 2;
    }
    return a;
}

// ---- conv_wr_kernel: the HBM-bound 1x1 layers (stride 1, pad 0, no second operand): the identity bottlenecks' c3 (K = 128 / 256 / 512,
// Cout = 4 K, residual) and stage 2's c1 (K = 512, Cout = 128).  Slice width / tile height by K so that the weights fit 64-128 VGPRs and two
// workgroups fit a CU's LDS.
static inline bool conv_wr_shape(const conv_args &a, const conv_opts &o, int *ns, int *pt)
{
    if (a.K == 128) { *ns = 256; *pt = 64; }
    else if (a.K == 256) { *ns = 128; *pt = o.wr_pt256 == 32 ? 32 : 64; }
    else if (a.K == 512) { *ns = 128; *pt = 32; }
    else return false;
    return a.Cout % *ns == 0;
}
static inline bool conv_wr_eligible(const conv_args &a, const conv_opts &o)
{
    if (o.p8 == 0 || a.X2 || a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0 || a.Cin != a.K) return false;
    int ns, pt;
    if (!conv_wr_shape(a, o, &ns, &pt)) return false;
    if (a.omap.sub && (a.K > 256 || pt != 64)) return false; // the mapped form exists for the 64-pixel tiles of K = 128 / 256
    if (a.K == 512 && a.Cout > 128 && a.Cout < 2048) return false; // (1024 -> ... K = 512 shapes other than 512 -> 128 / 512 -> 2048 do not occur; stride-2 c1 layers are not eligible anyway)
    if ((size_t)a.M * a.K * 2 >= (1ull << 31) || (size_t)a.M * a.Cout * 2 >= (1ull << 31)) return false; // 32-bit buffer offsets, BN56_OOB = 2^31
    if (a.omap.sub) { // the mapped form: the compact pixels are those of the map, and the FULL tensor stays below 2^31 bytes
        const prune_map &pm = a.omap;
        if (pm.sub < 1 || pm.Ho != prune_extent(pm.H, pm.sub) || pm.Wo != prune_extent(pm.W, pm.sub) || a.Ho != pm.Ho || a.Wo != pm.Wo) return false;
        if ((size_t)a.B * pm.H * pm.W * a.Cout * 2 >= (1ull << 31)) return false;
    }
    return true;
}

// ---- conv_p8_kernel (bf16 and split bf16): Cout a multiple of 256 (256 x 256 tile) or of 128 (512 x 128 tile), whole K-tiles of 64 channels
// and an even number of them.  ICL_CONV_P8_AUTO: K >= 256, whatever the tile count: with two forward passes in flight (the timed
// configuration) fewer, longer tiles leave CUs to the other pass -- the 7 x 7 layers (98 tiles) take longer as single launches than on the
// 128 x 128 kernels (293 vs 225 us for the three 3x3 layers) and the embedding as a whole is faster (profiles/r05_ab_conv_p8_*.json).
static inline int conv_p8_layout(const conv_args &a) { return a.Cout % 256 == 0 ? 1 : (a.Cout % 128 == 0 ? 2 : 0); } // 1: 2 x 4 waves, 2: 4 x 2 waves
static inline bool conv_p8_eligible(const conv_args &a, const conv_opts &o)
{
    if (o.p8 == 0) return false;
    const int lay = conv_p8_layout(a);
    if (!lay || a.Cin % 64 || (a.X2 && a.Cin2 % 64)) return false;
    if (a.KH * a.KW > 9 || a.KH * a.KW * a.Cin + (a.X2 ? a.Cin2 : 0) != a.K) return false;
    if (a.X2 && (a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0)) return false;
    const int nt = a.K / 64;
    if (a.K % 128) return false; // an even number of K-tiles (the loop is unrolled by two buffers); nt == 2 runs the prologue and the two peeled tiles only
    if ((size_t)a.B * a.H * a.W * a.Cin * 2 >= (1ull << 31) || (size_t)a.Cout * a.K * 2 >= (1ull << 31)) return false; // 32-bit buffer offsets, BN56_OOB = 2^31
    if (a.X2 && (size_t)a.B * a.H2 * a.W2 * a.Cin2 * 2 >= (1ull << 31)) return false;
    if (a.M >= (1ll << 31) - 512) return false;
    if (o.p8 >= 2) return true;
    return nt >= P8_AUTO_MIN_NT;
}
// The split form (opt-in: ICL_CONV_SPLIT / ICL_CONV_SK=1): a rule on the LAYER's shape only (never on the batch: an image's embedding must not depend
// on the images beside it) -- the 7 x 7 layers, whose 256 x 256 tiles number 0.38 per image.  It shortens a lone forward pass (3 476 -> 3 277 us per
// batch of 256; the three 3x3 layers 321 -> 227 us) and costs the throughput configuration 1.1-1.5 % (two passes in flight: the CUs a 98-tile
// launch leaves idle are the other pass's, and two half-K workgroups take more CU-time than one), hence off by default.  bf16, 256 x 256 tiles only.
static inline bool conv_p8_split_eligible(const conv_args &a, const conv_opts &o)
{
    return o.sk && !a.X2 && a.Ho * a.Wo <= 49 && a.K % 256 == 0 && a.K >= o.sk_min_k && a.Cout % 256 == 0;
}

// ---- conv3x3_halo_kernel: halo pieces per wave for an image width (0: the shape does not fit the halo kernel)
static inline int conv3x3_halo_npw(int W)
{
    const int rows = (W - 1 + CONV_TILE_M - 1) / W + 1 + 2; // image rows a run of 128 pixels can touch, plus one above and below
    const int pieces = (rows * (W + 2) + 7) / 8;
    const int npw = (pieces + 3) / 4;
    return npw <= HALO_MAXP ? npw : 0;
}
static inline size_t conv3x3_halo_lds(int bn, int npw, int ws) // [halo image][zero pixels][ws weight stages], or the epilogue tile
{
    const size_t body = (size_t)4 * npw * 1024 + 512 + (size_t)ws * bn * CONV_ROW_BYTES, ep = (size_t)64 * (bn + 4) * 4;
    return body > ep ? body : ep;
}
// ---- conv_igemm_kernel: nstages staging buffers, or the epilogue tile
static inline size_t conv_igemm_lds(int bn, int nstages)
{
    const size_t stages = (size_t)nstages * (bn + CONV_TILE_M) * CONV_ROW_BYTES, ep = (size_t)64 * (bn + 4) * 4;
    return stages > ep ? stages : ep;
}

// The choice for convolution a (real channels) in precision prec.  Tile / pipeline of the 128 x BN kernels (B = 256 shapes of ResNet50, measured
// with scratch/layer_report.py): 128 x 128 tile (128 x 64 for Cout = 64), two stages, two workgroups per CU, everything requested up front (EARLY);
// ICL_CONV_MODE=0 selects the plain two-stage loop (one k-step staged ahead) for A/B comparisons.  Deeper rings, 128 x 64 tiles for the 128-wide
// layers, weights in registers and dedicated loader waves were all measured slower.
static inline conv_choice conv_select(int prec, const conv_args &real, const conv_opts &o)
{
    const conv_args a = conv_kernel_view(prec, real);
    const bool bf16 = prec == CONV_PREC_BF16, x3 = prec == CONV_PREC_BF16X3;
    conv_choice c = {};
    // the HBM-bound c3 layers of the identity bottlenecks: weights in registers, streaming tiles (conv_wr.h; no split-bf16 form)
    if (bf16 && o.wr && conv_wr_eligible(a, o)) {
        int pt = 0;
        (void)conv_wr_shape(a, o, &c.wr_ns, &pt);
        c.family = CONV_WR;
        c.wr_k = a.K;
        c.wr_mt = pt / 16;
        c.res = a.R != nullptr;
        c.mapped = a.omap.sub != 0;
        c.slices = a.Cout / c.wr_ns;
        const int ntiles = (int)conv_ceil_div(a.M, pt);
        const int per_cu = (a.K == 256 && pt == 32) ? 3 : 2; // workgroups per CU the LDS (2 x image) and the registers allow
        const int workers = (per_cu * o.ncu / c.slices) & ~7, cap = (int)conv_ceil_div(ntiles, 8) * 8;
        c.workers = workers < 8 ? 8 : workers;
        if (c.workers > cap) c.workers = cap;
        c.gx = ntiles;
        c.gy = c.slices;
        c.blocks = (unsigned)(c.slices * c.workers);
        c.threads = 256;
        return c;
    }
    if (a.omap.sub) {
        c.why = "conv: only the streaming 1x1 kernel writes through an output-pixel map (bf16, K = 128 or 256)";
        return c;
    }
    // the K-heavy layers: 256 x 256 tiles on the deep-pipelined loop (conv_p8.h)
    if ((bf16 || x3) && conv_p8_eligible(a, o)) {
        c.family = CONV_P8;
        c.layout = conv_p8_layout(a);
        c.dual = a.X2 != nullptr;
        c.taps = !c.dual && (a.KH * a.KW > 1 || a.pad != 0);
        c.x3 = x3;
        c.split = c.layout == 1 && !x3 && conv_p8_split_eligible(a, o); // (the split form is bf16 only: under BF16X3 it is ignored)
        c.gx = (int)conv_ceil_div(a.M, c.layout == 1 ? 256 : 512);
        c.gy = a.Cout / (c.layout == 1 ? 256 : 128);
        c.blocks = (unsigned)(c.gx * c.gy);
        c.threads = 512;
        return c;
    }
    const bool wide = a.Cout % 128 == 0;
    c.counter = 1;
    c.gx = (int)conv_ceil_div(a.M, CONV_TILE_M);
    c.threads = 256;
    // (Cin = 64, stage 1: one channel chunk, 9 short k-steps per tile -- nothing to hide the halo fetch behind, the implicit-GEMM
    // kernel's fully pipelined staging is 3-5 % faster there although it moves three times the bytes)
    if (o.conv_mode == 1 && !a.X2 && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.Ho == a.H && a.Wo == a.W && a.Cin >= 128 && conv3x3_halo_npw(a.W)) {
        c.family = CONV_HALO; // every 3x3 layer of ResNet50 (W = 56, 28, 14, 7) fits
        c.bn = wide ? 128 : 64;
        c.npw = conv3x3_halo_npw(a.W);
        // 3 weight stages (two k-steps of weights in flight) where two workgroups still fit a CU's 160 KB of LDS, else 2
        c.ring = conv3x3_halo_lds(c.bn, c.npw, 3) <= 80 * 1024 ? 3 : 2;
        c.lds = conv3x3_halo_lds(c.bn, c.npw, c.ring);
    } else {
        c.family = CONV_IGEMM;
        c.dual = a.X2 != nullptr;
        c.bn = (c.dual || wide) ? 128 : 64;
        c.early = o.conv_mode != 0;
        const int nk = a.K / (prec == CONV_PREC_FP32 ? 32 : 64);
        c.stages = (c.dual || nk > 1) ? 2 : 1; // single-k-step layers need one stage only -> more workgroups per CU
        c.lds = conv_igemm_lds(c.bn, c.stages);
    }
    c.gy = a.Cout / c.bn;
    c.blocks = (unsigned)(c.gx * c.gy);
    return c;
}

// Same family and the same parameters that fix the order in which K is summed: everything but the grid and the mapped flag.  Two launches
// for which this holds give every output element they both compute the same bits.
static inline bool conv_same_arithmetic(const conv_choice &p, const conv_choice &q)
{
    if (p.family == CONV_UNSUPPORTED || p.family != q.family) return false;
    return p.wr_k == q.wr_k && p.wr_ns == q.wr_ns && p.wr_mt == q.wr_mt && p.res == q.res && p.layout == q.layout && p.taps == q.taps &&
           p.split == q.split && p.x3 == q.x3 && p.dual == q.dual && p.bn == q.bn && p.ring == q.ring && p.early == q.early && p.stages == q.stages;
}

// ------------------------------------------------------------------------------------------------------------
// The forward plan: every launch of one forward pass of B images, decided before the first of them -- the fuse mask, the pruned blocks, the
// tap stop, each convolution's arguments and choice, and which of the lane's five activation buffers each step reads and writes (the x / y
// swaps already played).  resnet.hip's forward_batch runs a plan on a lane and a stream: it patches the pointers in and launches.  A plan
// lives for one call; nothing is cached.
// ------------------------------------------------------------------------------------------------------------
#include <utility>
#include <vector>

#define BN56_COLS 14 /* output columns per strip of bneck56_kernel (resnet_fused.h) */
#define FWD_STEM_STRIPS 8 /* == SP_STRIPS: work units per image of the fused stems */

// A plain k x k convolution over square B x H x H x Cin images: no second operand; conv_select decides the tile counts (gx, gy), the launcher
// of the split form its fields.
static inline conv_args conv_plain(const void *X, const void *Wt, void *Y, const void *R, const float *scale, const float *shift, const void *zero, int B,
                                   int H, int Cin, int Cout, int k, int stride, int pad, int relu)
{
    conv_args a = {};
    a.X = X; a.Wt = Wt; a.Y = Y; a.R = R; a.scale = scale; a.shift = shift; a.zero = zero;
    a.B = B; a.H = a.W = H; a.Cin = Cin; a.Cout = Cout; a.KH = a.KW = k; a.stride = stride; a.pad = pad; a.relu = relu;
    a.Ho = a.Wo = (H + 2 * pad - k) / stride + 1;
    a.M = (int64_t)B * a.Ho * a.Wo;
    a.K = k * k * Cin;
    return a;
}
// ... plus a 1x1 / stride2 convolution over X2 ([B][H2][H2][Cin2]) accumulated into the same tiles: K = [k*k*Cin of X | Cin2 of X2]
static inline void conv_add_operand(conv_args &a, const void *X2, int H2, int Cin2, int stride2)
{
    a.X2 = X2; a.H2 = a.W2 = H2; a.Cin2 = Cin2; a.stride2 = stride2;
    a.K += Cin2;
}
// the grid of bneck56_kernel: strips of BN56_COLS columns x groups of images
static inline void bneck56_grid(int B, int W, int ncu, int *nstrips, int *ngroups)
{
    *nstrips = (W + BN56_COLS - 1) / BN56_COLS;
    const int g = ncu / *nstrips < B ? ncu / *nstrips : B;
    *ngroups = g < 1 ? 1 : g;
}
// the persistent grid of a stem kernel: units of work, at most per_cu workgroups on each compute unit; max_blocks > 0 (icl_set_stem_max_blocks,
// tests only) caps it further, so that a workgroup walks several units at a batch of a few images
static inline unsigned fwd_stem_blocks(int64_t units, int per_cu, int ncu, int max_blocks = 0)
{
    const int64_t g = units < (int64_t)per_cu * ncu ? units : (int64_t)per_cu * ncu;
    return (unsigned)(max_blocks > 0 && max_blocks < g ? max_blocks : g);
}

struct fwd_opts {
    conv_opts conv;
    int fuse;        // ICL_FUSE mask: bit 0 stem + maxpool in one launch, bit 1 / 2 stage 1's identity / first bottleneck in one launch, bit 3 stem2_pool_kernel
    int prune;       // icl_set_forward_prune
    int stem_per_cu; // workgroups per CU of the stem kernel this precision and mask take
    int prune_fused = 1; // icl_set_forward_prune_fused: with `prune` on, the rule also prunes a bottleneck that runs as ONE fused launch
    int stem_max_blocks = 0; // icl_set_stem_max_blocks (tests only): cap on the stem kernel's persistent grid, 0 = none
};

enum fwd_kind { FWD_STEM2_POOL, FWD_STEM_POOL, FWD_STEM, FWD_MAXPOOL, FWD_BNECK56, FWD_CONV, FWD_AVGPOOL, FWD_FC };
enum { FWD_X = 0, FWD_T1 = 1, FWD_T2 = 2, FWD_DS = 3, FWD_Y = 4, FWD_NONE = -1 }; // the lane's five activation buffers

struct fwd_step {
    int kind;
    int layer;     // record of the step's (first) convolution: whose weights it reads
    bool ds;       // FWD_BNECK56: the form with the downsample branch; FWD_CONV: the dual-operand c3 of a block 0 (fused weights, second operand x2)
    bool pruned;   // FWD_CONV: the launch that completes a pruned block (icl_forward_prune_stats)
    int sub;       // FWD_BNECK56: 1, or 2 -- the pruned instantiation, which writes the pixels (2 oy, 2 ox) only (icl_forward_prune_fused_stats)
    conv_args a;   // FWD_CONV: shapes and relu; the pointers are the lane's and the model's, patched in when the step runs
    conv_choice c; // FWD_CONV
    int x, y, r, x2; // roles of the lane's buffers: input, output, residual, second operand (FWD_NONE: none)
    unsigned blocks, threads; // the launch (FWD_CONV: the choice's)
};
struct fwd_plan {
    std::vector<fwd_step> steps;
    int out = FWD_X;   // the buffer that holds the last block's (a tap: the tapped block's) output, [B][H][H][C]
    int H = 56, C = 64;
    int B = 0;         // images
    int pruned = 0;    // blocks run in the pruned form
    const char *err = nullptr; // the pass cannot run: why (layer: which record)
    int err_layer = 0;
};

// The last identity block in front of a strided block 0 (prune_map.h: s = prune_stride(..) > 1), bf16: c2 as the 3x3 / stride s / pad 1
// convolution into a compact t2, c3 over that compact tensor with its residual and output at pixel (s oy, s ox) of the full-size x and y;
// the pixels in between are not written and nobody reads them.  Both launches must sum K as the unpruned layers' launches do
// (conv_same_arithmetic: the values that are still computed keep their bits); false -- the block runs unpruned -- if not.
static inline bool plan_pruned_block(const icl_conv_rec &r2, const icl_conv_rec &r3, int s, int B, const conv_opts &o, conv_args *p2, conv_args *p3)
{
    if (s <= 1) return false;
    const int prec = CONV_PREC_BF16;
    const conv_args u2 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, r2.hin, r2.cin, r2.cout, r2.k, r2.stride, r2.pad, 1);
    conv_args u3 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, r3.hin, r3.cin, r3.cout, 1, 1, 0, 1);
    *p2 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, r2.hin, r2.cin, r2.cout, r2.k, s, r2.pad, 1);
    *p3 = conv_plain(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, B, p2->Ho, r3.cin, r3.cout, 1, 1, 0, 1);
    u3.R = p3->R = &u3; // (the choice reads only whether there is a residual; the step's own pointer is patched in when it runs)
    p3->omap = prune_map_make(s, r3.hout, r3.hout);
    if (u2.K != r2.cin * r2.k * r2.k || u3.K != r3.cin || p2->Ho != p3->omap.Ho) return false;
    const bool same = conv_same_arithmetic(conv_select(prec, u2, o), conv_select(prec, *p2, o)) && conv_same_arithmetic(conv_select(prec, u3, o), conv_select(prec, *p3, o));
    p3->R = nullptr;
    return same;
}

// recs: the model's nconv convolution records in canonical order.  tap >= 0 (icl_embed_taps): the pass ends after the stem + maxpool (0) or after
// bottleneck `tap` (1..16) and plan.out is the buffer that holds that tensor; nothing else differs.  tap < 0: avgpool (and fc for the dense head).
static inline fwd_plan forward_make_plan(const icl_conv_rec *recs, int nconv, int prec, int B, bool dense_head, int tap, const fwd_opts &o)
{
    fwd_plan p;
    p.B = B;
    const bool bf16 = prec == CONV_PREC_BF16, x3 = prec == CONV_PREC_BF16X3;
    const int bk = bf16 ? 64 : 32; // real channels per k-step
    int x = FWD_X, y = FWD_Y;
    auto add = [&](int kind, int layer, int xi, int yi) -> fwd_step & {
        fwd_step s = {};
        s.kind = kind; s.layer = layer; s.x = xi; s.y = yi; s.r = s.x2 = FWD_NONE;
        p.steps.push_back(s);
        return p.steps.back();
    };
    auto fail = [&](const char *why, int layer) { p.err = why; p.err_layer = layer; return p; };
    // a convolution step over the record's shape (stride s, input height h: the pruned forms differ there), residual buffer ri
    auto conv = [&](int layer, int xi, int yi, int ri, int h, int s, const prune_map *omap, int x2i) {
        const icl_conv_rec &r = recs[layer];
        fwd_step &st = add(FWD_CONV, layer, xi, yi);
        st.r = ri; st.x2 = x2i; st.ds = x2i != FWD_NONE;
        st.a = conv_plain(nullptr, nullptr, nullptr, ri != FWD_NONE ? (const void *)&st : nullptr, nullptr, nullptr, nullptr, B, h, r.cin, r.cout, r.k, s, r.pad, 1);
        if (st.ds) { // relu(bn3(conv3(t2)) + bn_ds(conv_ds(x))) as ONE dual-operand launch: the downsample tensor never exists
            const icl_conv_rec &d = recs[layer + 1];
            conv_add_operand(st.a, &st, d.hin, d.cin, d.stride);
        }
        if (omap) st.a.omap = *omap;
        st.c = conv_select(prec, st.a, o.conv);
        st.a.R = st.a.X2 = nullptr;
        st.blocks = st.c.blocks * (st.c.split ? 2u : 1u);
        st.threads = st.c.threads;
    };
    auto check = [&](int layer, int h, int s) -> const char * { // what launch_conv refuses
        const icl_conv_rec &r = recs[layer];
        const int ho = (h + 2 * r.pad - r.k) / s + 1;
        if ((int64_t)B * ho * ho >= (1LL << 31)) return "conv: the output pixels exceed the kernel's 32-bit pixel index";
        if (r.cin % bk || r.cout % 64) return "conv shape not supported by the implicit-GEMM kernel";
        return nullptr;
    };
    // ---- stem: conv0 + BN + ReLU + maxpool in one launch (BF16X3 has the fused stem only), or the two kernels
    if ((o.fuse & 1) || x3) {
        fwd_step &st = add(bf16 && (o.fuse & 8) ? FWD_STEM2_POOL : FWD_STEM_POOL, 0, FWD_NONE, x);
        st.blocks = fwd_stem_blocks((int64_t)B * FWD_STEM_STRIPS, o.stem_per_cu, o.conv.ncu, o.stem_max_blocks);
        st.threads = 256;
    } else {
        fwd_step &st = add(FWD_STEM, 0, FWD_NONE, y);
        st.blocks = fwd_stem_blocks((int64_t)B * 98, o.stem_per_cu, o.conv.ncu, o.stem_max_blocks); // 8x16-pixel tiles: 14 x 7 per image
        st.threads = 256;
        fwd_step &mp = add(FWD_MAXPOOL, 0, y, x);
        mp.blocks = 256 * 8;
        mp.threads = 256;
    }
    int ci = 1;
    for (int blk = 0; ci < nconv && blk != tap; ++blk) {
        const icl_conv_rec &c1 = recs[ci], &c2 = recs[ci + 1], &c3 = recs[ci + 2];
        const bool has_ds = c1.block == 0;
        const int cn = ci + (has_ds ? 4 : 3);
        p.H = c3.hout;
        p.C = c3.cout;
        if (bf16 && c1.stage == 1 && (o.fuse & (has_ds ? 4 : 2))) { // the whole bottleneck in one launch
            fwd_step &st = add(FWD_BNECK56, ci, x, y);
            st.ds = has_ds;
            // dead pixels (the rule of the layer-by-layer path below, on the same records): the block after this one reads at stride 2 only
            st.sub = (o.prune && o.prune_fused && !has_ds && blk + 1 != tap && cn + 3 < nconv && prune_stride(c2, c3, &recs[cn], &recs[cn + 3]) == 2) ? 2 : 1;
            int nstrips, ngroups;
            bneck56_grid(B, c2.hin, o.conv.ncu, &nstrips, &ngroups);
            st.blocks = (unsigned)(nstrips * ngroups);
            st.threads = 512;
            std::swap(x, y);
            ci = cn;
            continue;
        }
        for (int l = ci; l < ci + 3; ++l)
            if (const char *why = check(l, recs[l].hin, recs[l].stride)) return fail(why, l);
        if (c1.hout != (c1.hin - c1.k + 2 * c1.pad) / c1.stride + 1 || c2.hout != (c2.hin - c2.k + 2 * c2.pad) / c2.stride + 1 || c3.hout != c3.hin)
            return fail("conv shape not supported by the implicit-GEMM kernel", ci);
        conv(ci, x, FWD_T1, FWD_NONE, c1.hin, c1.stride, nullptr, FWD_NONE);
        // dead pixels: the block after this one reads its input at stride s only (never the block whose tensor a tap returns)
        conv_args p2, p3;
        if (bf16 && o.prune && !has_ds && blk + 1 != tap && cn + 3 < nconv &&
            plan_pruned_block(c2, c3, prune_stride(c2, c3, &recs[cn], &recs[cn + 3]), B, o.conv, &p2, &p3)) {
            conv(ci + 1, FWD_T1, FWD_T2, FWD_NONE, c2.hin, p2.stride, nullptr, FWD_NONE); // 3x3 / stride s: compact [B][h/s][h/s][mid]
            conv(ci + 2, FWD_T2, y, x, p3.H, 1, &p3.omap, FWD_NONE); // 1x1 over the compact tensor; residual and output at (s oy, s ox) of the full tensors
            p.steps.back().pruned = true;
            ++p.pruned;
        } else {
            conv(ci + 1, FWD_T1, FWD_T2, FWD_NONE, c2.hin, c2.stride, nullptr, FWD_NONE);
            if (has_ds) {
                const icl_conv_rec &d = recs[ci + 3];
                if (d.cin % bk || c3.cout % 128) return fail("fused downsample shape not supported", ci + 2);
                conv(ci + 2, FWD_T2, y, FWD_NONE, c3.hin, 1, nullptr, x);
            } else {
                conv(ci + 2, FWD_T2, y, x, c3.hin, 1, nullptr, FWD_NONE); // relu(bn(conv) + residual)
            }
        }
        std::swap(x, y);
        ci = cn;
    }
    for (const fwd_step &s : p.steps)
        if (s.kind == FWD_CONV && s.c.family == CONV_UNSUPPORTED) return fail(s.c.why, s.layer);
    p.out = x;
    if (tap >= 0) return p;
    fwd_step &ap = add(FWD_AVGPOOL, 0, x, FWD_NONE);
    ap.blocks = (unsigned)conv_ceil_div((int64_t)B * 2048, 256);
    ap.threads = 256;
    if (dense_head) {
        fwd_step &fc = add(FWD_FC, 0, FWD_NONE, FWD_NONE);
        const int64_t want = conv_ceil_div((int64_t)B * 1000, 4);
        fc.blocks = (unsigned)(want < 4096 ? want : 4096);
        fc.threads = 256;
    }
    return p;
}
