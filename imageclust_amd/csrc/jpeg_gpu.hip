// jpeg_gpu.hip -- batched image-file ingest: the host keeps the serial part of JPEG decoding (parsing + Huffman decoding,
// stage A of jpeg_decode.hip), the GPU rebuilds the pixels (stage B: dequantisation, islow IDCT, fancy upsampling, YCbCr->RGB)
// together with the EXIF orientation and the 224x224 resize, bit-identical to the host path (icl_load_image_224).
//
// Data per slab (one pinned host buffer, uploaded in three copies on the context's stream):
//   ingest_image[nimg]  one per output row: kind, sizes, orientation, plane offsets, the host-computed resize tables
//   ingest_plane[np]    one per JPEG component: block range, payload offsets, quantisation table
//   payload             per component: uint32 block offsets (nblocks + 1), then the int16 coefficients of every block in
//                       zig-zag order up to its last non-zero one; PNG / PPM / fallback images as finished 224x224x3 rows;
//                       with ICL_PNG_GPU a qualifying PNG as icl_png_desc + its zlib stream (KIND_PSTREAM; kernels: png_gpu.hip)
// Kernels: jpeg_idct_kernel (one thread per 8x8 block -> u8 planes in a scratch), jpeg_gather_resize_kernel (one thread per
// output pixel: reads the 2x2 source pixels of the resize through the orientation map, upsamples the chroma at those
// positions only, converts the colour and resizes).  Nothing is built at full-resolution RGB.
//
// Host driver: ingest_files = one ingest_pass in the context's entropy and PNG modes (ingest_modes) + a repair pass with both on the host over
// the files the GPU entropy check or the GPU PNG check (png_gpu.hip) rejected.  ingest_pass = ingest_buffers, then per slab slab_collect (rows in file order from the worker threads' ingest_feed,
// ingest_feed.h, into a pinned slab; slab_fill::fits says when a slab is full) -> run_slab_decode (upload, entropy decode, IDCT) ->
// slab_deliver (gather / resize, forward pass, NaN rows of failed files, into the call's ingest_sink), then tally_accepted.
// The batched downsizer at the end of the file (icl_downsize_images[_mem]) has a driver of the same shape, downsize_images_locked: per
// round dz_collect (images in list order into a dz_round, the JPEGs placed in the pinned slab; dz_round::admits says when a round is full)
// -> dz_rebuild (run_slab_decode to the planes, then per attempt a gather / resize at each image's own size and the JPEG encoder,
// jpeg_encode_gpu.hip) -> dz_deliver (files, statuses, failures and dz_totals in list order).
// Both drivers share the worker pool (worker_count, feed_worker), the failure capture of a worker (fail_from_tls, decoder_guard), the
// report of the lowest failed file (report_lowest), and, with the two test hooks, the placement code (slab_of_one).
#include "icl_common.h"
#include "ingest_feed.h"
#include "ingest_pixels.h"
#include "ingest_slab.h"
#include "jpeg_stage.h"
#include "png_stage.h"
#include "resnet_model.h" // icl_embed_dev_locked

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <thread>

namespace {

constexpr int OUTW = ICL_OUTW, OUTH = ICL_OUTH;
// (the row kinds and ingest_image: ingest_slab.h)

struct ingest_plane {
    int64_t first_block; // flat block index over the slab
    int64_t plane_off, plane_bytes;
    int64_t offs_off, coef_off; // payload byte offsets
    int32_t nblocks, wblocks;
    uint32_t ncoef;
    int32_t pad_;
    uint16_t qt[64]; // natural order
};

constexpr int IDCT_THREADS = 64;
constexpr int IDCT_SLOT = 65; // ints per thread in LDS (odd stride: no bank conflicts between the threads' slots)

// columns, rows, and the block's 8 x 8 pixels into its plane (shared by the two input forms below)
__device__ __forceinline__ void idct_store(const int *coef, uint8_t *dst, int64_t stride)
{
    int ws[64];
#pragma unroll
    for (int c = 0; c < 8; ++c) icl_idct_islow_col(coef + c, ws + c); // branch-free (the host's all-AC-zero shortcut gives the same values)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        int px[8];
        icl_idct_islow_row(ws + 8 * r, px);
        uint2 v;
        v.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
        v.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
        *(uint2 *)(dst + r * stride) = v; // plane offsets and strides are multiples of 8
    }
}

// IJG jidctint.c jpeg_idct_islow (ingest_pixels.h, as in host stage B): one thread per block; the dequantised coefficients are
// scattered from zig-zag order into the thread's LDS slot.
__global__ void __launch_bounds__(IDCT_THREADS) jpeg_idct_kernel(const ingest_plane *__restrict__ planes, int nplanes, const uint8_t *__restrict__ payload,
                                                                 int64_t payload_bytes, uint8_t *__restrict__ scratch, int64_t scratch_bytes, int64_t total_blocks)
{
    __shared__ int lds[IDCT_THREADS * IDCT_SLOT];
    int *coef = lds + threadIdx.x * IDCT_SLOT;
    const int64_t g = (int64_t)blockIdx.x * IDCT_THREADS + threadIdx.x;
    if (g >= total_blocks) return;
    int lo = 0, hi = nplanes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (planes[mid].first_block <= g) lo = mid;
        else hi = mid - 1;
    }
    const ingest_plane &P = planes[lo];
    const int64_t b = g - P.first_block;
    if (b < 0 || b >= P.nblocks || P.wblocks <= 0) return;
    // every offset was computed and validated on the host; these checks keep the kernel inside its buffers regardless
    if (P.offs_off < 0 || P.offs_off + ((int64_t)P.nblocks + 1) * 4 > payload_bytes || P.coef_off < 0 || P.coef_off + (int64_t)P.ncoef * 2 > payload_bytes) return;
    const int64_t stride = (int64_t)P.wblocks * 8, by = b / P.wblocks, bx = b - by * P.wblocks;
    const int64_t o = P.plane_off + by * 8 * stride + bx * 8;
    if (P.plane_off < 0 || P.plane_off + P.plane_bytes > scratch_bytes || (by * 8 + 7) * stride + bx * 8 + 8 > P.plane_bytes) return;
    const uint32_t *offs = (const uint32_t *)(payload + P.offs_off);
    const uint32_t o0 = offs[b], o1 = offs[b + 1];
    const int cnt = (o1 >= o0 && o1 - o0 <= 64 && o1 <= P.ncoef) ? (int)(o1 - o0) : 0;
    const int16_t *cf = (const int16_t *)(payload + P.coef_off) + o0;
#pragma unroll
    for (int i = 0; i < 64; ++i) coef[i] = 0;
    for (int i = 0; i < cnt; ++i) {
        const int z = icl_zigzag[i];
        coef[z] = (int)cf[i] * (int)P.qt[z];
    }
    idct_store(coef, scratch + o, stride);
}

// The dense-input form for planes whose coefficients were decoded on the GPU (jpeg_huff_gpu.hip): 64 int16 per block in natural order
// at byte offset coef_off of `dense` (such a plane has offs_off == -1, which the packed-input kernel above skips).
__global__ void __launch_bounds__(IDCT_THREADS) jpeg_idct_dense_kernel(const ingest_plane *__restrict__ planes, int nplanes, const int16_t *__restrict__ dense,
                                                                       int64_t dense_bytes, uint8_t *__restrict__ scratch, int64_t scratch_bytes, int64_t total_blocks)
{
    __shared__ int lds[IDCT_THREADS * IDCT_SLOT];
    int *coef = lds + threadIdx.x * IDCT_SLOT;
    const int64_t g = (int64_t)blockIdx.x * IDCT_THREADS + threadIdx.x;
    if (g >= total_blocks) return;
    int lo = 0, hi = nplanes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (planes[mid].first_block <= g) lo = mid;
        else hi = mid - 1;
    }
    const ingest_plane &P = planes[lo];
    const int64_t b = g - P.first_block;
    if (b < 0 || b >= P.nblocks || P.wblocks <= 0 || P.offs_off != -1) return;
    if (P.coef_off < 0 || (P.coef_off & 15) || P.coef_off + (int64_t)P.nblocks * 128 > dense_bytes) return;
    const int64_t stride = (int64_t)P.wblocks * 8, by = b / P.wblocks, bx = b - by * P.wblocks;
    const int64_t o = P.plane_off + by * 8 * stride + bx * 8;
    if (P.plane_off < 0 || P.plane_off + P.plane_bytes > scratch_bytes || (by * 8 + 7) * stride + bx * 8 + 8 > P.plane_bytes) return;
    const uint4 *cf = (const uint4 *)((const uint8_t *)dense + P.coef_off + b * 128);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint4 v = cf[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            coef[q * 8 + 2 * e] = (int)(int16_t)(w[e] & 0xffffu) * (int)P.qt[q * 8 + 2 * e];
            coef[q * 8 + 2 * e + 1] = (int)(int16_t)(w[e] >> 16) * (int)P.qt[q * 8 + 2 * e + 1];
        }
    }
    idct_store(coef, scratch + o, stride);
}

// the chroma sample at (X, y) of the full-resolution image from D's chroma plane pl (fancy upsampling: ingest_pixels.h)
__device__ __forceinline__ int chroma_at(const ingest_image &D, const uint8_t *pl, int X, int y)
{
    return icl_fancy_upsample(pl, D.cstride, D.cw, D.chh, D.hs, D.vs, X, y);
}

// RGB of pixel (x, y) of the ORIENTED image: the orientation map, fancy upsampling of the chroma at that pixel only, colour conversion
__device__ __forceinline__ void rgb_at(const ingest_image &D, const uint8_t *scratch, int x, int y, int &R, int &G, int &B)
{
    const int sw = D.W, sh = D.H;
    int sx, sy;
    icl_exif_source(D.orient, sw, sh, x, y, sx, sy);
    sx = min(max(sx, 0), sw - 1);
    sy = min(max(sy, 0), sh - 1);
    const int Y = scratch[D.yplane + (int64_t)sy * D.ystride + sx];
    if (D.ncomp == 1) { R = G = B = Y; return; }
    const int cb = chroma_at(D, scratch + D.cplane[0], sx, sy), cr = chroma_at(D, scratch + D.cplane[1], sx, sy);
    if (D.is_rgb) { R = Y; G = cb; B = cr; return; }
    icl_ycc_to_rgb(Y, cb, cr, R, G, B);
}

// one thread per output pixel of one image: cv::resize INTER_LINEAR (OpenCV's two-pass fixed-point rounding) or, for an exact
// 2x2 decimation, INTER_AREA (ingest_pixels.h), with the offset / weight tables computed on the host (icl_resize_coeffs)
// RGB of pixel (x, y) of a KIND_PSTREAM image from its unfiltered scanlines (D: its checked descriptor, icl_png_job)
__device__ __forceinline__ void png_rgb_at(const icl_png_desc *D, const uint8_t *lines, int x, int y, int &R, int &G, int &B)
{
    x = min(max(x, 0), D->w - 1);
    y = min(max(y, 0), D->h - 1);
    icl_png_sample_rgb(lines + (int64_t)y * ((int64_t)D->rowb + 1) + 1, x, D->ctype, D->depth, D->pal, R, G, B);
}

__global__ void __launch_bounds__(256) jpeg_gather_resize_kernel(const ingest_image *__restrict__ imgs, const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                                 const uint8_t *__restrict__ scratch, int64_t scratch_bytes, uint8_t *__restrict__ dst)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= OUTW * OUTH) return;
    const ingest_image &D = imgs[blockIdx.y];
    uint8_t *o = dst + (int64_t)blockIdx.y * ICL_IMG_BYTES + (int64_t)p * 3;
    if (D.kind == KIND_HOST) {
        if (D.host_off >= 0 && D.host_off + ICL_IMG_BYTES <= payload_bytes) {
            const uint8_t *s = payload + D.host_off + (int64_t)p * 3;
            o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        } else {
            o[0] = o[1] = o[2] = 0;
        }
        return;
    }
    const int dx = p % OUTW, dy = p / OUTW;
    int r[4], g[4], b[4];
    if (D.kind == KIND_PSTREAM) { // a PNG's scanlines (png_gpu.hip): the same four samples per output pixel; no EXIF step
        const icl_png_desc *P = icl_png_job(D, payload, payload_bytes, scratch_bytes);
        if (!P) { o[0] = o[1] = o[2] = 0; return; }
        const uint8_t *lines = scratch + D.yplane;
        if (D.area) {
            png_rgb_at(P, lines, 2 * dx, 2 * dy, r[0], g[0], b[0]);
            png_rgb_at(P, lines, 2 * dx + 1, 2 * dy, r[1], g[1], b[1]);
            png_rgb_at(P, lines, 2 * dx, 2 * dy + 1, r[2], g[2], b[2]);
            png_rgb_at(P, lines, 2 * dx + 1, 2 * dy + 1, r[3], g[3], b[3]);
            o[0] = icl_area_mean(r[0], r[1], r[2], r[3]);
            o[1] = icl_area_mean(g[0], g[1], g[2], g[3]);
            o[2] = icl_area_mean(b[0], b[1], b[2], b[3]);
            return;
        }
        const int sx = min(max(D.xofs[dx], 0), D.ow - 1), sx1 = min(sx + 1, D.ow - 1);
        const int sy = min(max(D.yofs[dy], 0), D.oh - 1), sy1 = min(sy + 1, D.oh - 1);
        png_rgb_at(P, lines, sx, sy, r[0], g[0], b[0]);
        png_rgb_at(P, lines, sx1, sy, r[1], g[1], b[1]);
        png_rgb_at(P, lines, sx, sy1, r[2], g[2], b[2]);
        png_rgb_at(P, lines, sx1, sy1, r[3], g[3], b[3]);
        const int a0 = D.xa[dx * 2], a1 = D.xa[dx * 2 + 1], b0 = D.ya[dy * 2], b1 = D.ya[dy * 2 + 1];
        o[0] = icl_resize_linear(r[0], r[1], r[2], r[3], a0, a1, b0, b1);
        o[1] = icl_resize_linear(g[0], g[1], g[2], g[3], a0, a1, b0, b1);
        o[2] = icl_resize_linear(b[0], b[1], b[2], b[3], a0, a1, b0, b1);
        return;
    }
    if (D.kind != KIND_JPEG) { o[0] = o[1] = o[2] = 0; return; }
    if (D.area) {
        rgb_at(D, scratch, 2 * dx, 2 * dy, r[0], g[0], b[0]);
        rgb_at(D, scratch, 2 * dx + 1, 2 * dy, r[1], g[1], b[1]);
        rgb_at(D, scratch, 2 * dx, 2 * dy + 1, r[2], g[2], b[2]);
        rgb_at(D, scratch, 2 * dx + 1, 2 * dy + 1, r[3], g[3], b[3]);
        o[0] = icl_area_mean(r[0], r[1], r[2], r[3]);
        o[1] = icl_area_mean(g[0], g[1], g[2], g[3]);
        o[2] = icl_area_mean(b[0], b[1], b[2], b[3]);
        return;
    }
    const int sx = min(max(D.xofs[dx], 0), D.ow - 1), sx1 = min(sx + 1, D.ow - 1);
    const int sy = min(max(D.yofs[dy], 0), D.oh - 1), sy1 = min(sy + 1, D.oh - 1);
    rgb_at(D, scratch, sx, sy, r[0], g[0], b[0]);
    rgb_at(D, scratch, sx1, sy, r[1], g[1], b[1]);
    rgb_at(D, scratch, sx, sy1, r[2], g[2], b[2]);
    rgb_at(D, scratch, sx1, sy1, r[3], g[3], b[3]);
    const int a0 = D.xa[dx * 2], a1 = D.xa[dx * 2 + 1], b0 = D.ya[dy * 2], b1 = D.ya[dy * 2 + 1];
    o[0] = icl_resize_linear(r[0], r[1], r[2], r[3], a0, a1, b0, b1);
    o[1] = icl_resize_linear(g[0], g[1], g[2], g[3], a0, a1, b0, b1);
    o[2] = icl_resize_linear(b[0], b[1], b[2], b[3], a0, a1, b0, b1);
}

__global__ void fill_nan_rows_kernel(float *out, const int32_t *rows, int nrows, int head)
{
    const int r = blockIdx.y;
    if (r >= nrows) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < head; i += gridDim.x * 256) out[(int64_t)rows[r] * head + i] = __int_as_float(0x7fc00000);
}

// ---- host side -------------------------------------------------------------------------------------------------------

constexpr int64_t SLAB_IMAGES = 256;                 // output rows per slab (the forward pass's batch)
constexpr int64_t SLAB_PAYLOAD = 128ll << 20;        // coefficient / stream / finished-image bytes per slab (pinned, two of them)
constexpr int64_t SLAB_SCRATCH = 768ll << 20;        // u8 planes of one slab on the device
constexpr int64_t SLAB_COEF = 2 * SLAB_SCRATCH;      // ICL_ENTROPY_GPU: dense int16 coefficients of one slab (two bytes per plane sample)
constexpr int64_t SLAB_SUBS = SLAB_PAYLOAD / (ICL_JE_SUB_BITS / 8); // ... subsequences of one slab
constexpr int64_t SLAB_WGS = SLAB_SUBS / ICL_JE_WG + SLAB_IMAGES;   // ... workgroups (every image rounds up)
constexpr int64_t HDR_SCANS = SLAB_IMAGES * (int64_t)sizeof(ingest_image) + 3 * SLAB_IMAGES * (int64_t)sizeof(ingest_plane); // offset of the scan descriptors
constexpr int64_t HDR_BYTES = HDR_SCANS + SLAB_IMAGES * (int64_t)sizeof(icl_je_scan);
// slab_fill::fits (below) tests rows, payload, scratch and subsequences; the other limits follow from those:
static_assert(ICL_PNG_PAYLOAD_CAP == SLAB_PAYLOAD && ICL_PNG_WANT_CAP <= SLAB_SCRATCH, "a qualifying PNG (png_stage.h) alone fits a slab");
static_assert(SLAB_COEF == 2 * SLAB_SCRATCH, "a stream plane's dense coefficients are two bytes per plane sample: coef_used <= 2 * scratch_used");
static_assert(SLAB_WGS == SLAB_SUBS / ICL_JE_WG + SLAB_IMAGES, "sum of ceil(nsub_i / WG) over k <= SLAB_IMAGES scans <= floor(sum nsub_i / WG) + k");
// (scans: at most one per row, SLAB_IMAGES of them in the header; planes: at most three per row, 3 * SLAB_IMAGES in the header)

// the parts of a slab: its header (HDR_BYTES: images, planes, scan descriptors) and its payload, in pinned host or in device memory
struct slab_view {
    ingest_image *imgs;
    ingest_plane *planes;
    icl_je_scan *scans;
    uint8_t *payload;
    slab_view(uint8_t *hdr, uint8_t *pay)
        : imgs((ingest_image *)hdr), planes((ingest_plane *)(hdr + SLAB_IMAGES * sizeof(ingest_image))), scans((icl_je_scan *)(hdr + HDR_SCANS)), payload(pay)
    {
    }
    // a row's start: its descriptor cleared up to the resize tables (place_* and the collectors fill in what the row's kind needs)
    void clear_row(int i) const { memset(&imgs[i], 0, offsetof(ingest_image, xofs)); }
};

static int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

struct comp_meta {
    int32_t wblocks, hblocks, dw, dh;
    int64_t offs_off, coef_off; // within the file's packed buffer
    uint32_t ncoef;
};

struct file_result { // what a worker hands the slab builder for one file
    int kind = KIND_FAILED;
    int rc = ICL_OK;
    std::string err;
    int W = 0, H = 0, ncomp = 0, hs = 1, vs = 1, is_rgb = 0, orient = 1;
    uint16_t qt[3][64];
    comp_meta cm[3];
    // KIND_JPEG: the components' block offsets + coefficients; KIND_HOST: the 224x224x3 image; KIND_JSTREAM: Huffman tables, restart
    // intervals, unstuffed stream (scan holds their offsets within this buffer)
    std::vector<uint8_t> packed;
    icl_je_scan scan;
    int64_t plane_bytes = 0;
    bool host_entropy = false; // a JPEG whose entropy decoder ran on the host
    bool host_png = false;     // a PNG that took the host decoder
};

struct ingest_modes { // where the serial part of a file's decoding runs: ICL_ENTROPY_*, ICL_PNG_*
    int entropy, png;
};
constexpr ingest_modes MODES_HOST = {ICL_ENTROPY_HOST, ICL_PNG_HOST};

static int64_t plane_bytes_of(const icl_jpeg_component &k) { return (int64_t)k.wblocks * 8 * k.hblocks * 8; }

static void frame_meta(const icl_jpeg_coefs &J, file_result &r)
{
    for (int c = 0; c < J.ncomp; ++c) {
        const icl_jpeg_component &k = J.comp[c];
        r.cm[c].wblocks = k.wblocks;
        r.cm[c].hblocks = k.hblocks;
        r.cm[c].dw = k.dw;
        r.cm[c].dh = k.dh;
        memcpy(r.qt[c], J.qt[c], sizeof r.qt[c]);
    }
    r.W = J.W;
    r.H = J.H;
    r.ncomp = J.ncomp;
    r.hs = J.comp[0].h;
    r.vs = J.comp[0].v;
    r.is_rgb = J.is_rgb ? 1 : 0;
    r.orient = J.orient;
}

// Stage-A output -> the compact per-block form: uint32 offsets (nblocks + 1) and the zig-zag coefficients up to each block's
// last non-zero one.  Returns false when the image does not fit one slab (it then takes the host path).
static bool pack_jpeg(const icl_jpeg_coefs &J, file_result &r, std::vector<uint32_t> &offs)
{
    int64_t total = 0, planes = 0;
    uint32_t ncoef[3] = {0, 0, 0};
    for (int c = 0; c < J.ncomp; ++c) {
        const icl_jpeg_component &k = J.comp[c];
        const int64_t nb = (int64_t)k.wblocks * k.hblocks;
        planes += plane_bytes_of(k);
        uint64_t nc = 0;
        for (int64_t b = 0; b < nb; ++b) {
            const int16_t *cf = k.coefs.data() + b * 64;
            int e = 63;
            while (e >= 0 && cf[icl_zigzag[e]] == 0) --e;
            nc += (uint64_t)(e + 1);
        }
        if (nc > 0xffffffffull) return false;
        ncoef[c] = (uint32_t)nc;
        total += align16((nb + 1) * 4) + align16((int64_t)nc * 2);
    }
    if (total > SLAB_PAYLOAD || planes > SLAB_SCRATCH) return false;
    r.packed.resize((size_t)total);
    r.plane_bytes = planes;
    frame_meta(J, r);
    int64_t pos = 0;
    for (int c = 0; c < J.ncomp; ++c) {
        const icl_jpeg_component &k = J.comp[c];
        const int64_t nb = (int64_t)k.wblocks * k.hblocks;
        comp_meta &m = r.cm[c];
        m.ncoef = ncoef[c];
        m.offs_off = pos;
        m.coef_off = pos + align16((nb + 1) * 4);
        offs.resize((size_t)nb + 1);
        int16_t *out = (int16_t *)(r.packed.data() + m.coef_off);
        uint32_t at = 0;
        for (int64_t b = 0; b < nb; ++b) {
            const int16_t *cf = k.coefs.data() + b * 64;
            int e = 63;
            while (e >= 0 && cf[icl_zigzag[e]] == 0) --e;
            offs[(size_t)b] = at;
            for (int i = 0; i <= e; ++i) out[at + i] = cf[icl_zigzag[i]];
            at += (uint32_t)(e + 1);
        }
        offs[(size_t)nb] = at;
        memcpy(r.packed.data() + m.offs_off, offs.data(), ((size_t)nb + 1) * 4);
        pos = m.coef_off + align16((int64_t)m.ncoef * 2);
    }
    return true;
}

// Host stage P0 (icl_png_parse) -> descriptor + zlib stream in one buffer (KIND_PSTREAM).  Returns false when the file does not qualify for
// the GPU route (its parse fails, it is interlaced, or it does not fit one slab): it then takes the host decoder, which reports what is wrong.
static bool pack_png(const uint8_t *data, size_t len, file_result &r)
{
    icl_png_parsed P;
    const size_t hdr = sizeof(icl_png_desc);
    r.packed.assign(hdr, 0);
    if (icl_png_parse(data, len, P, r.packed) != nullptr || !icl_png_qualifies(P, r.packed.size() - hdr)) {
        r.packed.clear();
        return false;
    }
    icl_png_desc D;
    icl_png_describe(P, r.packed.data() + hdr, r.packed.size() - hdr, D);
    memcpy(r.packed.data(), &D, sizeof D);
    r.W = (int)P.w;
    r.H = (int)P.h;
    r.plane_bytes = (int64_t)P.want;
    return true;
}

// Stage-A0 output -> one buffer: tables, intervals, stream (each on a 16-byte boundary).  Returns false when the image does not fit one slab.
static bool pack_stream(const icl_jpeg_coefs &J, const icl_jpeg_a0 &A, file_result &r)
{
    int64_t planes = 0;
    for (int c = 0; c < J.ncomp; ++c) planes += align16(plane_bytes_of(J.comp[c]));
    const int64_t tb = align16((int64_t)(2 * J.ncomp) * (int64_t)sizeof(icl_je_table)), ib = align16((int64_t)A.intervals.size() * (int64_t)sizeof(icl_je_interval));
    const int64_t sbytes = (int64_t)A.scan.nsub * (A.scan.sub_bits / 8);
    if ((int64_t)A.stream.size() != sbytes || tb + ib + sbytes > SLAB_PAYLOAD || planes > SLAB_SCRATCH || (int64_t)A.scan.nsub > SLAB_SUBS) return false;
    r.packed.resize((size_t)(tb + ib + sbytes));
    memcpy(r.packed.data(), A.tables, (size_t)(2 * J.ncomp) * sizeof(icl_je_table));
    memcpy(r.packed.data() + tb, A.intervals.data(), A.intervals.size() * sizeof(icl_je_interval));
    memcpy(r.packed.data() + tb + ib, A.stream.data(), (size_t)sbytes);
    r.scan = A.scan;
    r.scan.tables_off = 0;
    r.scan.intervals_off = tb;
    r.scan.stream_off = tb + ib;
    r.plane_bytes = planes;
    frame_meta(J, r);
    return true;
}

struct worker_state { // buffers a worker reuses from file to file
    icl_jpeg_coefs J;
    icl_jpeg_a0 A;
    std::vector<uint32_t> offs;
};

// A worker's failure into its result: the code, and the calling thread's last error text (what icl_fail left there).
static void fail_from_tls(file_result &r, int rc)
{
    r.kind = KIND_FAILED;
    r.rc = rc;
    r.err = icl_last_error(nullptr);
}

// body() on a worker thread; what a decoder throws becomes the failed result r of the image the messages call `name`.  false: it threw.
template <class Body> static bool decoder_guard(file_result &r, const char *name, const Body &body)
{
    auto threw = [&](int rc, const char *why) {
        r.kind = KIND_FAILED;
        r.rc = rc;
        r.err = std::string("failed to read image: ") + name + why;
        return false;
    };
    try {
        body();
        return true;
    } catch (const std::bad_alloc &) {
        return threw(ICL_ERR_NOMEM, ". Out of host memory while decoding");
    } catch (...) {
        return threw(ICL_ERR_IO, ". Decoder error");
    }
}

// One image (a file, or a memory source read in place: icl_image_src_read), on a worker thread: stage A0 for a JPEG whose entropy decoder runs on the GPU (entropy == ICL_ENTROPY_GPU and the file
// qualifies), stage A for every other JPEG the GPU takes, stage P0 for a PNG that qualifies for the GPU route (modes.png == ICL_PNG_GPU), the whole host path for everything else.  Status codes and messages are
// those of icl_load_image_224 (image_io.hip).
// finish_host(rgb, w, h) turns a host-decoded image into the result's KIND_HOST payload (or fails it: it returns false after icl_fail).
template <class FinishHost>
static void process_file_with(const ingest_src &src, const char *path /* what the messages call the image */, worker_state &ws, const ingest_modes &modes, file_result &r,
                              const FinishHost &finish_host)
{
    icl_jpeg_coefs &J = ws.J;
    decoder_guard(r, path, [&]() {
        std::vector<uint8_t> file, rgb;
        int w = 0, h = 0;
        const uint8_t *data;
        size_t len;
        const int fmt = icl_image_src_read(src, file, data, len);
        if (fmt == ICL_IMAGE_JPEG) {
            if (modes.entropy == ICL_ENTROPY_GPU) {
                bool qualifies = false;
                (void)icl_jpeg_stage_a0(data, len, path, ICL_JE_SUB_BITS, J, ws.A, qualifies); // (an error: the usual route reports it)
                if (qualifies && pack_stream(J, ws.A, r)) {
                    r.kind = KIND_JSTREAM;
                    return;
                }
            }
            r.host_entropy = true;
            const int rc = icl_jpeg_stage_a(nullptr, data, len, path, J);
            if (rc) return fail_from_tls(r, rc);
            if (pack_jpeg(J, r, ws.offs)) {
                r.kind = KIND_JPEG;
                return;
            }
            // too large for one slab: stage B on the host (the file has already been through stage A)
            w = J.W;
            h = J.H;
            const int rc2 = icl_jpeg_stage_b(nullptr, J, path, rgb);
            if (rc2) return fail_from_tls(r, rc2);
            icl_apply_exif_orientation(rgb, w, h, J.orient);
        } else { // PNG, PPM, or a file that cannot be read / an empty buffer: the host path decodes it or reports why not
            if (fmt == ICL_IMAGE_PNG) {
                if (modes.png == ICL_PNG_GPU && pack_png(data, len, r)) {
                    r.kind = KIND_PSTREAM;
                    return;
                }
                r.host_png = true;
            }
            const int rc = icl_image_decode(nullptr, src, path, fmt, data, len, rgb, w, h);
            if (rc) return fail_from_tls(r, rc);
        }
        if (!finish_host(rgb, w, h)) return fail_from_tls(r, ICL_ERR_ARG);
        r.kind = KIND_HOST;
    });
}

static void process_file(const ingest_src &src, worker_state &ws, const ingest_modes &modes, file_result &r)
{
    char nbuf[96];
    process_file_with(src, ingest_src_name(src, nbuf, sizeof nbuf), ws, modes, r, [&](std::vector<uint8_t> &rgb, int w, int h) {
        r.packed.resize((size_t)ICL_IMG_BYTES);
        icl_resize_bilinear_u8(rgb.data(), w, h, r.packed.data(), OUTW, OUTH);
        return true;
    });
}

} // namespace

// Buffers of the batched file path, kept by the context between calls (freed by icl_destroy).
struct icl_ingest_ws {
    uint8_t *h_slab[2] = {nullptr, nullptr}; // pinned: header (images + planes + scans) then payload
    hipEvent_t ev_up[2] = {nullptr, nullptr};
    uint8_t *d_hdr = nullptr, *d_payload = nullptr, *d_scratch = nullptr, *d_img = nullptr;
    icl_dev_grow emb; // float[SLAB_IMAGES][head] of the widest head asked for so far (ingest_buffers)
    int32_t *d_rows = nullptr;
    // ICL_ENTROPY_GPU (allocated on first use)
    int16_t *d_coef = nullptr;
    icl_je_sub *d_sub = nullptr;
    uint32_t *d_bound = nullptr;
    int32_t *d_accepted = nullptr;
    int32_t *h_accepted = nullptr; // pinned: one flag per stream image of a call
    int64_t h_accepted_cap = 0;
    // ICL_PNG_GPU (allocated when the first slab with a PNG stream is built)
    int32_t *d_png_ok = nullptr;
    int32_t *h_png_ok = nullptr; // pinned: one flag per row of a call
    int64_t h_png_ok_cap = 0;
    slab_view host(int q) const { return slab_view(h_slab[q], h_slab[q] + HDR_BYTES); }
    slab_view dev() const { return slab_view(d_hdr, d_payload); }
    ~icl_ingest_ws()
    {
        for (int q = 0; q < 2; ++q) {
            if (h_slab[q]) (void)hipHostFree(h_slab[q]);
            if (ev_up[q]) (void)hipEventDestroy(ev_up[q]);
        }
        if (h_accepted) (void)hipHostFree(h_accepted);
        if (h_png_ok) (void)hipHostFree(h_png_ok);
        if (d_png_ok) (void)hipFree(d_png_ok);
        for (void *p : {(void *)d_hdr, (void *)d_payload, (void *)d_scratch, (void *)d_img, (void *)d_rows, (void *)d_coef, (void *)d_sub, (void *)d_bound,
                        (void *)d_accepted})
            if (p) (void)hipFree(p);
        emb.release();
    }
};

void icl_ingest_free(icl_ctx *ctx)
{
    delete ctx->ingest;
    ctx->ingest = nullptr;
}

static int ingest_ws(icl_ctx *ctx, icl_ingest_ws *&ws)
{
    if (!ctx->ingest) {
        std::unique_ptr<icl_ingest_ws> w(new icl_ingest_ws());
        for (int q = 0; q < 2; ++q) {
            if (hipHostMalloc((void **)&w->h_slab[q], (size_t)(HDR_BYTES + SLAB_PAYLOAD), hipHostMallocDefault) != hipSuccess) {
                w->h_slab[q] = nullptr;
                return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: pinned staging slab");
            }
            ICL_HIP(ctx, hipEventCreateWithFlags(&w->ev_up[q], hipEventDisableTiming));
        }
        if (hipMalloc((void **)&w->d_hdr, (size_t)HDR_BYTES) != hipSuccess || hipMalloc((void **)&w->d_payload, (size_t)SLAB_PAYLOAD) != hipSuccess ||
            hipMalloc((void **)&w->d_scratch, (size_t)SLAB_SCRATCH) != hipSuccess ||
            hipMalloc((void **)&w->d_img, (size_t)SLAB_IMAGES * ICL_IMG_BYTES) != hipSuccess ||
            hipMalloc((void **)&w->d_rows, (size_t)SLAB_IMAGES * 4) != hipSuccess)
            return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: device buffers");
        ctx->ingest = w.release();
    }
    ws = ctx->ingest;
    return ICL_OK;
}

// the buffers of the GPU entropy decoder; room for the accepted flags of a call with n files
static int entropy_ws(icl_ctx *ctx, icl_ingest_ws *ws, int64_t n)
{
    if (!ws->d_coef) {
        if (hipMalloc((void **)&ws->d_coef, (size_t)SLAB_COEF) != hipSuccess || hipMalloc((void **)&ws->d_sub, (size_t)SLAB_SUBS * sizeof(icl_je_sub)) != hipSuccess ||
            hipMalloc((void **)&ws->d_bound, (size_t)SLAB_WGS * 4 * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void **)&ws->d_accepted, (size_t)SLAB_IMAGES * 4) != hipSuccess)
            return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: device buffers of the entropy decoder");
    }
    if (ws->h_accepted_cap < n) {
        if (ws->h_accepted) (void)hipHostFree(ws->h_accepted);
        ws->h_accepted = nullptr;
        ws->h_accepted_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 4096);
        if (hipHostMalloc((void **)&ws->h_accepted, (size_t)cap * 4, hipHostMallocDefault) != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: pinned flags");
        ws->h_accepted_cap = cap;
    }
    return ICL_OK;
}

// the buffers of the GPU PNG route; room for the accepted flags of a call with n files
static int png_ws(icl_ctx *ctx, icl_ingest_ws *ws, int64_t n)
{
    if (!ws->d_png_ok && hipMalloc((void **)&ws->d_png_ok, (size_t)SLAB_IMAGES * 4) != hipSuccess) {
        ws->d_png_ok = nullptr;
        return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: device buffers of the PNG route");
    }
    if (ws->h_png_ok_cap < n) {
        if (ws->h_png_ok) (void)hipHostFree(ws->h_png_ok);
        ws->h_png_ok = nullptr;
        ws->h_png_ok_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 4096);
        if (hipHostMalloc((void **)&ws->h_png_ok, (size_t)cap * 4, hipHostMallocDefault) != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "file ingest: pinned flags");
        ws->h_png_ok_cap = cap;
    }
    return ICL_OK;
}

namespace {

// what the slab builder has placed so far
struct slab_fill {
    int nimg = 0, npl = 0, nscan = 0, npacked = 0, ndense = 0, npng = 0;
    int64_t used = 0, scratch_used = 0, blocks = 0, coef_used = 0 /* bytes */, subs = 0, wgs = 0;
    // What a slab holds: does r still fit behind what has been placed?  (A result alone always does: pack_jpeg / pack_stream / pack_png saw to it;
    // a PNG stream's "plane" is the `want` bytes of its scanlines.)
    bool fits(const file_result &r) const
    {
        const int64_t pay = r.kind == KIND_FAILED ? 0 : align16((int64_t)r.packed.size()), nsub = r.kind == KIND_JSTREAM ? (int64_t)r.scan.nsub : 0;
        return nimg < SLAB_IMAGES && used + pay <= SLAB_PAYLOAD && scratch_used + align16(r.plane_bytes) <= SLAB_SCRATCH && subs + nsub <= SLAB_SUBS;
    }
};

// One KIND_JPEG / KIND_JSTREAM result into the slab: image descriptor, planes, payload, and (stream) the scan descriptor.
static bool place_jpeg(const file_result &r, slab_fill &F, const slab_view &S)
{
    if (!F.fits(r)) return false;
    const bool stream = r.kind == KIND_JSTREAM;
    ingest_image &D = S.imgs[F.nimg];
    D.kind = KIND_JPEG;
    D.W = r.W;
    D.H = r.H;
    D.orient = r.orient;
    D.ncomp = r.ncomp;
    D.hs = r.hs;
    D.vs = r.vs;
    D.is_rgb = r.is_rgb;
    const bool swap = icl_exif_swaps_axes(r.orient);
    D.ow = swap ? r.H : r.W;
    D.oh = swap ? r.W : r.H;
    D.area = icl_resize_is_area(D.ow, D.oh, OUTW, OUTH);
    icl_resize_coeffs(OUTW, D.ow, D.xofs, D.xa);
    icl_resize_coeffs(OUTH, D.oh, D.yofs, D.ya);
    memcpy(S.payload + F.used, r.packed.data(), r.packed.size());
    icl_je_scan *sc = nullptr;
    if (stream) {
        sc = &S.scans[F.nscan++];
        *sc = r.scan;
        sc->tables_off += F.used;
        sc->intervals_off += F.used;
        sc->stream_off += F.used;
        sc->sub_first = F.subs;
        sc->wg_first = F.wgs;
        F.subs += sc->nsub;
        F.wgs += icl_ceil_div(sc->nsub, ICL_JE_WG);
    }
    for (int c = 0; c < r.ncomp; ++c) {
        const comp_meta &cm = r.cm[c];
        ingest_plane &P = S.planes[F.npl++];
        P.first_block = F.blocks;
        P.nblocks = cm.wblocks * cm.hblocks;
        P.wblocks = cm.wblocks;
        P.plane_off = F.scratch_used;
        P.plane_bytes = (int64_t)cm.wblocks * 8 * cm.hblocks * 8;
        if (stream) { // dense coefficients, written by the GPU decoder
            P.ncoef = 0;
            P.offs_off = -1;
            P.coef_off = F.coef_used;
            sc->coef_off[c] = F.coef_used / 2;
            F.coef_used += align16((int64_t)P.nblocks * 128);
            ++F.ndense;
        } else {
            P.ncoef = cm.ncoef;
            P.offs_off = F.used + cm.offs_off;
            P.coef_off = F.used + cm.coef_off;
            ++F.npacked;
        }
        memcpy(P.qt, r.qt[c], sizeof P.qt);
        F.blocks += P.nblocks;
        if (c == 0) {
            D.yplane = P.plane_off;
            D.ystride = cm.wblocks * 8;
            D.yrows = cm.hblocks * 8;
        } else {
            D.cplane[c - 1] = P.plane_off;
            D.cstride = cm.wblocks * 8;
            D.crows = cm.hblocks * 8;
            D.cw = cm.dw;
            D.chh = cm.dh;
        }
        F.scratch_used += align16(P.plane_bytes);
    }
    // sizes were produced by stage A / A0 + pack_* on this host; re-check what the kernels rely on
    const bool ok = D.W >= 1 && D.H >= 1 && D.W <= D.ystride && D.H <= D.yrows && (D.ncomp == 1 || (D.cw >= 1 && D.chh >= 1 && D.cw <= D.cstride && D.chh <= D.crows)) &&
                    F.scratch_used <= SLAB_SCRATCH && F.coef_used <= SLAB_COEF && F.wgs <= SLAB_WGS;
    F.used += align16((int64_t)r.packed.size());
    return ok;
}

// One KIND_PSTREAM result into the slab: image descriptor (resize tables; no EXIF step for PNG), descriptor + zlib stream into the payload,
// `want` bytes of the scratch for its scanlines.
static bool place_png(const file_result &r, slab_fill &F, const slab_view &S)
{
    if (!F.fits(r) || r.packed.size() < sizeof(icl_png_desc)) return false;
    ingest_image &D = S.imgs[F.nimg];
    D.kind = KIND_PSTREAM;
    D.W = D.ow = r.W;
    D.H = D.oh = r.H;
    D.orient = 1;
    D.area = icl_resize_is_area(D.ow, D.oh, OUTW, OUTH);
    icl_resize_coeffs(OUTW, D.ow, D.xofs, D.xa);
    icl_resize_coeffs(OUTH, D.oh, D.yofs, D.ya);
    memcpy(S.payload + F.used, r.packed.data(), r.packed.size());
    D.host_off = F.used;
    D.yplane = F.scratch_used;
    F.used += align16((int64_t)r.packed.size());
    F.scratch_used += align16(r.plane_bytes);
    ++F.npng;
    // what the kernels rely on, by their own check (the descriptor was made by pack_png on this host)
    return F.used <= SLAB_PAYLOAD && F.scratch_used <= SLAB_SCRATCH && icl_png_job(D, S.payload, SLAB_PAYLOAD, SLAB_SCRATCH) != nullptr;
}

// upload of a filled slab and its kernels up to the planes: (entropy decode,) IDCT; (PNG streams: inflate, Adler-32, and with png_stages >= 2
// the unfilter -- only icl_png_raw_files stops before it)
static int run_slab_decode(icl_ctx *ctx, icl_ingest_ws *ws, const slab_view &H, const slab_fill &F, int64_t &upload, int png_stages = 2)
{
    hipStream_t st = ctx->stream;
    const slab_view D = ws->dev();
    if (F.nimg) ICL_HIP(ctx, hipMemcpyAsync(D.imgs, H.imgs, (size_t)F.nimg * sizeof(ingest_image), hipMemcpyHostToDevice, st));
    if (F.npl) ICL_HIP(ctx, hipMemcpyAsync(D.planes, H.planes, (size_t)F.npl * sizeof(ingest_plane), hipMemcpyHostToDevice, st));
    if (F.nscan) ICL_HIP(ctx, hipMemcpyAsync(D.scans, H.scans, (size_t)F.nscan * sizeof(icl_je_scan), hipMemcpyHostToDevice, st));
    if (F.used) ICL_HIP(ctx, hipMemcpyAsync(D.payload, H.payload, (size_t)F.used, hipMemcpyHostToDevice, st));
    upload += (int64_t)F.nimg * (int64_t)sizeof(ingest_image) + (int64_t)F.npl * (int64_t)sizeof(ingest_plane) + (int64_t)F.nscan * (int64_t)sizeof(icl_je_scan) + F.used;
    if (F.nscan) {
        ICL_HIP(ctx, hipMemsetAsync(ws->d_coef, 0, (size_t)F.coef_used, st)); // blocks end at their EOB: the rest of a block is zero
        icl_je_slab s;
        s.d_scans = D.scans;
        s.nscans = F.nscan;
        s.d_payload = ws->d_payload;
        s.payload_bytes = SLAB_PAYLOAD;
        s.d_sub = ws->d_sub;
        s.nsub_cap = SLAB_SUBS;
        s.d_bound = ws->d_bound;
        s.nwg_cap = SLAB_WGS;
        s.total_wgs = F.wgs;
        s.d_accepted = ws->d_accepted;
        s.d_coef = ws->d_coef;
        s.coef_elems = SLAB_COEF / 2;
        ICL_TRY(icl_je_decode_slab(ctx, st, s));
    }
    if (F.npacked) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)icl_ceil_div(F.blocks, IDCT_THREADS)), dim3(IDCT_THREADS), 0, st, D.planes, F.npl, (const uint8_t *)ws->d_payload,
                           (int64_t)SLAB_PAYLOAD, ws->d_scratch, (int64_t)SLAB_SCRATCH, F.blocks);
        ICL_HIP(ctx, hipGetLastError());
    }
    if (F.ndense) {
        hipLaunchKernelGGL(jpeg_idct_dense_kernel, dim3((unsigned)icl_ceil_div(F.blocks, IDCT_THREADS)), dim3(IDCT_THREADS), 0, st, D.planes, F.npl,
                           (const int16_t *)ws->d_coef, (int64_t)SLAB_COEF, ws->d_scratch, (int64_t)SLAB_SCRATCH, F.blocks);
        ICL_HIP(ctx, hipGetLastError());
    }
    if (F.npng)
        ICL_TRY(icl_png_decode_slab(ctx, st, D.imgs, F.nimg, (const uint8_t *)ws->d_payload, (int64_t)SLAB_PAYLOAD, ws->d_scratch, (int64_t)SLAB_SCRATCH, ws->d_png_ok, png_stages));
    return ICL_OK;
}

// One stream result alone in slab 0, through the pipeline's own placement and launch code up to the planes (the test hooks): a
// KIND_PSTREAM by place_png, a JPEG by place_jpeg.  d_flag / h_flag: the check's flag that applies, downloaded into accepted; the slab is
// ws->host(0), the stream is synchronised.  `name` is what the messages call the image.
static int slab_of_one(icl_ctx *ctx, icl_ingest_ws *ws, const file_result &r, int png_stages, const int32_t *d_flag, int32_t *h_flag, const char *what, const char *name,
                       bool &accepted)
{
    ICL_HIP(ctx, hipEventSynchronize(ws->ev_up[0]));
    const slab_view S = ws->host(0);
    const bool png = r.kind == KIND_PSTREAM;
    slab_fill F;
    S.clear_row(0);
    if (!(png ? place_png(r, F, S) : place_jpeg(r, F, S))) return icl_fail(ctx, ICL_ERR_IO, "%s: inconsistent %s geometry for %s", what, png ? "PNG" : "JPEG", name);
    F.nimg = 1;
    int64_t upload = 0;
    ICL_TRY(run_slab_decode(ctx, ws, S, F, upload, png_stages));
    ICL_HIP(ctx, hipEventRecord(ws->ev_up[0], ctx->stream));
    ICL_HIP(ctx, hipMemcpyAsync(h_flag, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    accepted = h_flag[0] != 0;
    return ICL_OK;
}

struct file_fail {
    int64_t index;
    int rc;
    std::string err;
};

// The report of a call whose list has been processed: the code of the lowest failed file with "<what>: file <index> of <n>: <its reason>"
// as the context's message (lowest_out, may be NULL, then names that file), or ICL_OK.
static int report_lowest(icl_ctx *ctx, const std::vector<file_fail> &fails, int64_t n, const char *what, icl_item_failure *lowest_out)
{
    const file_fail *lowest = nullptr;
    for (const file_fail &f : fails)
        if (!lowest || f.index < lowest->index) lowest = &f;
    if (!lowest) return ICL_OK;
    if (lowest_out) *lowest_out = icl_item_failure{lowest->index, lowest->rc, lowest->err};
    return icl_fail(ctx, lowest->rc, "%s: file %lld of %lld: %s", what, (long long)lowest->index, (long long)n, lowest->err.c_str());
}

// worker threads of a call over n items: the caller's figure, else up to 16 of the machine's; never more than items, at least one
static int worker_count(int64_t n, int32_t threads)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    return (int)std::max<int64_t>(1, std::min<int64_t>(n, threads > 0 ? threads : (int)std::min(16u, hw)));
}

// The produce function of a call's feed (pass it as std::ref): item(i, state, result) on a worker thread, with the thread's own
// worker_state, kept from item to item, and a fresh result (nullptr where either cannot be allocated: the feed stops).  decode_ns sums
// the threads' time in item(); it is complete once the feed has joined its workers.
template <class R> struct feed_worker {
    std::function<void(int64_t, worker_state &, R &)> item;
    std::atomic<int64_t> decode_ns{0};
    std::unique_ptr<R> operator()(int64_t i)
    {
        thread_local std::unique_ptr<worker_state> wst(new (std::nothrow) worker_state());
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<R> r(wst ? new (std::nothrow) R() : nullptr);
        if (r) item(i, *wst, *r);
        decode_ns += (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        return r;
    }
};

struct ingest_job { // the list a pass works on, and its caller
    const ingest_src *srcs;
    int64_t n;
    int32_t threads;
    int32_t *status; // may be NULL
    const char *what;
};

struct pass_result {
    std::vector<file_fail> fails;     // per-file failures (also in status[])
    std::vector<int64_t> rejected;    // rows whose GPU entropy decode was not accepted: to be redone by a pass with ICL_ENTROPY_HOST
    std::vector<int64_t> stream_rows; // the row of every stream image of the pass, in the order of h_accepted
    std::vector<int64_t> png_rejected; // rows whose GPU PNG decode was not accepted: to be redone by a pass with ICL_PNG_HOST
    std::vector<int64_t> png_rows;     // the row of every PNG stream of the pass (its flag: h_png_ok[row])
};

struct slab_rows { // what slab_collect leaves the stages behind it
    int64_t first = 0; // the list's row of the slab's first image
    slab_fill F;
    std::vector<int32_t> failed; // slab rows of the failed files
};

using file_feed = ingest_feed<file_result>;

// the workspace, the entropy decoder's buffers where the pass decodes on the GPU, the slab's embedding rows where the sink is on the host
static int ingest_buffers(icl_ctx *ctx, const ingest_sink &sink, int entropy, int64_t n, icl_ingest_ws *&ws)
{
    ICL_TRY(ingest_ws(ctx, ws));
    if (entropy == ICL_ENTROPY_GPU) ICL_TRY(entropy_ws(ctx, ws, n));
    if (sink.embeds()) ICL_TRY(ws->emb.ensure(ctx, (size_t)SLAB_IMAGES * sink.head * 4, "file ingest: embedding buffer"));
    return ICL_OK;
}

// Rows from the feed, in file order, into the pinned slab S until it is full or the list ends: status, failures, totals, stream rows.
static int slab_collect(icl_ctx *ctx, const ingest_job &job, file_feed &feed, const slab_view &S, slab_rows &R, pass_result &res, ingest_totals &tot)
{
    R.first = feed.taken();
    R.F = slab_fill();
    R.failed.clear();
    slab_fill &F = R.F;
    while (feed.taken() < job.n && F.nimg < SLAB_IMAGES) {
        const file_result *next = feed.peek();
        if (!next) return icl_fail(ctx, ICL_ERR_NOMEM, "%s: out of host memory", job.what);
        if (F.nimg > 0 && !F.fits(*next)) break;
        const std::unique_ptr<file_result> r = feed.take();
        const int64_t row = R.first + F.nimg;
        ingest_image &D = S.imgs[F.nimg];
        S.clear_row(F.nimg);
        D.kind = r->kind;
        if (job.status) job.status[row] = r->rc;
        if (r->kind == KIND_FAILED) {
            R.failed.push_back(F.nimg);
            res.fails.push_back(file_fail{row, r->rc ? r->rc : ICL_ERR_IO, r->err});
        } else if (r->kind == KIND_HOST) {
            D.host_off = F.used;
            memcpy(S.payload + F.used, r->packed.data(), (size_t)ICL_IMG_BYTES);
            F.used += align16(ICL_IMG_BYTES);
            ++tot.host_files;
        } else if (r->kind == KIND_PSTREAM) {
            if (!place_png(*r, F, S)) {
                char nbuf[96];
                return icl_fail(ctx, ICL_ERR_IO, "%s: inconsistent PNG geometry for %s", job.what, ingest_src_name(job.srcs[row], nbuf, sizeof nbuf));
            }
            ++tot.gpu_pngs;
            res.png_rows.push_back(row);
            tot.png_bytes += (int64_t)r->packed.size() - (int64_t)sizeof(icl_png_desc);
        } else {
            if (!place_jpeg(*r, F, S)) {
                char nbuf[96];
                return icl_fail(ctx, ICL_ERR_IO, "%s: inconsistent JPEG geometry for %s", job.what, ingest_src_name(job.srcs[row], nbuf, sizeof nbuf));
            }
            ++tot.gpu_jpegs;
            if (r->kind == KIND_JSTREAM) {
                res.stream_rows.push_back(row);
                tot.stream_bytes += (int64_t)r->scan.nsub * (ICL_JE_SUB_BITS / 8);
            }
        }
        if (r->host_entropy) ++tot.host_entropy; // (whatever became of it: stage A ran, or tried to)
        if (r->host_png) ++tot.host_pngs;        // (likewise)
        ++F.nimg;
    }
    return ICL_OK;
}

// The decoded slab into the sink: gather / resize to u8 rows, and for an embedding sink the forward pass, NaN in the rows of the failed
// files, and the download of a host sink's rows.
static int slab_deliver(icl_ctx *ctx, icl_ingest_ws *ws, const ingest_sink &sink, const slab_rows &R)
{
    hipStream_t st = ctx->stream;
    const int nimg = R.F.nimg, head = sink.head;
    uint8_t *d_img = sink.embeds() ? ws->d_img : (uint8_t *)sink.row(R.first);
    hipLaunchKernelGGL(jpeg_gather_resize_kernel, dim3((unsigned)icl_ceil_div(OUTW * OUTH, 256), (unsigned)nimg), dim3(256), 0, st, ws->dev().imgs,
                       (const uint8_t *)ws->d_payload, (int64_t)SLAB_PAYLOAD, (const uint8_t *)ws->d_scratch, (int64_t)SLAB_SCRATCH, d_img);
    ICL_HIP(ctx, hipGetLastError());
    if (!sink.embeds()) return ICL_OK;
    float *d_dst = sink.kind == ingest_sink::EMB_DEV ? (float *)sink.row(R.first) : ws->emb.as<float>();
    ICL_TRY(icl_embed_dev_locked(ctx, ws->d_img, nimg, head, sink.prec, d_dst)); // (ends with the stream synchronised)
    if (sink.kind == ingest_sink::EMB_HOST) {
        float *out = (float *)sink.row(R.first);
        ICL_HIP(ctx, hipMemcpyAsync(out, ws->emb.p, (size_t)nimg * head * 4, hipMemcpyDeviceToHost, st));
        ICL_HIP(ctx, hipStreamSynchronize(st));
        for (int32_t j : R.failed) std::fill(out + (int64_t)j * head, out + (int64_t)(j + 1) * head, std::nanf(""));
    } else if (!R.failed.empty()) {
        ICL_HIP(ctx, hipMemcpyAsync(ws->d_rows, R.failed.data(), R.failed.size() * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(fill_nan_rows_kernel, dim3((unsigned)icl_ceil_div(head, 256), (unsigned)R.failed.size()), dim3(256), 0, st, d_dst,
                           (const int32_t *)ws->d_rows, (int)R.failed.size(), head);
        ICL_HIP(ctx, hipGetLastError());
        ICL_HIP(ctx, hipStreamSynchronize(st)); // R.failed is reused by the next slab
    }
    return ICL_OK;
}

// the accepted flags of the pass's stream images (downloaded slab by slab; read after the pass's last synchronisation)
static void tally_accepted(const icl_ingest_ws *ws, pass_result &res, ingest_totals &tot)
{
    for (size_t q = 0; q < res.stream_rows.size(); ++q) {
        if (ws->h_accepted[q]) ++tot.gpu_entropy;
        else res.rejected.push_back(res.stream_rows[q]);
    }
    for (int64_t row : res.png_rows)
        if (!ws->h_png_ok[row]) res.png_rejected.push_back(row);
}

// One pass of the pipeline over job's files into sink: worker threads decode the files (at most two slabs' worth of rows and payload
// bytes ahead), this thread builds the slabs in file order, double-buffered in pinned memory, with everything on ctx->stream.
static int ingest_pass(icl_ctx *ctx, const ingest_job &job, const ingest_sink &sink, const ingest_modes &modes, pass_result &res, ingest_totals &tot)
{
    icl_ingest_ws *ws = nullptr;
    ICL_TRY(ingest_buffers(ctx, sink, modes.entropy, job.n, ws));
    feed_worker<file_result> work{[&](int64_t i, worker_state &wst, file_result &r) { process_file(job.srcs[i], wst, modes, r); }};
    {
        file_feed feed(job.n, worker_count(job.n, job.threads), 2 * SLAB_IMAGES, 2 * SLAB_PAYLOAD, std::ref(work),
                       [](const file_result &r) { return (int64_t)r.packed.size(); });
        slab_rows R;
        for (int64_t k = 0; feed.taken() < job.n; ++k) {
            const int q = (int)(k & 1);
            ICL_HIP(ctx, hipEventSynchronize(ws->ev_up[q])); // the upload that last read this slab has finished
            const slab_view S = ws->host(q);
            ICL_TRY(slab_collect(ctx, job, feed, S, R, res, tot));
            if (R.F.npng) ICL_TRY(png_ws(ctx, ws, job.n)); // (the first slab of the call that holds a PNG stream)
            ICL_TRY(run_slab_decode(ctx, ws, S, R.F, tot.upload));
            ICL_HIP(ctx, hipEventRecord(ws->ev_up[q], ctx->stream));
            if (R.F.npng) // one flag per row of the slab, kept under the row's place in the list
                ICL_HIP(ctx, hipMemcpyAsync(ws->h_png_ok + R.first, ws->d_png_ok, (size_t)R.F.nimg * 4, hipMemcpyDeviceToHost, ctx->stream));
            if (R.F.nscan) // the flags are read after the pass's last synchronisation
                ICL_HIP(ctx, hipMemcpyAsync(ws->h_accepted + (res.stream_rows.size() - (size_t)R.F.nscan), ws->d_accepted, (size_t)R.F.nscan * 4, hipMemcpyDeviceToHost,
                                            ctx->stream));
            ICL_TRY(slab_deliver(ctx, ws, sink, R));
        }
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } // (the feed has joined its workers: decode_ns is complete)
    tot.decode_ns += work.decode_ns.load();
    tally_accepted(ws, res, tot);
    return ICL_OK;
}

} // namespace

// The pipeline (declared in icl_common.h): one pass in the context's entropy and PNG modes; the images the GPU entropy check or the GPU PNG
// check rejected are then redone by a pass with both modes on the host over those sources alone (a memory source is read again from the caller's buffer) into a sink of the same kind on a temporary (rows do not depend on
// the batch they are rebuilt or embedded in), which also produces their status codes and messages.
int ingest_files(icl_ctx *ctx, const ingest_src *srcs, int64_t n, int32_t threads, const ingest_sink &sink, int32_t *status, const char *what,
                 icl_item_failure *lowest_out)
{
    pass_result res;
    ingest_totals tot;
    ICL_TRY(ingest_pass(ctx, ingest_job{srcs, n, threads, status, what}, sink, ingest_modes{ctx->entropy_mode, ctx->png_mode}, res, tot));
    const int64_t nrej_jpeg = (int64_t)res.rejected.size(), nrej_png = (int64_t)res.png_rejected.size(), nrej = nrej_jpeg + nrej_png;
    res.rejected.insert(res.rejected.end(), res.png_rejected.begin(), res.png_rejected.end()); // (JPEGs first, then PNGs)
    if (nrej) {
        std::vector<ingest_src> rp((size_t)nrej); // (each keeps its index in the caller's list: messages name it)
        for (int64_t q = 0; q < nrej; ++q) rp[(size_t)q] = srcs[res.rejected[(size_t)q]];
        std::vector<int32_t> rstatus((size_t)nrej, 0);
        pass_result rres;
        std::vector<float> h_tmp;
        dev_guard d_tmp;
        ingest_sink tmp = sink;
        if (sink.kind == ingest_sink::EMB_HOST) {
            h_tmp.resize((size_t)nrej * sink.head);
            tmp.dst = h_tmp.data();
        } else {
            ICL_TRY(icl_dev_alloc(ctx, d_tmp, (size_t)nrej * sink.row_bytes(), "%s: device buffer of the repair pass", what));
            tmp.dst = d_tmp.p;
        }
        ICL_TRY(ingest_pass(ctx, ingest_job{rp.data(), nrej, threads, rstatus.data(), what}, tmp, MODES_HOST, rres, tot));
        for (int64_t q = 0; q < nrej; ++q) {
            const int64_t row = res.rejected[(size_t)q];
            if (status) status[row] = rstatus[(size_t)q];
            if (sink.kind == ingest_sink::EMB_HOST) memcpy(sink.row(row), tmp.row(q), sink.row_bytes());
            else ICL_HIP(ctx, hipMemcpyAsync(sink.row(row), tmp.row(q), sink.row_bytes(), hipMemcpyDeviceToDevice, ctx->stream));
        }
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (file_fail &f : rres.fails) res.fails.push_back(file_fail{res.rejected[(size_t)f.index], f.rc, f.err});
        tot.gpu_jpegs -= nrej_jpeg;    // (the first pass counted them; the repair pass counts what became of them)
        tot.host_entropy -= nrej_jpeg; // they are reported as redone, not as routed to the host
        tot.gpu_pngs -= nrej_png;      // (the PNG rejections likewise: the repair pass counts them among host_files)
        tot.host_pngs -= nrej_png;
    }
    tot.redone_jpegs = nrej_jpeg;
    tot.redone_pngs = nrej_png;
    ctx->ingest_last = tot;
    return report_lowest(ctx, res.fails, n, what, lowest_out);
}

static int load_images_224_dev(icl_ctx *ctx, const ingest_list &imgs, int32_t threads, uint8_t *d_out, int32_t *status, const char *what)
{
    const int64_t n = imgs.n, bad = imgs.first_bad();
    if (!ctx || bad == ingest_list::NO_ARRAYS || (n && !d_out) || threads < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return no_throw(ctx, what, [&]() -> int {
        icl_ingest_stats_reset(ctx);
        if (n == 0) return ICL_OK;
        const std::vector<ingest_src> srcs = imgs.srcs();
        return ingest_files(ctx, srcs.data(), n, threads, ingest_sink{ingest_sink::U8_DEV, d_out, 0, 0}, status, what);
    });
}

extern "C" int icl_load_images_224_dev(icl_ctx *ctx, const char *const *paths, int64_t n, int32_t threads, uint8_t *d_out, int32_t *status)
{
    return load_images_224_dev(ctx, ingest_list::files(paths, n), threads, d_out, status, "icl_load_images_224_dev");
}

extern "C" int icl_load_images_224_mem_dev(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int32_t threads, uint8_t *d_out, int32_t *status)
{
    return load_images_224_dev(ctx, ingest_list::memory(data, bytes, n), threads, d_out, status, "icl_load_images_224_mem_dev");
}

static int embed_files(icl_ctx *ctx, const ingest_list &imgs, int head, int prec, int32_t threads, float *out, int32_t *status, bool dev, const char *what)
{
    const int64_t n = imgs.n, bad = imgs.first_bad();
    if (!ctx || bad == ingest_list::NO_ARRAYS || (n && !out) || threads < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    if (head != ICL_HEAD_POOLED && head != ICL_HEAD_DENSE0) return icl_fail(ctx, ICL_ERR_ARG, "head must be 2048 or 1000");
    if (prec != ICL_PREC_FP32 && prec != ICL_PREC_BF16 && prec != ICL_PREC_BF16X3)
        return icl_fail(ctx, ICL_ERR_ARG, "prec must be ICL_PREC_FP32, ICL_PREC_BF16 or ICL_PREC_BF16X3");
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    if (!ctx->model) return icl_fail(ctx, ICL_ERR_NOMODEL, "no model loaded (call icl_model_load_* first)");
    return no_throw(ctx, what, [&]() -> int {
        icl_ingest_stats_reset(ctx);
        if (n == 0) return ICL_OK;
        const std::vector<ingest_src> srcs = imgs.srcs();
        return ingest_files(ctx, srcs.data(), n, threads, ingest_sink{dev ? ingest_sink::EMB_DEV : ingest_sink::EMB_HOST, out, head, prec}, status, what);
    });
}

extern "C" int icl_embed_files(icl_ctx *ctx, const char *const *paths, int64_t n, int head, int prec, int32_t threads, float *out, int32_t *status)
{
    return embed_files(ctx, ingest_list::files(paths, n), head, prec, threads, out, status, false, "icl_embed_files");
}

extern "C" int icl_embed_files_dev(icl_ctx *ctx, const char *const *paths, int64_t n, int head, int prec, int32_t threads, float *d_out, int32_t *status)
{
    return embed_files(ctx, ingest_list::files(paths, n), head, prec, threads, d_out, status, true, "icl_embed_files_dev");
}

extern "C" int icl_embed_images_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int head, int prec, int32_t threads, float *out,
                                    int32_t *status)
{
    return embed_files(ctx, ingest_list::memory(data, bytes, n), head, prec, threads, out, status, false, "icl_embed_images_mem");
}

extern "C" int icl_embed_images_mem_dev(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int head, int prec, int32_t threads, float *d_out,
                                        int32_t *status)
{
    return embed_files(ctx, ingest_list::memory(data, bytes, n), head, prec, threads, d_out, status, true, "icl_embed_images_mem_dev");
}

extern "C" int icl_last_ingest_stats(icl_ctx *ctx, int64_t *gpu_jpegs, int64_t *host_files, int64_t *upload_bytes, double *host_decode_s)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (gpu_jpegs) *gpu_jpegs = ctx->ingest_last.gpu_jpegs;
    if (host_files) *host_files = ctx->ingest_last.host_files;
    if (upload_bytes) *upload_bytes = ctx->ingest_last.upload;
    if (host_decode_s) *host_decode_s = (double)ctx->ingest_last.decode_ns * 1e-9;
    return ICL_OK;
}

extern "C" int icl_set_ingest_options(icl_ctx *ctx, int entropy_mode)
{
    if (!ctx || (entropy_mode != ICL_ENTROPY_HOST && entropy_mode != ICL_ENTROPY_GPU))
        return icl_fail(ctx, ICL_ERR_ARG, "icl_set_ingest_options: entropy_mode must be ICL_ENTROPY_HOST or ICL_ENTROPY_GPU");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->entropy_mode = entropy_mode;
    return ICL_OK;
}

extern "C" int icl_last_entropy_stats(icl_ctx *ctx, int64_t *gpu_entropy_jpegs, int64_t *host_entropy_jpegs, int64_t *redone_on_host, int64_t *stream_bytes)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (gpu_entropy_jpegs) *gpu_entropy_jpegs = ctx->ingest_last.gpu_entropy;
    if (host_entropy_jpegs) *host_entropy_jpegs = ctx->ingest_last.host_entropy;
    if (redone_on_host) *redone_on_host = ctx->ingest_last.redone_jpegs;
    if (stream_bytes) *stream_bytes = ctx->ingest_last.stream_bytes;
    return ICL_OK;
}

extern "C" int icl_set_png_options(icl_ctx *ctx, int png_mode)
{
    if (!ctx || (png_mode != ICL_PNG_HOST && png_mode != ICL_PNG_GPU)) return icl_fail(ctx, ICL_ERR_ARG, "icl_set_png_options: png_mode must be ICL_PNG_HOST or ICL_PNG_GPU");
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->png_mode = png_mode;
    return ICL_OK;
}

extern "C" int icl_last_png_stats(icl_ctx *ctx, int64_t *gpu_pngs, int64_t *host_pngs, int64_t *redone_on_host, int64_t *stream_bytes)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (gpu_pngs) *gpu_pngs = ctx->ingest_last.gpu_pngs;
    if (host_pngs) *host_pngs = ctx->ingest_last.host_pngs;
    if (redone_on_host) *redone_on_host = ctx->ingest_last.redone_pngs;
    if (stream_bytes) *stream_bytes = ctx->ingest_last.png_bytes;
    return ICL_OK;
}

// Test hook: each file's scanlines as the GPU route leaves them -- inflated (stage 0) or unfiltered (stage 1) -- one single-image slab per
// file through the pipeline's own placement and launch code.
extern "C" int icl_png_raw_files(icl_ctx *ctx, const char *const *paths, int64_t n, int stage, uint8_t *raw, int64_t cap, int64_t *offsets, int32_t *state)
{
    const char *what = "icl_png_raw_files";
    const ingest_list imgs = ingest_list::files(paths, n);
    const int64_t bad = imgs.first_bad();
    if (!ctx || bad == ingest_list::NO_ARRAYS || !offsets || !state || cap < 0 || (stage != 0 && stage != 1)) return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return no_throw(ctx, what, [&]() -> int {
        const std::vector<ingest_src> srcs = imgs.srcs();
        icl_ingest_ws *ws = nullptr;
        std::unique_ptr<worker_state> wst(new worker_state());
        int64_t at = 0;
        for (int64_t i = 0; i < n; ++i) {
            offsets[i] = at;
            state[i] = -1;
            file_result r;
            process_file(srcs[i], *wst, ingest_modes{ICL_ENTROPY_HOST, ICL_PNG_GPU}, r);
            if (r.kind != KIND_PSTREAM) continue; // does not qualify (or cannot be read at all)
            state[i] = 0;
            const int64_t total = r.plane_bytes;
            if (raw) {
                if (at + total > cap) return icl_fail(ctx, ICL_ERR_ARG, "%s: buffer too small", what);
                ICL_TRY(ingest_ws(ctx, ws));
                ICL_TRY(png_ws(ctx, ws, 1));
                bool ok = false;
                ICL_TRY(slab_of_one(ctx, ws, r, stage == 0 ? 1 : 2, ws->d_png_ok, ws->h_png_ok, what, paths[i], ok));
                state[i] = ok ? 1 : 0;
                if (ok) ICL_HIP(ctx, hipMemcpy(raw + at, ws->d_scratch + ws->host(0).imgs[0].yplane, (size_t)total, hipMemcpyDeviceToHost));
            }
            at += total; // (a rejected file keeps its range; its contents are not written)
        }
        offsets[n] = at;
        return ICL_OK;
    });
}

// the body of icl_jpeg_coefs_files / _mem
static int jpeg_coefs(icl_ctx *ctx, const ingest_list &imgs, int entropy_mode, int16_t *coefs, int64_t cap, int64_t *offsets, int32_t *state, const char *what)
{
    const int64_t n = imgs.n, bad = imgs.first_bad();
    if (!ctx || bad == ingest_list::NO_ARRAYS || !offsets || !state || cap < 0 || (entropy_mode != ICL_ENTROPY_HOST && entropy_mode != ICL_ENTROPY_GPU))
        return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return no_throw(ctx, what, [&]() -> int {
        const std::vector<ingest_src> srcs = imgs.srcs();
        icl_ingest_ws *ws = nullptr;
        if (entropy_mode == ICL_ENTROPY_GPU) {
            ICL_TRY(ingest_ws(ctx, ws));
            ICL_TRY(entropy_ws(ctx, ws, 1));
        }
        std::unique_ptr<worker_state> wst(new worker_state());
        int64_t at = 0;
        for (int64_t i = 0; i < n; ++i) {
            offsets[i] = at;
            state[i] = -1;
            char nbuf[96];
            const char *name = ingest_src_name(srcs[i], nbuf, sizeof nbuf);
            if (entropy_mode == ICL_ENTROPY_HOST) {
                std::vector<uint8_t> file;
                const uint8_t *jd;
                size_t jn;
                if (icl_image_src_read(srcs[i], file, jd, jn) != ICL_IMAGE_JPEG) return icl_fail(ctx, ICL_ERR_IO, "%s: %s is not a readable JPEG", what, name);
                const int rc = icl_jpeg_stage_a(nullptr, jd, jn, name, wst->J);
                if (rc) return icl_fail(ctx, rc, "%s: %s", what, icl_last_error(nullptr));
                state[i] = 1;
                for (int c = 0; c < wst->J.ncomp; ++c) {
                    const std::vector<int16_t> &cf = wst->J.comp[c].coefs;
                    if (coefs) {
                        if (at + (int64_t)cf.size() > cap) return icl_fail(ctx, ICL_ERR_ARG, "%s: buffer too small", what);
                        memcpy(coefs + at, cf.data(), cf.size() * 2);
                    }
                    at += (int64_t)cf.size();
                }
                continue;
            }
            file_result r;
            process_file(srcs[i], *wst, ingest_modes{ICL_ENTROPY_GPU, ICL_PNG_HOST}, r);
            if (r.kind != KIND_JSTREAM) continue; // does not qualify (or cannot be read at all)
            int64_t total = 0;
            for (int c = 0; c < r.ncomp; ++c) total += (int64_t)r.cm[c].wblocks * r.cm[c].hblocks * 64;
            state[i] = 0;
            if (coefs) {
                if (at + total > cap) return icl_fail(ctx, ICL_ERR_ARG, "%s: buffer too small", what);
                bool ok = false;
                ICL_TRY(slab_of_one(ctx, ws, r, 2, ws->d_accepted, ws->h_accepted, what, name, ok));
                state[i] = ok ? 1 : 0;
                int64_t o = at;
                for (int c = 0; c < r.ncomp && ok; ++c) {
                    const int64_t ne = (int64_t)r.cm[c].wblocks * r.cm[c].hblocks * 64;
                    ICL_HIP(ctx, hipMemcpy(coefs + o, ws->d_coef + ws->host(0).scans[0].coef_off[c], (size_t)ne * 2, hipMemcpyDeviceToHost));
                    o += ne;
                }
            }
            at += total; // (a rejected file keeps its range; its contents are not written)
        }
        offsets[n] = at;
        return ICL_OK;
    });
}

// Test hook: the quantised coefficients of each file as stage A leaves them, by host stage A or by the GPU entropy decoder (one
// single-image slab per file through the pipeline's own placement and launch code).
extern "C" int icl_jpeg_coefs_files(icl_ctx *ctx, const char *const *paths, int64_t n, int entropy_mode, int16_t *coefs, int64_t cap, int64_t *offsets, int32_t *state)
{
    return jpeg_coefs(ctx, ingest_list::files(paths, n), entropy_mode, coefs, cap, offsets, state, "icl_jpeg_coefs_files");
}

extern "C" int icl_jpeg_coefs_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int entropy_mode, int16_t *coefs, int64_t cap,
                                  int64_t *offsets, int32_t *state)
{
    return jpeg_coefs(ctx, ingest_list::memory(data, bytes, n), entropy_mode, coefs, cap, offsets, state, "icl_jpeg_coefs_mem");
}

// ---- the batched downsizer: resizeImageIfNeeded (rekognition.go:173-259) over a list, icl_downsize_images[_mem] ------------------------
// Per image a worker thread measures the bytes (at or under the limit: passed through), and otherwise does what process_file does for the
// ingest calls; the slab's JPEGs go through run_slab_decode to their planes, jpeg_gather_resize_var_kernel takes planes to RGB at each
// image's own new size, host-decoded images arrive as resized RGB, and the encoder (jpeg_encode_gpu.hip) codes the slab's RGB.  The coded
// sizes come back once per slab; images still above the limit get a second pass at half the size from the planes still held.
namespace {

struct dz_image { // one image of the variable-size gather
    int32_t img;       // its ingest_image in the slab
    int32_t nw, nh, area;
    int64_t rgb_off;   // where its RGB goes in the RGB scratch
    int64_t tab_off;   // its tables in the table buffer: int32 xofs[nw], yofs[nh], then int16 xa[2 nw], ya[2 nh]
};

// jpeg_gather_resize_kernel for an output size of the image's own: one thread per output pixel, tables from the table buffer
__global__ void __launch_bounds__(256) jpeg_gather_resize_var_kernel(const ingest_image *__restrict__ imgs, const dz_image *__restrict__ dz, const uint8_t *__restrict__ tabs,
                                                                     int64_t tab_bytes, const uint8_t *__restrict__ scratch, uint8_t *__restrict__ rgb, int64_t rgb_bytes)
{
    const dz_image &Z = dz[blockIdx.y];
    const ingest_image &D = imgs[Z.img];
    const int64_t npx = (int64_t)Z.nw * Z.nh;
    if (D.kind != KIND_JPEG || Z.rgb_off < 0 || Z.rgb_off + npx * 3 > rgb_bytes || Z.tab_off < 0 || Z.tab_off + ((int64_t)Z.nw + Z.nh) * 8 > tab_bytes) return;
    const int32_t *xofs = (const int32_t *)(tabs + Z.tab_off), *yofs = xofs + Z.nw;
    const int16_t *xa = (const int16_t *)(yofs + Z.nh), *ya = xa + 2 * Z.nw;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npx; p += (int64_t)gridDim.x * 256) {
        const int dy = (int)(p / Z.nw), dx = (int)(p - (int64_t)dy * Z.nw);
        uint8_t *o = rgb + Z.rgb_off + p * 3;
        int r[4], g[4], b[4];
        if (Z.area) {
            rgb_at(D, scratch, 2 * dx, 2 * dy, r[0], g[0], b[0]);
            rgb_at(D, scratch, 2 * dx + 1, 2 * dy, r[1], g[1], b[1]);
            rgb_at(D, scratch, 2 * dx, 2 * dy + 1, r[2], g[2], b[2]);
            rgb_at(D, scratch, 2 * dx + 1, 2 * dy + 1, r[3], g[3], b[3]);
            o[0] = icl_area_mean(r[0], r[1], r[2], r[3]);
            o[1] = icl_area_mean(g[0], g[1], g[2], g[3]);
            o[2] = icl_area_mean(b[0], b[1], b[2], b[3]);
            continue;
        }
        const int sx = min(max(xofs[dx], 0), D.ow - 1), sx1 = min(sx + 1, D.ow - 1);
        const int sy = min(max(yofs[dy], 0), D.oh - 1), sy1 = min(sy + 1, D.oh - 1);
        rgb_at(D, scratch, sx, sy, r[0], g[0], b[0]);
        rgb_at(D, scratch, sx1, sy, r[1], g[1], b[1]);
        rgb_at(D, scratch, sx, sy1, r[2], g[2], b[2]);
        rgb_at(D, scratch, sx1, sy1, r[3], g[3], b[3]);
        const int a0 = xa[dx * 2], a1 = xa[dx * 2 + 1], b0 = ya[dy * 2], b1 = ya[dy * 2 + 1];
        o[0] = icl_resize_linear(r[0], r[1], r[2], r[3], a0, a1, b0, b1);
        o[1] = icl_resize_linear(g[0], g[1], g[2], g[3], a0, a1, b0, b1);
        o[2] = icl_resize_linear(b[0], b[1], b[2], b[3], a0, a1, b0, b1);
    }
}

constexpr int64_t DZ_RGB_BUDGET = 1ll << 30; // resized RGB of one slab on the device
enum { DZ_PASS = 0, DZ_FAILED, DZ_GPU, DZ_HOST, DZ_DONE };

struct dz_result { // what a worker hands the slab builder for one image
    int type = DZ_FAILED;
    file_result fr;             // DZ_GPU: as for the ingest calls; DZ_HOST: fr.packed is the resized RGB; DZ_FAILED: rc, err
    std::vector<uint8_t> bytes; // DZ_PASS of a file (a memory source is copied from the caller's buffer); DZ_DONE: the finished file
    std::vector<uint8_t> orig;  // DZ_HOST: the decoded image, for a second attempt
    int ow = 0, oh = 0, nw = 0, nh = 0;
    int attempts = 0; // DZ_DONE
    int64_t in_bytes = 0;
    int64_t held() const { return (int64_t)(fr.packed.size() + bytes.size() + orig.size()); }
};

static void dz_process(const ingest_src &src, worker_state &ws, int entropy, int64_t max_bytes, int max_dim, dz_result &z)
{
    char nbuf[96];
    const char *name = ingest_src_name(src, nbuf, sizeof nbuf);
    file_result &r = z.fr;
    auto fail = [&](int rc) {
        z.type = DZ_FAILED;
        fail_from_tls(r, rc);
    };
    const bool done = decoder_guard(r, name, [&]() {
        const uint8_t *data = nullptr;
        size_t len = 0;
        const int rc = icl_src_bytes(src, name, z.bytes, data, len);
        if (rc) return fail(rc);
        z.in_bytes = (int64_t)len;
        if ((int64_t)len <= max_bytes) {
            z.type = DZ_PASS;
            return;
        }
        const ingest_src mem{nullptr, data, (int64_t)len, src.index};
        // what cannot go through a slab is done here, start to end, by the host call
        auto whole_on_host = [&]() {
            int32_t info[6];
            std::vector<uint8_t> out;
            const int rc2 = icl_downsize_src(src, max_bytes, max_dim, out, info);
            if (rc2) return fail(rc2);
            z.bytes.swap(out);
            z.attempts = info[5];
            z.type = DZ_DONE;
        };
        auto too_large = [&](int nw, int nh) { return (int64_t)nw * nh * 3 > SLAB_PAYLOAD / 4 || icl_jenc_blocks(nw, nh) > icl_jenc_max_batch_blocks() / 4; };
        bool oversize = false;
        process_file_with(mem, name, ws, ingest_modes{entropy, ICL_PNG_HOST}, r, [&](std::vector<uint8_t> &rgb, int w, int h) {
            if (icl_downsize_dims_checked(name, w, h, max_dim, z.nw, z.nh)) return false;
            if (too_large(z.nw, z.nh)) {
                oversize = true;
                return true;
            }
            z.ow = w;
            z.oh = h;
            r.packed.resize((size_t)z.nw * z.nh * 3);
            icl_resize_bilinear_u8(rgb.data(), w, h, r.packed.data(), z.nw, z.nh);
            z.orig.swap(rgb);
            return true;
        });
        if (r.kind == KIND_FAILED) {
            z.type = DZ_FAILED;
            return;
        }
        if (oversize) return whole_on_host();
        if (r.kind == KIND_HOST) {
            z.type = DZ_HOST;
            z.bytes.clear();
            z.bytes.shrink_to_fit();
            return;
        }
        const bool swap = icl_exif_swaps_axes(r.orient);
        z.ow = swap ? r.H : r.W;
        z.oh = swap ? r.W : r.H;
        if (icl_downsize_dims_checked(name, z.ow, z.oh, max_dim, z.nw, z.nh)) return fail(ICL_ERR_ARG);
        if (too_large(z.nw, z.nh)) return whole_on_host();
        z.type = DZ_GPU;
        z.bytes.clear();
        z.bytes.shrink_to_fit();
    });
    if (!done) z.type = DZ_FAILED;
}

struct dz_entry { // one image of a slab, in list order
    int64_t row;
    std::unique_ptr<dz_result> z;
    int img = -1, scan = -1; // DZ_GPU: its ingest_image; its place among the slab's stream images (-1: entropy-decoded on the host)
    int slot[2] = {-1, -1};  // its file in the first / second encoder batch
};

struct dz_ws { // device buffers of the call: grown from slab to slab, released when it ends
    icl_dev_grow dz, tabs, rgb;
    ~dz_ws()
    {
        for (icl_dev_grow *b : {&dz, &tabs, &rgb}) b->release();
    }
};

// One encoder batch over the entries `which` of a slab at attempt a (0: nw x nh, 1: half of it): gather / upload their RGB, encode, and
// bring the files to the host.  files / off: the batch's files; entry e's is slot[a].
static int dz_encode_pass(icl_ctx *ctx, icl_ingest_ws *ws, dz_ws &B, std::vector<dz_entry> &E, const std::vector<int> &which, int a, std::vector<uint8_t> &files,
                          std::vector<int64_t> &off)
{
    hipStream_t st = ctx->stream;
    std::vector<dz_image> dz;
    std::vector<uint8_t> tabs;
    std::vector<icl_jenc_item> items;
    std::vector<std::vector<uint8_t>> host_rgb; // second attempt of host-decoded images
    int64_t rgb_used = 0, max_px = 0;
    for (int e : which) {
        dz_entry &X = E[(size_t)e];
        const dz_result &z = *X.z;
        const int nw = a ? z.nw / 2 : z.nw, nh = a ? z.nh / 2 : z.nh;
        X.slot[a] = (int)items.size();
        items.push_back(icl_jenc_item{rgb_used, nw, nh});
        if (z.type == DZ_GPU) {
            dz_image Z;
            Z.img = X.img;
            Z.nw = nw;
            Z.nh = nh;
            Z.area = icl_resize_is_area(z.ow, z.oh, nw, nh) ? 1 : 0;
            Z.rgb_off = rgb_used;
            Z.tab_off = (int64_t)tabs.size();
            tabs.resize(tabs.size() + (size_t)align16(((int64_t)nw + nh) * 8));
            int32_t *xofs = (int32_t *)(tabs.data() + Z.tab_off), *yofs = xofs + nw;
            int16_t *xa = (int16_t *)(yofs + nh), *ya = xa + 2 * nw;
            icl_resize_coeffs(nw, z.ow, xofs, xa);
            icl_resize_coeffs(nh, z.oh, yofs, ya);
            dz.push_back(Z);
            max_px = std::max(max_px, (int64_t)nw * nh);
        }
        rgb_used += align16((int64_t)nw * nh * 3);
    }
    ICL_TRY(B.rgb.ensure(ctx, (size_t)std::max<int64_t>(rgb_used, 16), "downsize: RGB buffer"));
    size_t k = 0;
    for (int e : which) { // host-decoded images: their RGB as it stands
        const dz_result &z = *E[(size_t)e].z;
        const icl_jenc_item &it = items[k++];
        if (z.type != DZ_HOST) continue;
        const uint8_t *src = z.fr.packed.data();
        if (a) {
            host_rgb.emplace_back((size_t)it.w * it.h * 3);
            icl_resize_bilinear_u8(z.orig.data(), z.ow, z.oh, host_rgb.back().data(), it.w, it.h);
            src = host_rgb.back().data();
        }
        ICL_HIP(ctx, hipMemcpyAsync((uint8_t *)B.rgb.p + it.rgb_off, src, (size_t)it.w * it.h * 3, hipMemcpyHostToDevice, st));
    }
    if (!dz.empty()) {
        ICL_TRY(B.dz.ensure(ctx, dz.size() * sizeof(dz_image), "downsize: image table"));
        ICL_TRY(B.tabs.ensure(ctx, tabs.size(), "downsize: resize tables"));
        ICL_HIP(ctx, hipMemcpyAsync(B.dz.p, dz.data(), dz.size() * sizeof(dz_image), hipMemcpyHostToDevice, st));
        ICL_HIP(ctx, hipMemcpyAsync(B.tabs.p, tabs.data(), tabs.size(), hipMemcpyHostToDevice, st));
        const unsigned gx = (unsigned)std::min<int64_t>(icl_ceil_div(max_px, 256), 8192);
        hipLaunchKernelGGL(jpeg_gather_resize_var_kernel, dim3(gx, (unsigned)dz.size()), dim3(256), 0, st, (const ingest_image *)ws->dev().imgs, (const dz_image *)B.dz.p,
                           (const uint8_t *)B.tabs.p, (int64_t)tabs.size(), (const uint8_t *)ws->d_scratch, (uint8_t *)B.rgb.p, (int64_t)B.rgb.bytes);
        ICL_HIP(ctx, hipGetLastError());
    }
    ICL_HIP(ctx, hipStreamSynchronize(st)); // (the host vectors above go out of scope; the encoder synchronises anyway)
    const uint8_t *d_files = nullptr;
    ICL_TRY(icl_jenc_run(ctx, (const uint8_t *)B.rgb.p, items.data(), (int64_t)items.size(), ICL_DOWNSIZE_QUALITY, &d_files, off));
    files.resize((size_t)std::max<int64_t>(off.back(), 1));
    if (off.back()) ICL_HIP(ctx, hipMemcpy(files.data(), d_files, (size_t)off.back(), hipMemcpyDeviceToHost));
    return ICL_OK;
}

struct dz_job { // the list a downsize call works on, its limits, where its files go (back to back in out[cap], out_off[n + 1]), and its caller
    const ingest_src *srcs;
    int64_t n, max_bytes;
    int max_dim;
    uint8_t *out;
    int64_t cap, *out_off;
    int32_t *status; // may be NULL
    const char *what;
};

// One round of the downsizer: the images one slab, one RGB scratch and one encoder batch take, in list order, with the finished results
// that lie between them.
struct dz_round {
    std::vector<dz_entry> E;
    slab_fill F;
    int64_t rgb = 0, blocks = 0, coded = 0; // of the images to encode: resized RGB bytes, encoder blocks, their number
    int64_t finished = 0;                   // bytes of the finished results (passed-through files, whole-on-host outputs) waiting in E
    std::vector<uint8_t> files[2];          // the coded files of the first / second encoder batch, off[a][slot] .. off[a][slot + 1]
    std::vector<int64_t> off[2];
    void reset() { E.clear(), F = slab_fill(), rgb = blocks = coded = finished = 0; }
    static int64_t rgb_bytes(const dz_result &z) { return align16((int64_t)z.nw * z.nh * 3); }
    // Does z, next in the list, still belong to this round?  An image to encode needs room in the RGB scratch, the encoder's batch and
    // (a JPEG for the GPU) the slab; alone it always fits.  A finished result has left the feed's byte budget and waits in E for its turn:
    // the round ends once it holds 2 * SLAB_PAYLOAD of them, so a long run of small files is delivered as it goes.
    bool admits(const dz_result &z) const
    {
        if (z.type != DZ_GPU && z.type != DZ_HOST) return !(finished > 2 * SLAB_PAYLOAD && !E.empty());
        const bool room = rgb + rgb_bytes(z) <= DZ_RGB_BUDGET && blocks + icl_jenc_blocks(z.nw, z.nh) <= icl_jenc_max_batch_blocks() && coded < icl_jenc_max_batch_images() &&
                          (z.type == DZ_HOST || (F.nimg < SLAB_IMAGES && F.fits(z.fr)));
        return room || rgb == 0;
    }
    // whether the GPU entropy check took X's stream (an image entropy-decoded on the host has none)
    static bool accepted(const icl_ingest_ws *ws, const dz_entry &X) { return X.scan < 0 || ws->h_accepted[X.scan] != 0; }
};

// Images from the feed, in list order, into round R until dz_round::admits says it is full or the list ends; the JPEGs the GPU rebuilds
// are placed in the pinned slab S as they come (passed-through, host-decoded and failed images take no slab row).
static int dz_collect(icl_ctx *ctx, const dz_job &job, ingest_feed<dz_result> &feed, const slab_view &S, dz_round &R)
{
    R.reset();
    slab_fill &F = R.F;
    while (feed.taken() < job.n) {
        const dz_result *next = feed.peek();
        if (!next) return icl_fail(ctx, ICL_ERR_NOMEM, "%s: out of host memory", job.what);
        if (!R.admits(*next)) break;
        if (next->type == DZ_GPU || next->type == DZ_HOST) {
            R.rgb += dz_round::rgb_bytes(*next);
            R.blocks += icl_jenc_blocks(next->nw, next->nh);
            ++R.coded;
        } else {
            R.finished += (int64_t)next->bytes.size();
        }
        dz_entry X;
        X.row = feed.taken();
        X.z = feed.take();
        if (X.z->type == DZ_GPU) {
            S.clear_row(F.nimg);
            X.img = F.nimg;
            X.scan = X.z->fr.kind == KIND_JSTREAM ? F.nscan : -1;
            if (!place_jpeg(X.z->fr, F, S)) {
                char nbuf[96];
                return icl_fail(ctx, ICL_ERR_IO, "%s: inconsistent JPEG geometry for %s", job.what, ingest_src_name(job.srcs[X.row], nbuf, sizeof nbuf));
            }
            ++F.nimg;
        }
        R.E.push_back(std::move(X));
    }
    return ICL_OK;
}

// The round's slab to its planes (run_slab_decode; the accepted flags of its streams come back with the first encoder batch, which
// synchronises), every image to encode through the encoder at its new size, then those still above the limit, whose stream was accepted
// and that can still be halved, through it again at half that size from the planes still held.  ev_up: recorded behind the slab's upload.
static int dz_rebuild(icl_ctx *ctx, icl_ingest_ws *ws, dz_ws &B, const slab_view &S, hipEvent_t ev_up, int64_t max_bytes, dz_round &R)
{
    std::vector<int> first, second;
    for (size_t e = 0; e < R.E.size(); ++e)
        if (R.E[e].z->type == DZ_GPU || R.E[e].z->type == DZ_HOST) first.push_back((int)e);
    if (R.F.nimg) {
        int64_t upload = 0;
        ICL_TRY(run_slab_decode(ctx, ws, S, R.F, upload));
        ICL_HIP(ctx, hipEventRecord(ev_up, ctx->stream));
        if (R.F.nscan) ICL_HIP(ctx, hipMemcpyAsync(ws->h_accepted, ws->d_accepted, (size_t)R.F.nscan * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (!first.empty()) ICL_TRY(dz_encode_pass(ctx, ws, B, R.E, first, 0, R.files[0], R.off[0])); // (synchronises: h_accepted is there)
    for (int e : first) {
        const dz_entry &X = R.E[(size_t)e];
        const int64_t len = R.off[0][(size_t)X.slot[0] + 1] - R.off[0][(size_t)X.slot[0]];
        if (dz_round::accepted(ws, X) && len > max_bytes && X.z->nw / 2 >= 1 && X.z->nh / 2 >= 1) second.push_back(e);
    }
    if (!second.empty()) ICL_TRY(dz_encode_pass(ctx, ws, B, R.E, second, 1, R.files[1], R.off[1]));
    return ICL_OK;
}

// The round's results in list order into the caller's buffer: a passed-through source as it stands, a coded file from the batch of its
// last attempt, a finished file, nothing for a failed image.  An image whose stream the GPU entropy check rejected is redone here by the
// host call, which also reports what it finds.  Statuses, failures and the call's totals (tot.bytes_out is where the next file goes).
static void dz_deliver(const icl_ingest_ws *ws, const dz_job &job, dz_round &R, std::vector<file_fail> &fails, dz_totals &tot)
{
    auto deliver = [&](int64_t row, const uint8_t *p, int64_t len) {
        job.out_off[row] = tot.bytes_out;
        if (job.out && len && tot.bytes_out + len <= job.cap) memcpy(job.out + tot.bytes_out, p, (size_t)len);
        tot.bytes_out += len;
    };
    for (dz_entry &X : R.E) {
        dz_result &z = *X.z;
        tot.bytes_in += z.in_bytes;
        if (z.type == DZ_GPU && !dz_round::accepted(ws, X)) {
            int32_t info[6];
            const int rc = icl_downsize_src(job.srcs[X.row], job.max_bytes, job.max_dim, z.bytes, info);
            if (rc) {
                z.type = DZ_FAILED;
                fail_from_tls(z.fr, rc);
            } else {
                z.type = DZ_DONE;
                z.attempts = info[5];
            }
        }
        if (job.status) job.status[X.row] = z.type == DZ_FAILED ? (z.fr.rc ? z.fr.rc : ICL_ERR_IO) : ICL_OK;
        switch (z.type) {
        case DZ_PASS: {
            const ingest_src &s = job.srcs[X.row];
            deliver(X.row, s.path ? z.bytes.data() : s.data, z.in_bytes);
            ++tot.passthrough;
            break;
        }
        case DZ_DONE:
            deliver(X.row, z.bytes.data(), (int64_t)z.bytes.size());
            ++tot.host_decoded;
            tot.second_attempts += z.attempts == 2;
            break;
        case DZ_GPU:
        case DZ_HOST: {
            const int a = X.slot[1] >= 0 ? 1 : 0;
            const int64_t lo = R.off[a][(size_t)X.slot[a]], hi = R.off[a][(size_t)X.slot[a] + 1];
            deliver(X.row, R.files[a].data() + lo, hi - lo);
            (z.type == DZ_GPU ? tot.gpu_rebuilt : tot.host_decoded) += 1;
            tot.second_attempts += a;
            break;
        }
        default:
            deliver(X.row, nullptr, 0);
            fails.push_back(file_fail{X.row, z.fr.rc ? z.fr.rc : ICL_ERR_IO, z.fr.err});
            break;
        }
    }
}

// The downsizer's driver: worker threads run dz_process over the list (at most two slabs' worth of images and bytes ahead), this thread
// runs the rounds in list order, double-buffered in the pinned slabs, with everything on ctx->stream.
static int downsize_images_locked(icl_ctx *ctx, const dz_job &job, int32_t threads)
{
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    ctx->downsize_last = dz_totals();
    job.out_off[0] = 0;
    if (job.n == 0) return ICL_OK;
    const int entropy = ctx->entropy_mode;
    icl_ingest_ws *ws = nullptr;
    ICL_TRY(ingest_ws(ctx, ws));
    if (entropy == ICL_ENTROPY_GPU) ICL_TRY(entropy_ws(ctx, ws, SLAB_IMAGES));
    dz_ws B;
    dz_totals tot;
    std::vector<file_fail> fails;
    feed_worker<dz_result> work{[&](int64_t i, worker_state &wst, dz_result &z) { dz_process(job.srcs[i], wst, entropy, job.max_bytes, job.max_dim, z); }};
    {
        ingest_feed<dz_result> feed(job.n, worker_count(job.n, threads), 2 * SLAB_IMAGES, 2 * SLAB_PAYLOAD, std::ref(work), [](const dz_result &z) { return z.held(); });
        dz_round R;
        for (int64_t k = 0; feed.taken() < job.n; ++k) {
            const int q = (int)(k & 1);
            ICL_HIP(ctx, hipEventSynchronize(ws->ev_up[q])); // the upload that last read this slab has finished
            const slab_view S = ws->host(q);
            ICL_TRY(dz_collect(ctx, job, feed, S, R));
            const auto t_gpu = clk::now();
            ICL_TRY(dz_rebuild(ctx, ws, B, S, ws->ev_up[q], job.max_bytes, R));
            tot.gpu_ms += ms_since(t_gpu);
            const auto t_out = clk::now();
            dz_deliver(ws, job, R, fails, tot);
            tot.out_ms += ms_since(t_out);
        }
        ICL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    } // (the feed has joined its workers: decode_ns is complete)
    tot.decode_ns = work.decode_ns.load();
    job.out_off[job.n] = tot.bytes_out;
    ctx->downsize_last = tot;
    if (!job.out || tot.bytes_out > job.cap) return icl_fail(ctx, ICL_ERR_ARG, "%s: buffer too small (%lld bytes needed)", job.what, (long long)tot.bytes_out);
    return report_lowest(ctx, fails, job.n, job.what, nullptr);
}

} // namespace

static int downsize_images(icl_ctx *ctx, const ingest_list &imgs, int64_t max_bytes, int32_t max_dim, int32_t threads, uint8_t *out, int64_t cap, int64_t *out_off,
                           int32_t *status, const char *what)
{
    const int64_t bad = imgs.first_bad();
    if (!ctx || bad == ingest_list::NO_ARRAYS || !out_off || cap < 0 || max_bytes < 0 || max_dim < 1 || threads < 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: bad argument", what);
    if (bad >= 0) return icl_fail(ctx, ICL_ERR_ARG, "%s: paths[%lld] is NULL", what, (long long)bad);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return no_throw(ctx, what, [&]() -> int {
        const std::vector<ingest_src> srcs = imgs.srcs();
        return downsize_images_locked(ctx, dz_job{srcs.data(), imgs.n, max_bytes, max_dim, out, cap, out_off, status, what}, threads);
    });
}

extern "C" int icl_downsize_images(icl_ctx *ctx, const char *const *paths, int64_t n, int64_t max_bytes, int32_t max_dim, int32_t threads, uint8_t *out, int64_t cap,
                                   int64_t *out_off, int32_t *status)
{
    return downsize_images(ctx, ingest_list::files(paths, n), max_bytes, max_dim, threads, out, cap, out_off, status, "icl_downsize_images");
}

extern "C" int icl_downsize_images_mem(icl_ctx *ctx, const uint8_t *const *data, const int64_t *bytes, int64_t n, int64_t max_bytes, int32_t max_dim, int32_t threads,
                                       uint8_t *out, int64_t cap, int64_t *out_off, int32_t *status)
{
    return downsize_images(ctx, ingest_list::memory(data, bytes, n), max_bytes, max_dim, threads, out, cap, out_off, status, "icl_downsize_images_mem");
}

extern "C" int icl_last_downsize_stats(icl_ctx *ctx, int64_t *passthrough, int64_t *gpu_rebuilt, int64_t *host_decoded, int64_t *second_attempts, int64_t *bytes_in,
                                       int64_t *bytes_out, double *stage_ms)
{
    if (!ctx) return ICL_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    const dz_totals &t = ctx->downsize_last;
    if (passthrough) *passthrough = t.passthrough;
    if (gpu_rebuilt) *gpu_rebuilt = t.gpu_rebuilt;
    if (host_decoded) *host_decoded = t.host_decoded;
    if (second_attempts) *second_attempts = t.second_attempts;
    if (bytes_in) *bytes_in = t.bytes_in;
    if (bytes_out) *bytes_out = t.bytes_out;
    if (stage_ms) stage_ms[0] = (double)t.decode_ns * 1e-6, stage_ms[1] = t.gpu_ms, stage_ms[2] = t.out_ms;
    return ICL_OK;
}
