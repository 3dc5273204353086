// jpeg_encode_gpu.hip -- the batched JPEG encoder on the GPU: n resident RGB images of any sizes -> n complete files, byte-equal to the
// host encoder's (jpeg_encode.hip) because both run the arithmetic of jpeg_encode_pixels.h.  Everything of one batch is enqueued on the
// context's stream without a host round trip; the host reads the file offsets once at the end.
//
//   jenc_block_kernel    one thread per 8x8 block of the batch in scan order (6 per MCU: Y00 Y01 Y10 Y11 Cb Cr): colour conversion,
//                        downsampling, forward DCT, quantisation -> 64 int16 in zig-zag order (dummy blocks: zeros)
//   jenc_length_kernel   one thread per block: its DC difference (the predecessor's quantised DC is final by now) and coded length in bits
//   jenc_scan_kernel     one workgroup per image: exclusive scan of the lengths (then of the chunks' 0xFF counts)
//   jenc_zero_kernel     clears the words the image's bits will occupy
//   jenc_pack_kernel     one thread per block: its bits at its offset; neighbouring blocks share words, so every word is OR-ed in atomically
//   jenc_count_kernel    one thread per 256-byte chunk of the unstuffed stream: its 0xFF bytes
//   jenc_offsets_kernel  file sizes and offsets of the batch
//   jenc_emit_kernel     one thread per chunk: its bytes, a 0x00 behind every 0xFF, at its place in the file; jenc_header_kernel: header, EOI
#include "icl_common.h"
#include "jpeg_encode_pixels.h"
#include "jpeg_stage.h"

#include <cstring>
#include <memory>

namespace {

constexpr int JT = 64;          // threads of the per-block kernels
constexpr int CHUNK = 256;      // unstuffed bytes per thread of the stuffing pass
constexpr int SCAN_T = 256;
constexpr int64_t MAX_BATCH_BLOCKS = 4ll << 20; // blocks of one batch (its buffers: about 800 bytes per block)
constexpr int64_t MAX_BATCH_IMAGES = 65535;     // images of one batch: the per-image kernels take the image from gridDim.y

struct jenc_img { // one image of a batch (host-computed; every capacity is the proven bound)
    int64_t rgb_off;
    int64_t first_block, nblocks;
    int64_t raw_off, raw_words; // its unstuffed stream: first word, words reserved
    int64_t first_chunk, chunks_cap;
    icl_jenc_geom g;
    int32_t pad_;
};
struct jenc_state { // what the kernels learn about it
    unsigned long long totbits, nff;
};
struct jenc_dev_tables {
    icl_jenc_tables T;
    uint8_t header[ICL_JENC_HEADER + 1];
};

__device__ __forceinline__ int find_img(const jenc_img *imgs, int n, int64_t g)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].first_block <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(JT) jenc_block_kernel(const jenc_img *__restrict__ imgs, int n, const jenc_dev_tables *__restrict__ tab,
                                                        const uint8_t *__restrict__ rgb, int16_t *__restrict__ coef, int64_t total_blocks)
{
    const int64_t gb = (int64_t)blockIdx.x * JT + threadIdx.x;
    if (gb >= total_blocks) return;
    const jenc_img &I = imgs[find_img(imgs, n, gb)];
    const int64_t b = gb - I.first_block;
    if (b < 0 || b >= I.nblocks) return;
    const int64_t m = b / 6;
    const int k = (int)(b - m * 6), my = (int)(m / I.g.mw), mx = (int)(m - (int64_t)my * I.g.mw);
    uint4 *dst = (uint4 *)(coef + gb * 64);
    if (icl_jenc_is_dummy(I.g, mx, my, k)) {
#pragma unroll
        for (int q = 0; q < 8; ++q) dst[q] = make_uint4(0, 0, 0, 0);
        return;
    }
    int s[64];
    icl_jenc_block_samples(rgb + I.rgb_off, I.g, mx, my, k, s);
    int16_t zz[64];
    icl_jenc_block_coefs(s, tab->T.qt[k < 4 ? 0 : 1], zz);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = (uint32_t)(uint16_t)zz[q * 8 + 2 * e] | ((uint32_t)(uint16_t)zz[q * 8 + 2 * e + 1] << 16);
        dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the quantised DC of block b of an image: a dummy carries the DC of the block before it in scan order (Y00 is never a dummy)
__device__ __forceinline__ int dc_of(const jenc_img &I, const int16_t *cf, int64_t b)
{
    for (;;) {
        const int64_t m = b / 6;
        const int k = (int)(b - m * 6), my = (int)(m / I.g.mw), mx = (int)(m - (int64_t)my * I.g.mw);
        if (k == 0 || !icl_jenc_is_dummy(I.g, mx, my, k)) return cf[b * 64];
        --b;
    }
}
__device__ __forceinline__ int dc_diff_of(const jenc_img &I, const int16_t *cf, int64_t b)
{
    const int64_t m = b / 6;
    const int64_t p = icl_jenc_dc_pred_block(m, (int)(b - m * 6));
    return dc_of(I, cf, b) - (p < 0 ? 0 : dc_of(I, cf, p));
}

struct coef_reader {
    const int16_t *p;
    __device__ __forceinline__ int operator()(int k) const { return p[k]; }
};

__global__ void __launch_bounds__(JT) jenc_length_kernel(const jenc_img *__restrict__ imgs, int n, const jenc_dev_tables *__restrict__ tab,
                                                         const int16_t *__restrict__ coef, uint32_t *__restrict__ len, int64_t total_blocks)
{
    const int64_t gb = (int64_t)blockIdx.x * JT + threadIdx.x;
    if (gb >= total_blocks) return;
    const jenc_img &I = imgs[find_img(imgs, n, gb)];
    const int64_t b = gb - I.first_block;
    if (b < 0 || b >= I.nblocks) return;
    const int16_t *cf = coef + I.first_block * 64;
    const int k = (int)(b % 6);
    icl_jenc_count_sink sink;
    icl_jenc_encode_block(coef_reader{cf + b * 64}, dc_diff_of(I, cf, b), tab->T, k < 4 ? ICL_JENC_DC0 : ICL_JENC_DC1, k < 4 ? ICL_JENC_AC0 : ICL_JENC_AC1, sink);
    len[gb] = sink.bits;
}

// exclusive scan of in[first .. first + cnt) into out, by one workgroup; returns the total (valid in every thread)
__device__ unsigned long long segment_scan(const uint32_t *in, unsigned long long *out, int64_t first, int64_t cnt)
{
    __shared__ unsigned long long part[SCAN_T];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < cnt; base += SCAN_T) {
        const int64_t i = base + threadIdx.x;
        const unsigned long long v = i < cnt ? in[first + i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < SCAN_T; d <<= 1) {
            const unsigned long long a = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += a;
            __syncthreads();
        }
        if (i < cnt) out[first + i] = carry + part[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 0) carry += part[SCAN_T - 1];
        __syncthreads();
    }
    return carry;
}

__device__ __forceinline__ int64_t raw_bytes_of(const jenc_state &s) { return (int64_t)((s.totbits + 7) >> 3); }
__device__ __forceinline__ int64_t chunks_of(const jenc_img &I, const jenc_state &s)
{
    const int64_t c = (raw_bytes_of(s) + CHUNK - 1) / CHUNK;
    return c < I.chunks_cap ? c : I.chunks_cap;
}

__global__ void __launch_bounds__(SCAN_T) jenc_scan_kernel(const jenc_img *__restrict__ imgs, jenc_state *__restrict__ st, const uint32_t *__restrict__ in,
                                                           unsigned long long *__restrict__ out, int chunks)
{
    const jenc_img &I = imgs[blockIdx.x];
    if (!chunks) {
        const unsigned long long t = segment_scan(in, out, I.first_block, I.nblocks);
        if (threadIdx.x == 0) st[blockIdx.x].totbits = t;
    } else {
        const unsigned long long t = segment_scan(in, out, I.first_chunk, chunks_of(I, st[blockIdx.x]));
        if (threadIdx.x == 0) st[blockIdx.x].nff = t;
    }
}

__global__ void __launch_bounds__(256) jenc_zero_kernel(const jenc_img *__restrict__ imgs, const jenc_state *__restrict__ st, uint32_t *__restrict__ raw)
{
    const jenc_img &I = imgs[blockIdx.y];
    int64_t words = (int64_t)((st[blockIdx.y].totbits + 31) >> 5) + 1;
    if (words > I.raw_words) words = I.raw_words;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (int64_t)gridDim.x * 256) raw[I.raw_off + i] = 0;
}

// the bits of one block into the image's stream at bit position pos: most significant bit first, in 32-bit words
struct pack_sink {
    uint32_t *words;
    int64_t nwords, widx;
    uint64_t acc;
    int nacc;
    __device__ __forceinline__ pack_sink(uint32_t *w, int64_t nw, unsigned long long pos) : words(w), nwords(nw), widx((int64_t)(pos >> 5)), acc(0), nacc((int)(pos & 31)) {}
    __device__ __forceinline__ void store(uint32_t v)
    {
        if (v && widx < nwords) atomicOr(words + widx, v);
        ++widx;
    }
    __device__ __forceinline__ void put(uint32_t v, int n)
    {
        acc = (acc << n) | v;
        nacc += n;
        if (nacc >= 32) {
            store((uint32_t)(acc >> (nacc - 32)));
            nacc -= 32;
            acc &= ((uint64_t)1 << nacc) - 1;
        }
    }
    __device__ __forceinline__ void flush()
    {
        if (nacc) store((uint32_t)(acc << (32 - nacc)));
    }
};

__global__ void __launch_bounds__(JT) jenc_pack_kernel(const jenc_img *__restrict__ imgs, int n, const jenc_state *__restrict__ st,
                                                       const jenc_dev_tables *__restrict__ tab, const int16_t *__restrict__ coef,
                                                       const unsigned long long *__restrict__ bitoff, uint32_t *__restrict__ raw, int64_t total_blocks)
{
    const int64_t gb = (int64_t)blockIdx.x * JT + threadIdx.x;
    if (gb >= total_blocks) return;
    const int ii = find_img(imgs, n, gb);
    const jenc_img &I = imgs[ii];
    const int64_t b = gb - I.first_block;
    if (b < 0 || b >= I.nblocks) return;
    const int16_t *cf = coef + I.first_block * 64;
    const int k = (int)(b % 6);
    pack_sink sink(raw + I.raw_off, I.raw_words, bitoff[gb]);
    icl_jenc_encode_block(coef_reader{cf + b * 64}, dc_diff_of(I, cf, b), tab->T, k < 4 ? ICL_JENC_DC0 : ICL_JENC_DC1, k < 4 ? ICL_JENC_AC0 : ICL_JENC_AC1, sink);
    if (b == I.nblocks - 1) { // the last partial byte is padded with 1 bits
        const int pad = (int)((8 - (st[ii].totbits & 7)) & 7);
        if (pad) sink.put((1u << pad) - 1, pad);
    }
    sink.flush();
}

__device__ __forceinline__ uint32_t raw_byte(const uint32_t *raw, int64_t j) { return (raw[j >> 2] >> (24 - 8 * (int)(j & 3))) & 255u; }

__global__ void __launch_bounds__(256) jenc_count_kernel(const jenc_img *__restrict__ imgs, const jenc_state *__restrict__ st, const uint32_t *__restrict__ raw,
                                                         uint32_t *__restrict__ cnt)
{
    const jenc_img &I = imgs[blockIdx.y];
    const int64_t nraw = raw_bytes_of(st[blockIdx.y]), nch = chunks_of(I, st[blockIdx.y]);
    const uint32_t *r = raw + I.raw_off;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nch; c += (int64_t)gridDim.x * 256) {
        const int64_t e = min(nraw, (c + 1) * CHUNK);
        uint32_t k = 0;
        for (int64_t j = c * CHUNK; j < e; ++j) k += raw_byte(r, j) == 255u;
        cnt[I.first_chunk + c] = k;
    }
}

__global__ void jenc_offsets_kernel(const jenc_state *__restrict__ st, int n, int64_t *__restrict__ off)
{
    if (blockIdx.x || threadIdx.x) return;
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = at;
        at += ICL_JENC_HEADER + raw_bytes_of(st[i]) + (int64_t)st[i].nff + 2;
    }
    off[n] = at;
}

__global__ void __launch_bounds__(256) jenc_emit_kernel(const jenc_img *__restrict__ imgs, const jenc_state *__restrict__ st, const uint32_t *__restrict__ raw,
                                                        const unsigned long long *__restrict__ ffoff, const int64_t *__restrict__ off, uint8_t *__restrict__ out,
                                                        int64_t cap)
{
    const jenc_img &I = imgs[blockIdx.y];
    const int64_t lo = off[blockIdx.y], hi = off[blockIdx.y + 1];
    if (hi > cap) return; // (the host reports the size needed)
    const int64_t nraw = raw_bytes_of(st[blockIdx.y]), nch = chunks_of(I, st[blockIdx.y]);
    const uint32_t *r = raw + I.raw_off;
    const int64_t end = hi - 2;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nch; c += (int64_t)gridDim.x * 256) {
        int64_t d = lo + ICL_JENC_HEADER + c * CHUNK + (int64_t)ffoff[I.first_chunk + c];
        const int64_t e = min(nraw, (c + 1) * CHUNK);
        for (int64_t j = c * CHUNK; j < e; ++j) {
            const uint32_t v = raw_byte(r, j);
            if (d < end) out[d] = (uint8_t)v;
            ++d;
            if (v == 255u) {
                if (d < end) out[d] = 0;
                ++d;
            }
        }
    }
}

__global__ void __launch_bounds__(256) jenc_header_kernel(const jenc_img *__restrict__ imgs, const jenc_dev_tables *__restrict__ tab, const int64_t *__restrict__ off,
                                                          uint8_t *__restrict__ out, int64_t cap)
{
    const jenc_img &I = imgs[blockIdx.x];
    const int64_t lo = off[blockIdx.x], hi = off[blockIdx.x + 1];
    if (hi > cap || hi - lo < ICL_JENC_HEADER + 2) return;
    constexpr int SOF = 2 + 18 + 2 * 69; // FF C0, length, precision, then height and width
    for (int i = threadIdx.x; i < ICL_JENC_HEADER; i += 256) {
        uint8_t v = tab->header[i];
        if (i == SOF + 5) v = (uint8_t)(I.g.H >> 8);
        if (i == SOF + 6) v = (uint8_t)(I.g.H & 255);
        if (i == SOF + 7) v = (uint8_t)(I.g.W >> 8);
        if (i == SOF + 8) v = (uint8_t)(I.g.W & 255);
        out[lo + i] = v;
    }
    if (threadIdx.x == 0) {
        out[hi - 2] = 0xFF;
        out[hi - 1] = 0xD9;
    }
}

} // namespace

// Buffers of the GPU encoder, kept by the context between calls and grown on demand (freed by icl_destroy).
struct icl_jenc_ws {
    icl_dev_grow imgs, state, off;                          // jenc_img[n], jenc_state[n], int64_t[n + 1]
    icl_dev_grow tab;                                       // jenc_dev_tables of tab_quality
    int tab_quality = 0;
    icl_dev_grow coef, len, bitoff, raw, cnt, ffoff, out;   // int16_t[64 blocks], uint32_t[blocks], u64[blocks], uint32_t[words], uint32_t[chunks], u64[chunks], the files
    int64_t *h_off = nullptr; // pinned
    int64_t h_off_cap = 0;
};

void icl_jenc_free(icl_ctx *ctx)
{
    if (!ctx->jenc) return;
    icl_jenc_ws *ws = ctx->jenc;
    for (icl_dev_grow *b : {&ws->imgs, &ws->state, &ws->off, &ws->tab, &ws->coef, &ws->len, &ws->bitoff, &ws->raw, &ws->cnt, &ws->ffoff, &ws->out}) b->release();
    if (ws->h_off) (void)hipHostFree(ws->h_off);
    delete ws;
    ctx->jenc = nullptr;
}

int64_t icl_jenc_max_batch_blocks() { return MAX_BATCH_BLOCKS; }
int64_t icl_jenc_max_batch_images() { return MAX_BATCH_IMAGES; }
int64_t icl_jenc_blocks(int w, int h)
{
    const icl_jenc_geom g = icl_jenc_geometry(w, h);
    return (int64_t)g.mw * g.mh * 6;
}

// One batch (at most MAX_BATCH_BLOCKS blocks and MAX_BATCH_IMAGES images; expects ctx->mu held and the device selected): the files into the workspace's own
// buffer *d_files, file i at off[i] .. off[i + 1].  Ends with the stream synchronised.
int icl_jenc_run(icl_ctx *ctx, const uint8_t *d_rgb, const icl_jenc_item *items, int64_t n, int quality, const uint8_t **d_files, std::vector<int64_t> &off)
{
    off.assign((size_t)n + 1, 0);
    *d_files = nullptr;
    if (n == 0) return ICL_OK;
    if (n > MAX_BATCH_IMAGES) return icl_fail(ctx, ICL_ERR_ARG, "JPEG encoder: %lld images in one batch (at most %lld)", (long long)n, (long long)MAX_BATCH_IMAGES);
    if (!ctx->jenc) ctx->jenc = new icl_jenc_ws();
    icl_jenc_ws *ws = ctx->jenc;
    hipStream_t st = ctx->stream;
    std::vector<jenc_img> imgs((size_t)n);
    int64_t blocks = 0, words = 0, chunks = 0, out_need = 0, max_words = 0, max_chunks = 0;
    for (int64_t i = 0; i < n; ++i) {
        jenc_img &I = imgs[(size_t)i];
        memset(&I, 0, sizeof I);
        I.g = icl_jenc_geometry(items[i].w, items[i].h);
        I.rgb_off = items[i].rgb_off;
        I.first_block = blocks;
        I.nblocks = (int64_t)I.g.mw * I.g.mh * 6;
        I.raw_off = words;
        I.raw_words = I.nblocks * (ICL_JENC_BLOCK_BITS / 32) + 2; // the bound on its bits, the padding, one word of slack
        I.first_chunk = chunks;
        I.chunks_cap = icl_ceil_div(I.raw_words * 4, CHUNK);
        blocks += I.nblocks;
        words += I.raw_words;
        chunks += I.chunks_cap;
        out_need += icl_jenc_bound(items[i].w, items[i].h);
        max_words = std::max(max_words, I.raw_words);
        max_chunks = std::max(max_chunks, I.chunks_cap);
    }
    if (blocks > MAX_BATCH_BLOCKS) return icl_fail(ctx, ICL_ERR_OVERSIZE, "JPEG encoder: %lld blocks in one batch (at most %lld)", (long long)blocks, (long long)MAX_BATCH_BLOCKS);
    const char *what = "JPEG encoder: device buffer";
    ICL_TRY(ws->imgs.ensure(ctx, (size_t)n * sizeof(jenc_img), what));
    ICL_TRY(ws->state.ensure(ctx, (size_t)n * sizeof(jenc_state), what));
    ICL_TRY(ws->off.ensure(ctx, (size_t)(n + 1) * 8, what));
    ICL_TRY(ws->coef.ensure(ctx, (size_t)blocks * 64 * 2, what));
    ICL_TRY(ws->len.ensure(ctx, (size_t)blocks * 4, what));
    ICL_TRY(ws->bitoff.ensure(ctx, (size_t)blocks * 8, what));
    ICL_TRY(ws->raw.ensure(ctx, (size_t)words * 4, what));
    ICL_TRY(ws->cnt.ensure(ctx, (size_t)chunks * 4, what));
    ICL_TRY(ws->ffoff.ensure(ctx, (size_t)chunks * 8, what));
    ICL_TRY(ws->out.ensure(ctx, (size_t)out_need, what));
    if (ws->h_off_cap < n + 1) {
        if (ws->h_off) (void)hipHostFree(ws->h_off);
        ws->h_off = nullptr;
        ws->h_off_cap = 0;
        if (hipHostMalloc((void **)&ws->h_off, (size_t)(n + 1) * 8, hipHostMallocDefault) != hipSuccess) return icl_fail(ctx, ICL_ERR_NOMEM, "JPEG encoder: pinned offsets");
        ws->h_off_cap = n + 1;
    }
    if (!ws->tab.p) ws->tab_quality = 0;
    ICL_TRY(ws->tab.ensure(ctx, sizeof(jenc_dev_tables), "JPEG encoder: tables"));
    if (ws->tab_quality != quality) {
        std::unique_ptr<jenc_dev_tables> t(new jenc_dev_tables());
        memset(t.get(), 0, sizeof *t);
        icl_jenc_make_tables(quality, t->T);
        icl_jenc_write_header(t->T, 0, 0, t->header);
        ICL_HIP(ctx, hipMemcpyAsync(ws->tab.p, t.get(), sizeof *t, hipMemcpyHostToDevice, st));
        ICL_HIP(ctx, hipStreamSynchronize(st)); // (t goes out of scope)
        ws->tab_quality = quality;
    }
    const jenc_img *d_imgs = ws->imgs.as<jenc_img>();
    jenc_state *d_state = ws->state.as<jenc_state>();
    const jenc_dev_tables *d_tab = ws->tab.as<jenc_dev_tables>();
    int64_t *d_off = ws->off.as<int64_t>();
    int16_t *d_coef = ws->coef.as<int16_t>();
    uint32_t *d_len = ws->len.as<uint32_t>(), *d_raw = ws->raw.as<uint32_t>(), *d_cnt = ws->cnt.as<uint32_t>();
    unsigned long long *d_bitoff = ws->bitoff.as<unsigned long long>(), *d_ffoff = ws->ffoff.as<unsigned long long>();
    uint8_t *d_out = ws->out.as<uint8_t>();
    const int64_t out_cap = (int64_t)ws->out.bytes;
    ICL_HIP(ctx, hipMemcpyAsync(ws->imgs.p, imgs.data(), (size_t)n * sizeof(jenc_img), hipMemcpyHostToDevice, st));
    const unsigned gb = (unsigned)icl_ceil_div(blocks, JT);
    const int ni = (int)n;
    hipLaunchKernelGGL(jenc_block_kernel, dim3(gb), dim3(JT), 0, st, d_imgs, ni, d_tab, d_rgb, d_coef, blocks);
    hipLaunchKernelGGL(jenc_length_kernel, dim3(gb), dim3(JT), 0, st, d_imgs, ni, d_tab, (const int16_t *)d_coef,
                       d_len, blocks);
    hipLaunchKernelGGL(jenc_scan_kernel, dim3((unsigned)n), dim3(SCAN_T), 0, st, d_imgs, d_state, (const uint32_t *)d_len, d_bitoff, 0);
    const unsigned gz = (unsigned)std::min<int64_t>(icl_ceil_div(max_words, 256), 4096), gc = (unsigned)std::min<int64_t>(icl_ceil_div(max_chunks, 256), 4096);
    hipLaunchKernelGGL(jenc_zero_kernel, dim3(gz, (unsigned)n), dim3(256), 0, st, d_imgs, (const jenc_state *)d_state, d_raw);
    hipLaunchKernelGGL(jenc_pack_kernel, dim3(gb), dim3(JT), 0, st, d_imgs, ni, (const jenc_state *)d_state, d_tab,
                       (const int16_t *)d_coef, (const unsigned long long *)d_bitoff, d_raw, blocks);
    hipLaunchKernelGGL(jenc_count_kernel, dim3(gc, (unsigned)n), dim3(256), 0, st, d_imgs, (const jenc_state *)d_state,
                       (const uint32_t *)d_raw, d_cnt);
    hipLaunchKernelGGL(jenc_scan_kernel, dim3((unsigned)n), dim3(SCAN_T), 0, st, d_imgs, d_state, (const uint32_t *)d_cnt, d_ffoff, 1);
    hipLaunchKernelGGL(jenc_offsets_kernel, dim3(1), dim3(1), 0, st, (const jenc_state *)d_state, ni, d_off);
    hipLaunchKernelGGL(jenc_emit_kernel, dim3(gc, (unsigned)n), dim3(256), 0, st, d_imgs, (const jenc_state *)d_state, (const uint32_t *)d_raw,
                       (const unsigned long long *)d_ffoff, (const int64_t *)d_off, d_out, out_cap);
    hipLaunchKernelGGL(jenc_header_kernel, dim3((unsigned)n), dim3(256), 0, st, d_imgs, d_tab, (const int64_t *)d_off,
                       d_out, out_cap);
    ICL_HIP(ctx, hipGetLastError());
    ICL_HIP(ctx, hipMemcpyAsync(ws->h_off, d_off, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
    ICL_HIP(ctx, hipStreamSynchronize(st));
    for (int64_t i = 0; i <= n; ++i) off[(size_t)i] = ws->h_off[i];
    if (off[(size_t)n] > out_cap) return icl_fail(ctx, ICL_ERR_IO, "JPEG encoder: a stream exceeded its proven bound");
    *d_files = d_out;
    return ICL_OK;
}

extern "C" int icl_jpeg_encode_rgb_dev(icl_ctx *ctx, const uint8_t *d_rgb, const int64_t *offsets, const int32_t *w, const int32_t *h, int64_t n, int32_t quality,
                                       uint8_t *out, int32_t out_on_device, int64_t cap, int64_t *out_off)
{
    if (!ctx || n < 0 || !out_off || cap < 0 || (n && (!d_rgb || !offsets || !w || !h))) return icl_fail(ctx, ICL_ERR_ARG, "icl_jpeg_encode_rgb_dev: bad argument");
    if (quality < 1 || quality > 100) return icl_fail(ctx, ICL_ERR_ARG, "icl_jpeg_encode_rgb_dev: quality %d is outside 1..100", (int)quality);
    for (int64_t i = 0; i < n; ++i)
        if (w[i] < 1 || h[i] < 1 || w[i] > 65535 || h[i] > 65535 || offsets[i] < 0)
            return icl_fail(ctx, ICL_ERR_ARG, "icl_jpeg_encode_rgb_dev: image %lld: %d x %d is outside 1..65535", (long long)i, (int)w[i], (int)h[i]);
    std::lock_guard<std::mutex> lk(ctx->mu);
    icl_device_guard g(ctx->device);
    return no_throw(ctx, "icl_jpeg_encode_rgb_dev", [&]() -> int {
        int64_t at = 0;
        out_off[0] = 0;
        std::vector<icl_jenc_item> items;
        std::vector<int64_t> off;
        for (int64_t i = 0; i < n;) { // batches of at most MAX_BATCH_BLOCKS blocks and MAX_BATCH_IMAGES images
            items.clear();
            int64_t blocks = 0, j = i;
            for (; j < n; ++j) {
                const int64_t nb = icl_jenc_blocks(w[j], h[j]);
                if (!items.empty() && (blocks + nb > MAX_BATCH_BLOCKS || (int64_t)items.size() >= MAX_BATCH_IMAGES)) break;
                items.push_back(icl_jenc_item{offsets[j], w[j], h[j]});
                blocks += nb;
            }
            const uint8_t *d_files = nullptr;
            ICL_TRY(icl_jenc_run(ctx, d_rgb, items.data(), (int64_t)items.size(), quality, &d_files, off));
            const int64_t total = off.back();
            if (out && at + total <= cap && total)
                ICL_HIP(ctx, hipMemcpyAsync(out + at, d_files, (size_t)total, out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
            ICL_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the next batch reuses the buffer
            for (int64_t q = i; q < j; ++q) out_off[q + 1] = at + off[(size_t)(q - i) + 1];
            at += total;
            i = j;
        }
        if (!out || at > cap) return icl_fail(ctx, ICL_ERR_ARG, "icl_jpeg_encode_rgb_dev: buffer too small (%lld bytes needed)", (long long)at);
        return ICL_OK;
    });
}
