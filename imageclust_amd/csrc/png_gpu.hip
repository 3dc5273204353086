// png_gpu.hip -- PNG on the GPU for the batched file path (jpeg_gpu.hip): the kernels that take a PNG's zlib stream, as host stage P0
// (png_decode.hip, icl_png_parse) left it in the slab's payload, to unfiltered scanlines in the slab's scratch, from which
// jpeg_gather_resize_kernel samples.  The arithmetic and the inflate schedule are png_inflate.h's, which the host rehearsal
// (icl_png_raw_file_host) runs too.
//   png_inflate_kernel   one workgroup (one wave) per PNG, no communication between workgroups: DEFLATE with the window as an LDS ring
//   png_adler_kernel     Adler-32 of the inflated bytes by position-weighted chunks, against the stream's trailer
//   png_unfilter_kernel  the five filters in place: bands of 64 rows, lane l one pixel behind lane l - 1
// The GPU never produces a status: d_ok[i] is set only when the stream was legal by the host decoder's rules and ended with exactly the
// expected byte count, the Adler-32 matched, every filter byte was 0..4 and no palette index was out of range.  Everything else is
// redone by the host decoder (ingest_files' repair pass).
// Hostile input: every length is the file's.  icl_png_job checks descriptor, stream and scanlines against the buffers' extents before
// anything is touched; LDS indices are masked to their arrays; the inflate loop is bounded by the stream's bits plus `want`.
#include "icl_common.h"
#include "ingest_slab.h"
#include "png_inflate.h"

namespace {

__global__ void __launch_bounds__(ICL_PNG_LANES) png_inflate_kernel(const ingest_image *__restrict__ imgs, const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                                    uint8_t *__restrict__ scratch, int64_t scratch_bytes, int32_t *__restrict__ ok)
{
    __shared__ icl_png_lds L;
    const ingest_image &I = imgs[blockIdx.x];
    const icl_png_desc *D = icl_png_job(I, payload, payload_bytes, scratch_bytes);
    if (!D) {
        if (threadIdx.x == 0) ok[blockIdx.x] = 0;
        return;
    }
    const int lane = (int)threadIdx.x;
    icl_png_inflate_run(L, payload + I.host_off + sizeof(icl_png_desc), (int64_t)D->zbytes, scratch + I.yplane, D->want, lane, lane + 1, [] { __syncthreads(); });
    if (lane == 0) ok[blockIdx.x] = L.ok;
}

constexpr int ADLER_THREADS = 256;

__global__ void __launch_bounds__(ADLER_THREADS) png_adler_kernel(const ingest_image *__restrict__ imgs, const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                                  const uint8_t *__restrict__ scratch, int64_t scratch_bytes, int32_t *__restrict__ ok)
{
    __shared__ uint32_t sum[2];
    const ingest_image &I = imgs[blockIdx.x];
    const icl_png_desc *D = icl_png_job(I, payload, payload_bytes, scratch_bytes);
    if (!D || !ok[blockIdx.x]) return;
    if (threadIdx.x == 0) sum[0] = sum[1] = 0;
    __syncthreads();
    const int64_t n = D->want, nchunk = (n + ICL_ADLER_CHUNK - 1) / ICL_ADLER_CHUNK;
    const uint8_t *p = scratch + I.yplane;
    uint32_t sa = 0, sb = 0;
    for (int64_t c = threadIdx.x; c < nchunk; c += ADLER_THREADS) {
        const int64_t s = c * ICL_ADLER_CHUNK;
        const int m = (int)(n - s < ICL_ADLER_CHUNK ? n - s : ICL_ADLER_CHUNK);
        icl_adler_chunk(p + s, m, n - s - m, sa, sb);
    }
    atomicAdd(&sum[0], sa); // (256 sums below 65521 each)
    atomicAdd(&sum[1], sb);
    __syncthreads();
    if (threadIdx.x == 0 && icl_adler_finish(sum[0], sum[1], n) != D->adler) ok[blockIdx.x] = 0;
}

__device__ __forceinline__ uint64_t shfl_up1(uint64_t v)
{
    const uint32_t lo = __shfl_up((uint32_t)v, 1), hi = __shfl_up((uint32_t)(v >> 32), 1);
    return ((uint64_t)hi << 32) | lo;
}

// In place on the scanlines.  Average and Paeth are serial along a row and down the rows, but pixel (x, y) needs only (x - 1, y), (x, y - 1)
// and (x - 1, y - 1): lane l works on row r0 + l and is at pixel t - l at step t.  Its left neighbour stays in a register; the pixel above is
// what lane l - 1 produced one step earlier (a shuffle; lane 0 reads the previous band's last row, final behind the barrier), and
// above-left is the lane's own previous `above`.
__global__ void __launch_bounds__(ICL_PNG_LANES) png_unfilter_kernel(const ingest_image *__restrict__ imgs, const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                                     uint8_t *__restrict__ scratch, int64_t scratch_bytes, int32_t *__restrict__ ok)
{
    const ingest_image &I = imgs[blockIdx.x];
    const icl_png_desc *D = icl_png_job(I, payload, payload_bytes, scratch_bytes);
    if (!D || !ok[blockIdx.x]) return;
    const int lane = (int)threadIdx.x, bpp = D->bpp, w = D->w, depth = D->depth, npal = D->npal;
    const int64_t h = D->h, rowb = D->rowb, pitch = rowb + 1, npx = rowb / bpp;
    const bool check_pal = D->ctype == 3 && npal < (1 << depth);
    uint8_t *base = scratch + I.yplane;
    bool bad = false;
    for (int64_t r0 = 0; r0 < h; r0 += ICL_PNG_LANES) {
        const int64_t row = r0 + lane;
        const bool active = row < h;
        uint8_t *line = base + (active ? row : 0) * pitch;
        int ft = active ? line[0] : 0;
        if (ft > 4) {
            bad = true;
            ft = 0;
        }
        uint64_t left = 0, above = 0, mine = 0;
        const int64_t steps = npx + (h - r0 < ICL_PNG_LANES ? h - r0 : ICL_PNG_LANES) - 1;
        for (int64_t t = 0; t < steps; ++t) {
            const uint64_t from_up = shfl_up1(mine);
            const int64_t x = t - lane;
            if (active && x >= 0 && x < npx) {
                uint8_t *px = line + 1 + x * bpp;
                const uint64_t b = lane == 0 ? (row > 0 ? icl_png_load_px(px - pitch, bpp) : 0) : from_up;
                const uint64_t c = x > 0 ? above : 0, a = x > 0 ? left : 0;
                const uint64_t o = icl_png_unfilter_px(ft, bpp, icl_png_load_px(px, bpp), a, b, c);
                icl_png_store_px(px, bpp, o);
                if (check_pal && icl_png_pal_bad((uint32_t)(o & 255u), x, w, depth, npal)) bad = true;
                left = o;
                above = b;
                mine = o;
            }
        }
        __syncthreads();
    }
    if (bad) ok[blockIdx.x] = 0;
}

} // namespace

int icl_png_decode_slab(icl_ctx *ctx, hipStream_t st, const ingest_image *d_imgs, int nimg, const uint8_t *d_payload, int64_t payload_bytes, uint8_t *d_scratch,
                        int64_t scratch_bytes, int32_t *d_ok, int stages)
{
    if (nimg <= 0) return ICL_OK;
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)nimg), dim3(ICL_PNG_LANES), 0, st, d_imgs, d_payload, payload_bytes, d_scratch, scratch_bytes, d_ok);
    ICL_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(png_adler_kernel, dim3((unsigned)nimg), dim3(ADLER_THREADS), 0, st, d_imgs, d_payload, payload_bytes, (const uint8_t *)d_scratch, scratch_bytes, d_ok);
    ICL_HIP(ctx, hipGetLastError());
    if (stages >= 2) {
        hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)nimg), dim3(ICL_PNG_LANES), 0, st, d_imgs, d_payload, payload_bytes, d_scratch, scratch_bytes, d_ok);
        ICL_HIP(ctx, hipGetLastError());
    }
    return ICL_OK;
}
