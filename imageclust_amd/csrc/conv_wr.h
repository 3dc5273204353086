// conv_wr.h -- the HBM-bound 1x1 convolutions of the identity bottlenecks (c3: Cout = 4 K, y = relu(bn(conv(t2)) + x)) as a STREAMING kernel
// (bf16; included by resnet.hip).
//
// These layers (128 -> 512 at 28x28, 256 -> 1024 at 14x14: 650 of the 3 500 us of a forward pass) move 9 bytes per MAC-poor output: the residual
// read and the output write dominate, K is 2-4 K-tiles, and the 128 x 128 kernel (conv_igemm_kernel, two workgroups per CU) ran them at
// 3.4-4.3 TB/s: every tile re-stages its weights through LDS and goes through load -> wait -> MFMA -> LDS transposition -> store in sequence.
// Here (the back-wave design of bneck56_kernel, on its own):
//   weights in REGISTERS  a workgroup owns NS output channels for the whole launch; wave w holds its NS / 4 channels x K as MFMA A fragments
//                         (64 VGPRs), loaded once: no weight byte crosses L2 -> LDS again
//   persistent            workgroup (slice, worker) walks the 64-pixel tiles worker, worker + nworkers, ...; two workgroups of 4 waves per CU
//                         run out of phase (memory beside MFMA)
//   A tile                64 pixels x K by LDS-DMA into a double buffer (the tile after next is requested while this one is consumed)
//   residual              requested one tile ahead, 16 bytes per lane in the layout the epilogue ends in
//   epilogue              in registers (v_permlane16_swap, conv_p8.h): 8 consecutive channels per lane, fp32 scale/shift + residual + ReLU, one rounding
// The slices of one worker sit on one XCD (blocks b, b + 8, ...): the A tile they share crosses the fabric once.
// MAP (the c3 of a bottleneck whose output is read at a stride only, prune_map.h): the rows of X are the pixels that are read, compact;
// the residual and the output stay full-size tensors and row m is their pixel prune_map_pixel(pm, m) -- one offset for the residual load and
// the store, nothing else differs.  The instantiations without MAP are the code they were before the flag (profiles/r37_isa_compare.txt).
#pragma once
#include "conv_select.h"
#include "mfma_tile.h"
#include "prune_map.h"
#include "resnet_fused.h"

// the LDS-DMA pieces (32 rows each: 4 waves x 8 rows x 128 B, 4 KiB apart) of ONE 64-channel chunk of a PT-pixel A image (PT = 64: two pieces,
// PT = 32: one).  The chunk's channels are selected by the SCALAR offset (128 * chunk): an instruction offset would be added to the LDS address
// as well (MUBUF with lds = 1); lds0 is the chunk's PT * 128 bytes of the image
template <int NP>
__device__ __forceinline__ void wr_dma_chunk(const i32x4_t &srd, unsigned v0, unsigned v1, unsigned soff, unsigned lds0)
{
    unsigned keep;
    if constexpr (NP == 2)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\t"
                     "s_mov_b32 m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(v0), "v"(v1), "s"(srd), "s"(soff), "s"(lds0), "s"(lds0 + 4096u)
                     : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(v0), "s"(srd), "s"(soff), "s"(lds0)
                     : "memory");
}
template <int KC, int PT>
__device__ __forceinline__ void wr_dma(const i32x4_t &srd, unsigned v0, unsigned v1, unsigned lds0)
{
    static_assert(PT == 64 || PT == 32, "64- or 32-pixel tiles");
#pragma unroll
    for (int c = 0; c < KC; ++c) wr_dma_chunk<PT / 32>(srd, v0, v1, 128u * c, lds0 + (unsigned)(PT * 128) * c);
}

struct wr_args {
    const uint16_t *X; // [M][K]     the 1x1 convolution's input pixels (t2)
    const uint16_t *W; // [N][K]
    const uint16_t *R; // [M][N]     residual (the block input) or nullptr
    uint16_t *Y;       // [M][N]
    const float *scale, *shift; // [N]
    int M, N, relu;
    int nslices, nworkers; // grid = nslices * nworkers, nworkers % 8 == 0
    prune_map pm;          // MAP kernels: X is compact ([M = B * Ho * Wo][K]); R and Y are full [B][H][W][N] tensors, row m is pixel prune_map_pixel(pm, m)
};

template <int K, int NS, int MT, bool RES, bool MAP = false>
__global__ __launch_bounds__(256, (K == 256 && MT == 2) ? 3 : 2) void conv_wr_kernel(const wr_args p)
{
    typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    constexpr int KC = K / 64, KF = K / 32; // 128-byte chunks / 32-deep MFMA steps per pixel row
    constexpr int CW = NS / 4, NT = CW / 16; // channels, 16-channel accumulator tiles per wave
    constexpr int PT = 16 * MT;              // pixels per tile (MT 16-pixel accumulator tiles per wave: every wave sees the whole tile)
    constexpr int ABYTES = KC * PT * 128;    // one A image: [KC][PT pixels][128 B], swizzled
    static_assert(NT % 2 == 0 && NT * KF * 4 <= 128 && (MT == 4 || MT == 2), "pairs of accumulator tiles for the lane swap; <= 128 VGPRs of weights");
    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * ABYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, q = lane >> 4;
    // block -> (slice, worker): the slices of a worker on one XCD
    const int xcd = (int)blockIdx.x & 7, rr = (int)blockIdx.x >> 3;
    const int slice = rr % p.nslices, worker = (rr / p.nslices) * 8 + xcd;
    const int n0 = slice * NS + wid * CW; // this wave's first channel
    const int ntiles = (p.M + PT - 1) / PT;
    if (worker >= ntiles) return; // (uniform per workgroup: nobody is left at a barrier)

    // ---- weights: A fragments, once.  Fragment (nt, kf): channel n0 + 16 nt + l15, k = 32 kf + 8 q .. + 7
    u32x4_t wreg[NT][KF]; // (ext-vector type: it can be named as a "+v" asm operand)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) wreg[nt][kf] = *reinterpret_cast<const u32x4_t *>(p.W + (size_t)(n0 + 16 * nt + l15) * K + 32 * kf + 8 * q);
    // (hipcc would otherwise wait for these loads lazily INSIDE the tile loop, with counts that also drain the loop's own requests:
    // one explicit wait here, and the values are opaque from now on)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) asm volatile("" : "+v"(wreg[nt][kf]));
    // ---- epilogue constants: after the lane swap this lane holds channels n0 + 32 i + cbl .. + 7 (i = pair of accumulator tiles)
    const int cbl = (q & 1) * 16 + (q >> 1) * 8;
    float sc[NT / 2][8], sh[NT / 2][8];
#pragma unroll
    for (int i = 0; i < NT / 2; ++i) {
        const int c = n0 + i * 32 + cbl;
        const float4 a0 = *reinterpret_cast<const float4 *>(p.scale + c), a1 = *reinterpret_cast<const float4 *>(p.scale + c + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(p.shift + c), b1 = *reinterpret_cast<const float4 *>(p.shift + c + 4);
        sc[i][0] = a0.x; sc[i][1] = a0.y; sc[i][2] = a0.z; sc[i][3] = a0.w; sc[i][4] = a1.x; sc[i][5] = a1.y; sc[i][6] = a1.z; sc[i][7] = a1.w;
        sh[i][0] = b0.x; sh[i][1] = b0.y; sh[i][2] = b0.z; sh[i][3] = b0.w; sh[i][4] = b1.x; sh[i][5] = b1.y; sh[i][6] = b1.z; sh[i][7] = b1.w;
    }
    // ---- LDS-DMA role: piece j covers tile rows (j * 4 + wid) * 8 + (lane >> 3), physical 16-byte chunk lane & 7 (source-side swizzle)
    const i32x4_t xsrd = bn56_srd(p.X, (unsigned)((size_t)p.M * K * 2));
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem) + wid * 1024);
    int drow[2];
    unsigned dsw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        drow[j] = (j * 4 + wid) * 8 + (lane >> 3);
        dsw[j] = (unsigned)(((lane & 7) ^ ((drow[j] >> 1) & 7)) << 4);
    }
    auto stage = [&](int tile, int buf) {
        unsigned v[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = tile * PT + drow[j];
            v[j] = (tile < ntiles && m < p.M) ? (unsigned)m * (unsigned)(K * 2) + dsw[j] : BN56_OOB; // (a tile past the end: zeros, never read)
        }
        wr_dma<KC, PT>(xsrd, v[0], v[1], lds0 + buf * ABYTES);
    };
    // ---- fragment reads: pixel tile mt, k-step kf: chunk kf >> 1, k-sub kf & 1
    const int fsw = (l15 >> 1) & 7;
    unsigned xoff[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) xoff[s] = (unsigned)(l15 * 128 + ((((4 * s + q) ^ fsw) & 7) << 4));

    typedef uint16_t elem;
    // residual loads and output stores through buffer descriptors: rows beyond M (and tiles beyond the last) are out-of-range lanes -- no
    // branches, the same number of vector-memory operations every tile; hipcc counts these (builtins), the LDS-DMA above it does not
    // (MAP: both descriptors cover the full tensor, whose pixels the rows of this launch are scattered over)
    const size_t ypix = MAP ? (size_t)(p.M / (p.pm.Ho * p.pm.Wo)) * p.pm.H * p.pm.W : (size_t)p.M;
    const __amdgpu_buffer_rsrc_t rsrd = __builtin_amdgcn_make_buffer_rsrc((void *)(RES ? p.R : p.Y), 0, (int)(ypix * p.N * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t ysrd = __builtin_amdgcn_make_buffer_rsrc((void *)p.Y, 0, (int)(ypix * p.N * 2), 0x00020000);
    u32x4_t rv[MT][NT / 2];
    auto row_off = [&](int tile, int mt) -> unsigned { // byte offset of this lane's first chunk of pixel row mt * 16 + l15 of the tile
        const int64_t m = (int64_t)tile * PT + mt * 16 + l15;
        if constexpr (MAP) { // the same offset serves the residual load and the store: pixel (b, sub * oy, sub * ox) of the full tensor
            if (!(tile < ntiles && m < p.M)) return BN56_OOB;
            return (unsigned)((prune_map_pixel(p.pm, (unsigned)m) * p.N + n0 + cbl) * 2);
        }
        return (tile < ntiles && m < p.M) ? (unsigned)((m * p.N + n0 + cbl) * 2) : BN56_OOB;
    };
    auto load_res = [&](int tile) {
        if (!RES) return;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const unsigned o = row_off(tile, mt);
#pragma unroll
            for (int i = 0; i < NT / 2; ++i) rv[mt][i] = __builtin_amdgcn_raw_buffer_load_b128(rsrd, (int)o, i * 64, 0);
        }
    };
    int tile = worker;
    stage(tile, 0);
    stage(tile + p.nworkers, 1);
    load_res(tile);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // both images and the first residual chunks
    for (int it = 0; tile < ntiles; ++it, tile += p.nworkers) {
        const int buf = it & 1;
        __builtin_amdgcn_s_barrier(); // every wave's pieces of this image have landed (each waited for its own before it came here); raw: a
                                      // __syncthreads() would also drain the stores and the requests just issued (vmcnt(0))
        __builtin_amdgcn_sched_barrier(0);
        f32x4 acc[MT][NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const unsigned char *img = smem + buf * ABYTES;
#pragma unroll
        for (int kf = 0; kf < KF; ++kf) {
            uint4 xf[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) xf[mt] = *reinterpret_cast<const uint4 *>(img + (kf >> 1) * (PT * 128) + mt * 2048 + xoff[kf & 1]);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(__builtin_bit_cast(uint4, wreg[nt][kf]), xf[mt], acc[mt][nt]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier(); // the image has been read by every wave: it may be refilled
        // epilogue of this tile; the residual chunks were requested one tile ago
        if (RES) { // this tile's residual chunks (requested a tile ago) and, older than they, this wave's pieces of the NEXT image: one wait
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int i = 0; i < NT / 2; ++i) asm volatile("" : "+v"(rv[mt][i]));
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's pieces of the next image (and the previous tile's stores)
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const unsigned o = row_off(tile, mt);
#pragma unroll
            for (int i = 0; i < NT / 2; ++i) {
                const f32x4 ta = acc[mt][2 * i], tb = acc[mt][2 * i + 1];
                float v[8];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(ta[j]), __float_as_uint(tb[j]), false, false);
                    v[j] = __uint_as_float(r[0]);
                    v[4 + j] = __uint_as_float(r[1]);
                }
                const elem *re = reinterpret_cast<const elem *>(&rv[mt][i]);
                u32x4_t ov;
                elem *oe = reinterpret_cast<elem *>(&ov);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float y = v[e] * sc[i][e] + sh[i][e];
                    if (RES) y += BF16::to_f(re[e]);
                    if (p.relu) y = fmaxf(y, 0.0f);
                    oe[e] = BF16::from_f(y);
                }
                __builtin_amdgcn_raw_buffer_store_b128(ov, ysrd, (int)o, i * 64, 0);
            }
        }
        // the tile after next into the buffer just read; the next tile's residual chunks.  (Their first use -- a tile from now -- waits
        // for everything older, this wave's pieces of the NEXT image included: the barrier at the loop's head then publishes them.)
        stage(tile + 2 * p.nworkers, buf);
        load_res(tile + p.nworkers);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (LDS-DMA of tiles past the end: zeros into LDS nobody reads; drained before the wave ends)
}

template <int K, int NS, int MT>
static void launch_conv_wr_t(hipStream_t strm, const wr_args &w, dim3 grid, bool res)
{
    if (w.pm.sub) { // (the pruned c3 layers: K = 128 / 256 with a residual; the other mapped forms are not instantiated)
        if constexpr (K <= 256 && MT == 4) {
            if (res) hipLaunchKernelGGL((conv_wr_kernel<K, NS, MT, true, true>), grid, dim3(256), 0, strm, w);
            else hipLaunchKernelGGL((conv_wr_kernel<K, NS, MT, false, true>), grid, dim3(256), 0, strm, w);
        }
        return;
    }
    if (res) hipLaunchKernelGGL((conv_wr_kernel<K, NS, MT, true>), grid, dim3(256), 0, strm, w);
    else hipLaunchKernelGGL((conv_wr_kernel<K, NS, MT, false>), grid, dim3(256), 0, strm, w);
}
// c: conv_select's choice (family CONV_WR) for a
static void launch_conv_wr(icl_ctx *ctx, const conv_args &a, const conv_choice &c)
{
    hipStream_t strm = ctx->cur_stream ? ctx->cur_stream : ctx->stream;
    wr_args w;
    w.X = (const uint16_t *)a.X; w.W = (const uint16_t *)a.Wt; w.R = (const uint16_t *)a.R; w.Y = (uint16_t *)a.Y;
    w.scale = a.scale; w.shift = a.shift; w.M = (int)a.M; w.N = a.Cout; w.relu = a.relu;
    w.pm = a.omap;
    w.nslices = c.slices;
    w.nworkers = c.workers;
    const dim3 grid(c.blocks);
    if (c.wr_k == 128) launch_conv_wr_t<128, 256, 4>(strm, w, grid, c.res);
    else if (c.wr_k == 256 && c.wr_mt == 4) launch_conv_wr_t<256, 128, 4>(strm, w, grid, c.res);
    else if (c.wr_k == 256) launch_conv_wr_t<256, 128, 2>(strm, w, grid, c.res);
    else launch_conv_wr_t<512, 128, 2>(strm, w, grid, c.res);
}
