// band_select.h -- the band walk of icl_nearest (nearest.hip) and icl_cluster_fit (fit.hip), stated once: its LDS layout, its kernel
// and the host plan that launches it.
//
// A workgroup owns a BAND of 128 query rows and walks its share of the library's 128-column tiles (ward_exact_tile.h); each row's k best
// (value, j) stay in LDS from the first tile to the last, a finished tile goes through LDS a quarter at a time into them, and nothing
// of size nq x n is ever written.  With few bands and a large library the column tiles are SPLIT over several workgroups per band
// (band_plan.h), each leaves a partial list, and nearest_merge_kernel (nearest.hip) joins them.  What a list keeps and in which order
// is decided by nearest_select.h / fit_select.h alone.  A unit supplies a POLICY, a struct of __device__ __forceinline__ statics with
// exactly what the two walks do differently:
//   args                       band_args and the unit's output pointers behind it
//   band_start(a, split, i0, r)   once per row slot r of the band before the first tile (row i0 + r may lie past nq)
//   items(size)                the item count ward_scale takes for a staged column size
//   row_key(a, i)              what the unit reads per row and quarter before the row's list is touched
//   quarter_key(a, i, key, jb, ncol, sub, srow)   the row's key for the quarter whose first column is jb (its values: sub[srow * BAND_SUB_LD + col])
//   left_out(j, col, key, q_size, size, max_size)   whether column j, the quarter's col-th, is kept from the row's list
//
// The kernel sits at 168 VGPRs, occupancy 3, one register allocation away from occupancy 2 ("Nearest clusters"): the
// __global__ function itself is the template and reads `a.` directly, and the hooks stand where the statements they replace stood.
// Only units compiled with -ffp-contract=off -fno-slp-vectorize may include this header, as ward_exact_tile.h (the Makefile's rules of
// nearest.o and fit.o).
#pragma once
#include "band_plan.h"
#include "icl_common.h"
#include "nearest_select.h"
#include "ward_exact_tile.h" // DT_TILE, DT_KC, DT_LD, ward_exact_tile
#include "ward_value.h"

#pragma clang fp contract(off)

#define BAND_STAGE (2 * DT_KC * DT_LD) // floats of the two operand chunks; the finished tile's quarters reuse them
#define BAND_SUB 64                    // a quarter: 64 rows x 64 columns ...
#define BAND_SUB_LD 65                 // ... at an odd pitch (64 * 65 <= BAND_STAGE): the selecting lanes, one per row, hit distinct banks

static_assert(BAND_SUB * BAND_SUB_LD <= BAND_STAGE, "a quarter tile must fit the operand staging area");
static_assert(NS_KMAX == 64, "the LDS budget below is worked out for k <= 64");

// What every walk receives, in the order the kernels have always received it; a unit's args add its output pointers behind.
struct band_args {
    const float *Q, *E;
    const int32_t *qs, *es, *sel; // device copies of the row sizes, the column sizes (either may be null: all 1) and the unit's per-row selector
    int64_t nq, n;
    int d, k, max_size, vec;
    int64_t ntiles, nbands;
    int splits;
};

// floats of dynamic LDS: operand chunks, the band's lists (pitch k | 1: a row per lane, distinct banks), per-row counts, the band's
// row sizes, the tile's column sizes.  k = 64: 84 992 bytes of the 160 KiB.
static inline size_t band_lds_bytes(int k) { return (size_t)(BAND_STAGE + 2 * DT_TILE * (k | 1) + 3 * DT_TILE) * 4; }

// a.val / a.idx: [splits][nq][k], the result itself when splits == 1, else the partial lists
template <class P> static __global__ __launch_bounds__(256) void band_select_kernel(typename P::args a)
{
    extern __shared__ __attribute__((aligned(16))) float band_smem[];
    float(*As)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(band_smem);
    float(*Bs)[DT_LD] = reinterpret_cast<float(*)[DT_LD]>(band_smem + DT_KC * DT_LD);
    float *sub = band_smem;
    const int k = a.k, ks = a.k | 1;
    float *lv = band_smem + BAND_STAGE;
    int32_t *lj = reinterpret_cast<int32_t *>(lv + DT_TILE * ks);
    int32_t *cnt = lj + DT_TILE * ks;
    int32_t *qsz = cnt + DT_TILE;
    int32_t *esz = qsz + DT_TILE;

    // workgroups of one split are neighbours: the bands that run together read the same library tiles at about the same time
    const int64_t band = (int64_t)blockIdx.x % a.nbands, split = (int64_t)blockIdx.x / a.nbands;
    const int64_t t_lo = split * a.ntiles / a.splits, t_hi = (split + 1) * a.ntiles / a.splits;
    const int64_t i0 = band * DT_TILE;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;

    if (tid < DT_TILE) {
        cnt[tid] = 0;
        qsz[tid] = (a.qs && i0 + tid < a.nq) ? a.qs[i0 + tid] : 1;
        P::band_start(a, split, i0, tid);
    }
    __syncthreads();

    for (int64_t t = t_lo; t < t_hi; ++t) {
        const int64_t j0 = t * DT_TILE;
        if (tid < DT_TILE) esz[tid] = (a.es && j0 + tid < a.n) ? a.es[j0 + tid] : 1; // (read after the tile's barriers)

        float acc[8][8];
        ward_exact_tile(a.Q, a.nq, i0, a.E, a.n, j0, a.d, a.vec != 0, As, Bs, acc);

        // The finished tile, a quarter at a time: every thread scales its 4 x 4 values of the quarter (clustering.go:142-144) into the
        // staging area, then one lane per row offers the row's 64 values to the row's list.  The selecting lanes are every fourth
        // thread, so all four waves (SIMDs) take a share; the selection holds a handful of registers while acc stays live.
#pragma unroll
        for (int ah = 0; ah < 2; ++ah)
#pragma unroll
            for (int bh = 0; bh < 2; ++bh) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int sa = qsz[ah * 64 + ty * 4 + r];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        sub[(ty * 4 + r) * BAND_SUB_LD + tx * 4 + c] =
                            ward_scale(acc[ah * 4 + r][bh * 4 + c], sa, P::items(esz[bh * 64 + tx * 4 + c]));
                }
                __syncthreads();
                if ((tid & 3) == 0) {
                    const int row = ah * 64 + (tid >> 2);
                    const int64_t i = i0 + row;
                    if (i < a.nq) {
                        const auto rkey = P::row_key(a, i);
                        const int sq = qsz[row];
                        float *rv = lv + row * ks;
                        int32_t *rj = lj + row * ks;
                        int c = cnt[row];
                        const int64_t jb = j0 + bh * 64;
                        const int ncol = (int)(a.n - jb < BAND_SUB ? (a.n - jb > 0 ? a.n - jb : 0) : BAND_SUB);
                        const auto key = P::quarter_key(a, i, rkey, jb, ncol, sub, tid >> 2);
                        for (int col = 0; col < ncol; ++col) {
                            if (P::left_out(jb + col, col, key, sq, esz[bh * 64 + col], a.max_size)) continue;
                            ns_insert(rv, rj, k, c, sub[(tid >> 2) * BAND_SUB_LD + col], (int32_t)(jb + col));
                        }
                        cnt[row] = c;
                    }
                }
                __syncthreads();
            }
    }

    // the band's lists, short rows with their tails
    float *ov = a.val + (split * a.nq + i0) * k;
    int32_t *oj = a.idx + (split * a.nq + i0) * k;
    const int rows = (int)(a.nq - i0 < DT_TILE ? a.nq - i0 : DT_TILE);
    for (int e = tid; e < rows * k; e += 256) {
        const int row = e / k, p = e - row * k;
        const bool have = p < cnt[row];
        ov[e] = have ? lv[row * ks + p] : NS_MAXF;
        oj[e] = have ? lj[row * ks + p] : -1;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// One walk's geometry and its launch.  decide() before the caller lays out its workspace (two partial arrays of part_bytes each),
// run() once the caller's arrays are up and a's operands, sizes, selector, nq, n, d, k, max_size and own outputs are filled in.
// Both expect ctx->mu held and the device selected.
struct band_plan {
    int64_t nbands = 0, ntiles = 0;
    int splits = 0;        // (icl_set_nearest_options governs every walk)
    size_t part_bytes = 0; // of the partial values, and as many of the partial indices: 0 with one split

    int decide(icl_ctx *ctx, const char *what, int64_t nq, int64_t n, int k)
    {
        nbands = icl_ceil_div(nq, DT_TILE);
        ntiles = icl_ceil_div(n, DT_TILE);
        splits = band_splits(ctx->nearest_splits, ctx->prop.multiProcessorCount, nbands, ntiles);
        if (nbands * splits > 0x7fffffffLL) return icl_fail(ctx, ICL_ERR_UNSUPPORTED, "%s: grid too large (nq=%lld)", what, (long long)nq);
        part_bytes = splits > 1 ? (size_t)splits * nq * k * 4 : 0;
        return ICL_OK;
    }

    // The walk into d_val / d_idx [nq][k], through the partial lists and the merge when there are splits.
    template <class P> int run(icl_ctx *ctx, typename P::args &a, float *part_val, int32_t *part_idx, float *d_val, int32_t *d_idx) const
    {
        a.vec = (a.d & 3) == 0 && (((uintptr_t)a.Q | (uintptr_t)a.E) & 15) == 0;
        a.ntiles = ntiles;
        a.nbands = nbands;
        a.splits = splits;
        a.val = splits > 1 ? part_val : d_val;
        a.idx = splits > 1 ? part_idx : d_idx;
        icl_lds_optin(ctx, (const void *)band_select_kernel<P>, (int)band_lds_bytes(NS_KMAX));
        hipLaunchKernelGGL(band_select_kernel<P>, dim3((unsigned)(nbands * splits)), dim3(256), band_lds_bytes(a.k), ctx->stream, a);
        ICL_HIP(ctx, hipGetLastError());
        if (splits > 1) ICL_TRY(nearest_merge_launch(ctx, a.val, a.idx, a.nq, a.k, splits, d_val, d_idx));
        return ICL_OK;
    }
};
