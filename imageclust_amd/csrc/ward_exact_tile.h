// ward_exact_tile.h -- the bit-exact Ward distance tile, stated once: 128 x 128 pairs per workgroup of 256 threads, k-chunks of both
// operands staged in LDS, an 8 x 8 block of accumulators per thread, each accumulator one strictly sequential chain of
// fl(fl(a_k - b_k)^2) (clustering.go:137-141, 152-155).  ward_dist_exact_kernel (ward.hip) and icl_pairs_within's two passes (pairs.hip)
// run it on the lower triangle of one operand, band_select_kernel (band_select.h: nearest.hip, fit.hip) and icl_pairs_between's two
// passes (pairs.hip) on a rectangle of two; ward.hip, the band walk and pairs.hip each keep an epilogue of their own.  Every "bit-equal
// to the oracle" claim of the distance stage rests on the operation order below.
//
// Only units compiled with -ffp-contract=off -fno-slp-vectorize may include this header (the Makefile's rules of ward.o, nearest.o,
// pairs.o and fit.o): every difference, product and sum is rounded on its own, and the packed pairs below are the only packing wanted.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#pragma clang fp contract(off)

#define DT_TILE 128          /* rows of each operand per tile */
#define DT_KC 16             /* k per staged chunk */
#define DT_LD (DT_TILE + 4)  /* pitch of a chunk's k row in LDS */

typedef float dt_f2 __attribute__((ext_vector_type(2)));

// Which row (t = ty) or column (t = tx) of the tile a thread's accumulator index a (0 .. 7) stands for: four neighbours in each half.
__device__ __forceinline__ int dt_lane_index(int a, int t) { return a < 4 ? t * 4 + a : 64 + t * 4 + (a - 4); }

// acc[r][c] = sum over k < d, strictly in k order, of fl(fl(a - b)^2) for the pair of row i0 + dt_lane_index(r, ty) of A [na][d] and row
// j0 + dt_lane_index(c, tx) of B [nb][d], tx = thread & 15, ty = thread >> 4.  Called by all 256 threads of the workgroup (it
// synchronises); As / Bs: DT_KC rows of DT_LD floats each, free for other use on return.  vec: d % 4 == 0 and both operands 16-byte
// aligned (rows are then read 16 bytes at a time).
__device__ __forceinline__ void ward_exact_tile(const float *A, int64_t na, int64_t i0, const float *B, int64_t nb, int64_t j0, int d, bool vec,
                                                float (*As)[DT_LD], float (*Bs)[DT_LD], float (&acc)[8][8])
{
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int lrow = tid >> 2, lk = (tid & 3) * 4; // staging role: 2 rows per operand, 4 consecutive k

#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0.0f;

    // Rows past na / nb and k past d are staged as zeros.  That is harmless ONLY because every accumulator is its own chain (a
    // padded row or column meets nobody else's sum, and the callers' epilogues never store or offer its pairs) and a padded k adds
    // fl((0 - 0)^2) = +0 to a sum that is never below +0: s + 0 == s exactly, NaN and Inf included.
    float ra[2][4], rb[2][4];
    auto gload = [&](int kc) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t ri = i0 + lrow + 64 * h, rj = j0 + lrow + 64 * h;
            const int kk = kc + lk;
#pragma unroll
            for (int q = 0; q < 4; ++q) { ra[h][q] = 0.0f; rb[h][q] = 0.0f; }
            if (ri < na) {
                if (vec && kk + 3 < d) {
                    const float4 v = *reinterpret_cast<const float4 *>(A + ri * d + kk);
                    ra[h][0] = v.x; ra[h][1] = v.y; ra[h][2] = v.z; ra[h][3] = v.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (kk + q < d) ra[h][q] = A[ri * d + kk + q];
                }
            }
            if (rj < nb) {
                if (vec && kk + 3 < d) {
                    const float4 v = *reinterpret_cast<const float4 *>(B + rj * d + kk);
                    rb[h][0] = v.x; rb[h][1] = v.y; rb[h][2] = v.z; rb[h][3] = v.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (kk + q < d) rb[h][q] = B[rj * d + kk + q];
                }
            }
        }
    };

    gload(0);
    for (int kc = 0; kc < d; kc += DT_KC) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                As[lk + q][lrow + 64 * h] = ra[h][q];
                Bs[lk + q][lrow + 64 * h] = rb[h][q];
            }
        __syncthreads();
        if (kc + DT_KC < d) gload(kc + DT_KC);
#pragma unroll
        for (int kk = 0; kk < DT_KC; ++kk) {
            const float4 a0 = *reinterpret_cast<const float4 *>(&As[kk][ty * 4]);
            const float4 a1 = *reinterpret_cast<const float4 *>(&As[kk][64 + ty * 4]);
            const float4 b0 = *reinterpret_cast<const float4 *>(&Bs[kk][tx * 4]);
            const float4 b1 = *reinterpret_cast<const float4 *>(&Bs[kk][64 + tx * 4]);
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int c = 0; c < 8; c += 2) { // two neighbouring chains per packed operation (v_pk_add_f32 / v_pk_mul_f32)
                    const dt_f2 av2 = {av[r], av[r]};
                    const dt_f2 bv2 = {bv[c], bv[c + 1]};
                    dt_f2 s2 = {acc[r][c], acc[r][c + 1]};
                    const dt_f2 df = av2 - bv2; // clustering.go:139
                    const dt_f2 p = df * df;    // :154 product (rounded)
                    s2 = s2 + p;                // :154 sum (rounded), strictly in k order
                    acc[r][c] = s2.x;
                    acc[r][c + 1] = s2.y;
                }
        }
        __syncthreads();
    }
}
