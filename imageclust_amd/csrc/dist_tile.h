// dist_tile.h -- which tile of the lower triangle a workgroup of a distance kernel takes, and how many tiles a launch has: the one
// definition behind ward_dist_exact_kernel (ward.hip), dist_mfma_kernel / dist_bound_kernel (distance_mfma.hip) and
// dist_bound_i8_kernel (distance_i8.hip) and their launchers.  Integer results only, no HIP type: a plain host C++ compile can
// include it, and tests/dist_tile_main.cpp checks every rule below on the CPU.
//
// The header is included by units compiled with -ffp-contract=off (ward.hip) and without (distance_mfma.hip, distance_i8.hip).  The
// only floating-point in it is the sqrt GUESS of a band or row index, and the integer loops behind each guess move it to the one
// index that satisfies the integer conditions: whether the guess's expression is contracted or not cannot show in a result.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DTILE_HD __host__ __device__ __forceinline__
#else
#define DTILE_HD inline
#endif

// Tiles of the tile rows [tr_lo, tr_hi) (tile row ti holds the tiles tj = 0 .. ti), or -1 where that many do not fit a launch's grid.
inline int64_t tri_tile_count(int64_t tr_lo, int64_t tr_hi)
{
    const int64_t nblocks = tr_hi * (tr_hi + 1) / 2 - tr_lo * (tr_lo + 1) / 2;
    return nblocks > 0x7fffffffLL ? -1 : nblocks;
}

// Row-major order of the whole triangle: tile b is (ti, tj) with b = ti (ti + 1) / 2 + tj.
DTILE_HD void tri_decode32(int64_t b, int &ti, int &tj)
{
    int64_t t = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while ((t + 1) * (t + 2) / 2 <= b) ++t;
    while (t * (t + 1) / 2 > b) --t;
    ti = (int)t;
    tj = (int)(b - t * (t + 1) / 2);
}

// Tile order of a launch over tile rows [tr_lo, tr_hi): BANDS of 8 tile rows; inside a band the tiles left of the band's first
// diagonal tile go column by column -- 8 consecutive tiles share one row panel of the operand as their column operand, consecutive
// columns share the band's 8 row panels -- then the band's triangular cap.  With the XCD-aware dealing (mfma_tile.h, xcd_remap: each
// XCD takes a contiguous run of this order), the ~100 tiles an XCD runs at a time touch ~20 panels instead of ~100 (the kernels stream
// k-chunks, so tiles that run together read the same cache lines at about the same time): the row-major order fetched 21x the
// algorithmic bytes at N = 100 000 (profiles/r02c_pmc_traffic.json).
DTILE_HD void tri_band_decode(int64_t b, int64_t tr_lo, int64_t tr_hi, int &ti, int &tj)
{
    auto before = [&](int64_t q) { return 32 * q * q + q * (8 * tr_lo + 4); }; // tiles of the bands in front of band q
    const double c1 = 8.0 * (double)tr_lo + 4.0;
    int64_t q = (int64_t)((-c1 + sqrt(c1 * c1 + 128.0 * (double)b)) / 64.0);
    while (before(q + 1) <= b) ++q;
    while (q > 0 && before(q) > b) --q;
    const int64_t r0 = tr_lo + 8 * q;
    const int64_t h = tr_hi - r0 < 8 ? tr_hi - r0 : 8;
    int64_t r = b - before(q);
    const int64_t rect = h * (r0 + 1);
    if (r < rect) {
        tj = (int)(r / h);
        ti = (int)(r0 + r % h);
        return;
    }
    r -= rect; // the cap: row r0 + a holds the columns r0 + 1 .. r0 + a
    int a = 1;
    while ((int64_t)a * (a + 1) / 2 <= r) ++a;
    ti = (int)(r0 + a);
    tj = (int)(r0 + 1 + (r - (int64_t)a * (a - 1) / 2));
}
