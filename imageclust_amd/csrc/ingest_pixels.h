// ingest_pixels.h -- the integer pixel rules of image ingest, shared by the host path (jpeg_decode.hip stage B, image_io.hip)
// and the GPU rebuild of the batched file path (jpeg_gpu.hip).  Both paths call these functions, so their outputs agree byte for
// byte by construction: libjpeg-turbo's islow IDCT (jidctint.c), "fancy" chroma upsampling (jdsample.c) and fixed-point
// YCbCr->RGB (jdcolor.c), OpenCV's EXIF transform, and cv::resize's 8-bit INTER_LINEAR rounding with its INTER_AREA switch.
// Integer arithmetic only, no allocation: everything here is __host__ __device__.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define ICL_PX __host__ __device__ __forceinline__

// natural-order index of the k-th coefficient of a block in zig-zag order (T.81 figure A.6)
inline constexpr uint8_t icl_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

ICL_PX int icl_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- IJG jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2 ----
constexpr int ICL_IDCT_CB = 13, ICL_IDCT_P1 = 2;

ICL_PX int icl_idct_descale(long x, int n) { return (int)((x + (1L << (n - 1))) >> n); }

// the 8-point transform of both passes: x[0], x[s], .. x[7 * s] -> o[0..7], scaled by 2^CONST_BITS (not yet descaled)
ICL_PX void icl_idct_islow_1d(const int *x, int s, long o[8])
{
    constexpr long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                   F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    // even part
    long z2 = x[2 * s], z3 = x[6 * s];
    long z1 = (z2 + z3) * F0_541;
    long tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
    z2 = x[0];
    z3 = x[4 * s];
    long tmp0 = (z2 + z3) * (1L << ICL_IDCT_CB), tmp1 = (z2 - z3) * (1L << ICL_IDCT_CB);
    const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    tmp0 = x[7 * s];
    tmp1 = x[5 * s];
    tmp2 = x[3 * s];
    tmp3 = x[s];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    long z4 = tmp1 + tmp3;
    const long z5 = (z3 + z4) * F1_175;
    tmp0 *= F0_298;
    tmp1 *= F2_053;
    tmp2 *= F3_072;
    tmp3 *= F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3;
    o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2;
    o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1;
    o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0;
    o[4] = tmp13 - tmp0;
}

// pass 1 on one column: in[8 * r] are its dequantised coefficients (natural order), w[8 * r] receives the workspace column.
// (For a column whose AC terms are all zero this gives in[0] << PASS1_BITS in every row: jidctint.c's shortcut.)
ICL_PX void icl_idct_islow_col(const int *in, int *w)
{
    long o[8];
    icl_idct_islow_1d(in, 8, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[8 * r] = icl_idct_descale(o[r], ICL_IDCT_CB - ICL_IDCT_P1);
}

// pass 2 on one row w[0..7] of the workspace: the row's 8 samples.  range_limit[x & RANGE_MASK] of libjpeg == clamp(x + 128)
// for every value a legal stream can produce.
ICL_PX void icl_idct_islow_row(const int *w, int px[8])
{
    long o[8];
    icl_idct_islow_1d(w, 1, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) px[k] = icl_clamp8(icl_idct_descale(o[k], ICL_IDCT_CB + ICL_IDCT_P1 + 3) + 128);
}

// ---- jdsample.c chroma upsampling with libjpeg's default settings: "fancy" (triangle) filters 2x horizontally (h2v1), 2x both ways
// (h2v2) and 2x vertically (h1v2); plain replication (int_upsample) for every other factor, of which 4x1 and 1x4 are decoded ----
// the luma sampling factors (chroma 1x1) these rules cover: 4:4:4, 4:2:2, 4:2:0, 4:4:0 (1x2) and 4:1:1 (4x1, or 1x4 after a rotation)
ICL_PX bool icl_luma_sampling_ok(int hs, int vs)
{
    return (hs == 1 && (vs == 1 || vs == 2 || vs == 4)) || (hs == 2 && (vs == 1 || vs == 2)) || (hs == 4 && vs == 1);
}
// the nearer and the further input row of output row y for h2v2 and h1v2: y / 2, and the row above it (even y) or below it (odd y);
// rows above the first and below the last repeat the edge row
ICL_PX void icl_fancy_rows(int y, int dh, int &nearer, int &further)
{
    auto cl = [&](int r) { return r < 0 ? 0 : (r > dh - 1 ? dh - 1 : r); };
    const int r = y >> 1;
    nearer = cl(r);
    further = cl((y & 1) ? r + 1 : r - 1);
}
// h2v2 works on column sums of the two rows
ICL_PX int icl_fancy_colsum(int nearer, int further) { return nearer * 3 + further; }

// Sample X of a row upsampled 2x horizontally from dw input columns col(0) .. col(dw - 1): the samples of the input row (VS 1,
// h2v1) or its column sums (VS 2, h2v2).  Sample 2i + odd is a 3:1 blend of column i and its neighbour on that side (i - 1 or
// i + 1); at either end of the row (both ends when dw == 1) the edge column is its own neighbour, which gives libjpeg's edge
// formulas.
template <int VS, class Col>
ICL_PX int icl_fancy_h2(const Col &col, int dw, int X)
{
    auto blend = [](int c, int n, int odd) { return VS == 1 ? (c * 3 + n + 1 + odd) >> 2 : (c * 3 + n + 8 - odd) >> 4; };
    const int i = (X >> 1) < dw - 1 ? (X >> 1) : dw - 1;
    if (X & 1) return i >= dw - 1 ? blend(col(dw - 1), col(dw - 1), 1) : blend(col(i), col(i + 1), 1);
    return i == 0 ? blend(col(0), col(0), 0) : blend(col(i), col(i - 1), 0);
}

// h1v2: a 3:1 blend of the two rows with no horizontal filter; the bias is 1 in the upper (even y) and 2 in the lower row of a pair
ICL_PX int icl_fancy_v2(int nearer, int further, int y) { return (nearer * 3 + further + 1 + (y & 1)) >> 2; }

// Sample (X, y) of the full-resolution plane, from a chroma plane of dw x dh samples whose row r starts at pl + r * stride;
// hs x vs is the luma's sampling factor (icl_luma_sampling_ok): 1x1 (no upsampling), 2x1 (h2v1), 2x2 (h2v2), 1x2 (h1v2), or 4x1 /
// 1x4 (int_upsample: chroma sample (X / 4, y) or (X, y / 4), neither direction smoothed).
ICL_PX int icl_fancy_upsample(const uint8_t *pl, int64_t stride, int dw, int dh, int hs, int vs, int X, int y)
{
    auto row = [&](int r) { return pl + (int64_t)(r < 0 ? 0 : (r > dh - 1 ? dh - 1 : r)) * stride; };
    auto colx = [&](int x) { return x < dw - 1 ? x : dw - 1; };
    if (hs == 2 && vs == 1) {
        const uint8_t *p = row(y);
        return icl_fancy_h2<1>([&](int k) { return (int)p[k]; }, dw, X);
    }
    if (vs == 2) {
        int r0, r1;
        icl_fancy_rows(y, dh, r0, r1);
        const uint8_t *p0 = row(r0), *p1 = row(r1);
        if (hs == 1) return icl_fancy_v2(p0[colx(X)], p1[colx(X)], y);
        return icl_fancy_h2<2>([&](int k) { return icl_fancy_colsum(p0[k], p1[k]); }, dw, X);
    }
    return row(vs == 4 ? y >> 2 : y)[colx(hs == 4 ? X >> 2 : X)]; // 1x1, 4x1, 1x4
}

// ---- jdcolor.c ycc_rgb_convert: fixed-point YCbCr -> RGB (the products of its four tables, evaluated in place) ----
ICL_PX void icl_ycc_to_rgb(int Y, int cb, int cr, int &R, int &G, int &B)
{
    const int xr = cr - 128, xb = cb - 128;
    R = icl_clamp8(Y + ((91881 * xr + 32768) >> 16));               // FIX(1.40200)
    G = icl_clamp8(Y + ((-22554 * xb + 32768 + -46802 * xr) >> 16)); // FIX(0.34414), FIX(0.71414)
    B = icl_clamp8(Y + ((116130 * xb + 32768) >> 16));               // FIX(1.77200)
}

// ---- cv::imread's EXIF transform (OpenCV ExifTransform): 2 mirror horizontally, 3 rotate 180, 4 mirror vertically, 5 transpose,
// 6 rotate 90 clockwise, 7 transverse, 8 rotate 90 counter-clockwise; 5..8 swap the axes ----
ICL_PX bool icl_exif_swaps_axes(int orient) { return orient >= 5 && orient <= 8; }
// the source pixel (sx, sy) of pixel (x, y) of the oriented image, for a decoded image of sw x sh (any other orient: identity)
ICL_PX void icl_exif_source(int orient, int sw, int sh, int x, int y, int &sx, int &sy)
{
    switch (orient) {
    case 2: sx = sw - 1 - x; sy = y; break;
    case 3: sx = sw - 1 - x; sy = sh - 1 - y; break;
    case 4: sx = x; sy = sh - 1 - y; break;
    case 5: sx = y; sy = x; break;
    case 6: sx = y; sy = sh - 1 - x; break;
    case 7: sx = sw - 1 - y; sy = sh - 1 - x; break;
    case 8: sx = sw - 1 - y; sy = x; break;
    default: sx = x; sy = y; break;
    }
}

// ---- cv::resize on 8-bit data ----
// cv::resize switches INTER_LINEAR to INTER_AREA for an exact 2x2 decimation ("if (interpolation == INTER_LINEAR && is_area_fast &&
// iscale_x == 2 && iscale_y == 2) interpolation = INTER_AREA"); ResizeAreaFast on 8-bit data is the rounded mean of the 2x2 block
ICL_PX bool icl_resize_is_area(int sw, int sh, int dw, int dh) { return sw == 2 * dw && sh == 2 * dh; }
ICL_PX uint8_t icl_area_mean(int a, int b, int c, int d) { return (uint8_t)((a + b + c + d + 2) >> 2); }

// INTER_LINEAR with 11-bit weights: the two-pass rounding of OpenCV's HResizeLinear / VResizeLinear<uchar> on the 2x2 taps
// t00 t01 (source row sy) / t10 t11 (row sy + 1), horizontal weights a0 a1, vertical weights b0 b1
ICL_PX uint8_t icl_resize_linear(int t00, int t01, int t10, int t11, int a0, int a1, int b0, int b1)
{
    const int row0 = t00 * a0 + t01 * a1, row1 = t10 * a0 + t11 * a1;
    return (uint8_t)((((b0 * (row0 >> 4)) >> 16) + ((b1 * (row1 >> 4)) >> 16) + 2) >> 2);
}
