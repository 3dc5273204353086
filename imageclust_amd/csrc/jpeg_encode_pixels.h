// jpeg_encode_pixels.h -- the integer rules of the JPEG encoder, shared by the host encoder (jpeg_encode.hip) and the GPU encoder
// (jpeg_encode_gpu.hip).  Both call these functions, so their files agree byte for byte by construction.  The target is what libjpeg
// (-turbo) writes after jpeg_set_defaults + jpeg_set_quality(q, TRUE): baseline SOF0, YCbCr 4:2:0, the Annex K Huffman tables, no
// restart interval, the islow forward DCT.  From jccolor.c (rgb_ycc_convert), jcsample.c (h2v2_downsample, the edge expansion of
// jcprepct.c), jccoefct.c (dummy blocks), jfdctint.c, jcdctmgr.c (quantisation) and jchuff.c (encode_one_block).
// Integer arithmetic only, no allocation: everything here is __host__ __device__.
#pragma once
#include "ingest_pixels.h"

constexpr int ICL_JENC_HEADER = 623; // SOI, APP0, 2 x DQT, SOF0, 4 x DHT, SOS
constexpr int ICL_JENC_BLOCK_BITS = 64 * 27; // a coefficient costs at most a 16-bit code + 11 amplitude bits; ZRL and EOB stand for zeros
enum { ICL_JENC_DC0 = 0, ICL_JENC_AC0 = 1, ICL_JENC_DC1 = 2, ICL_JENC_AC1 = 3 };

// what one quality setting fixes: the two quantisation tables (natural order) and the codes of the four Huffman tables
struct icl_jenc_tables {
    uint16_t qt[2][64];
    uint16_t code[4][256];
    uint8_t size[4][256];
};

// the geometry of one 4:2:0 frame
struct icl_jenc_geom {
    int32_t W, H;
    int32_t mw, mh; // MCUs (16 x 16 pixels) per row, rows of MCUs
    int32_t wb, hb; // real luma block columns / rows: ceil(W / 8), ceil(H / 8); the blocks beyond them are dummies
    int32_t ch;     // real chroma rows: ceil(H / 2)
};
ICL_PX icl_jenc_geom icl_jenc_geometry(int W, int H)
{
    icl_jenc_geom g;
    g.W = W;
    g.H = H;
    g.mw = (W + 15) >> 4;
    g.mh = (H + 15) >> 4;
    g.wb = (W + 7) >> 3;
    g.hb = (H + 7) >> 3;
    g.ch = (H + 1) >> 1;
    return g;
}

// ---- jccolor.c rgb_ycc_convert: 16-bit fixed point; Cb and Cr carry (128 << 16) + 32767 ----
ICL_PX int icl_jenc_y(int R, int G, int B) { return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16; }
ICL_PX int icl_jenc_cb(int R, int G, int B) { return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16; }
ICL_PX int icl_jenc_cr(int R, int G, int B) { return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16; }

// Block k of an MCU in scan order: 0..3 luma (Y00 Y01 Y10 Y11), 4 Cb, 5 Cr.  A luma block beyond the real block columns / rows is a
// dummy of the coefficient controller: zero AC, the DC of the block before it in scan order (so its DC difference is 0).
ICL_PX bool icl_jenc_is_dummy(const icl_jenc_geom &g, int mx, int my, int k)
{
    return k < 4 && (2 * mx + (k & 1) >= g.wb || 2 * my + (k >> 1) >= g.hb);
}

// The 64 centred samples of a real block.  Luma: the right edge is replicated per row and the last row downwards.  Chroma: the
// pixel row is replicated to the right, rows H.. repeat row H - 1 up to an even count, h2v2_downsample averages 2 x 2 with the bias
// alternating 1, 2 along the row, and chroma rows beyond ceil(H / 2) repeat the last chroma row (not a downsampled padded pixel row).
ICL_PX void icl_jenc_block_samples(const uint8_t *rgb, const icl_jenc_geom &g, int mx, int my, int k, int s[64])
{
    const int W = g.W, H = g.H;
    if (k < 4) {
        const int x0 = (2 * mx + (k & 1)) * 8, y0 = (2 * my + (k >> 1)) * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = y0 + r < H - 1 ? y0 + r : H - 1;
            const uint8_t *row = rgb + (int64_t)y * W * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int x = x0 + c < W - 1 ? x0 + c : W - 1;
                const uint8_t *p = row + (int64_t)x * 3;
                s[r * 8 + c] = icl_jenc_y(p[0], p[1], p[2]) - 128;
            }
        }
        return;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int cy = my * 8 + r < g.ch - 1 ? my * 8 + r : g.ch - 1;
        const int ya = 2 * cy < H - 1 ? 2 * cy : H - 1, yb = 2 * cy + 1 < H - 1 ? 2 * cy + 1 : H - 1;
        const uint8_t *ra = rgb + (int64_t)ya * W * 3, *rb = rgb + (int64_t)yb * W * 3;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int cx = mx * 8 + c;
            const int xa = 2 * cx < W - 1 ? 2 * cx : W - 1, xb = 2 * cx + 1 < W - 1 ? 2 * cx + 1 : W - 1;
            const uint8_t *p0 = ra + (int64_t)xa * 3, *p1 = ra + (int64_t)xb * 3, *p2 = rb + (int64_t)xa * 3, *p3 = rb + (int64_t)xb * 3;
            int sum;
            if (k == 4) sum = icl_jenc_cb(p0[0], p0[1], p0[2]) + icl_jenc_cb(p1[0], p1[1], p1[2]) + icl_jenc_cb(p2[0], p2[1], p2[2]) + icl_jenc_cb(p3[0], p3[1], p3[2]);
            else sum = icl_jenc_cr(p0[0], p0[1], p0[2]) + icl_jenc_cr(p1[0], p1[1], p1[2]) + icl_jenc_cr(p2[0], p2[1], p2[2]) + icl_jenc_cr(p3[0], p3[1], p3[2]);
            s[r * 8 + c] = ((sum + 1 + (cx & 1)) >> 2) - 128;
        }
    }
}

// ---- jfdctint.c jpeg_fdct_islow: CONST_BITS 13, PASS1_BITS 2 ----
ICL_PX int icl_fdct_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass over d[0], d[s], .. d[7 * s]: the first pass (rows) leaves its results scaled up by 2^PASS1_BITS, the second
// (columns) removes that scaling again
template <bool FIRST> ICL_PX void icl_fdct_islow_1d(int *d, int s)
{
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                  F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    constexpr int CB = ICL_IDCT_CB, P1 = ICL_IDCT_P1, SH = FIRST ? CB - P1 : CB + P1;
    const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s], tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
    const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s], tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) * (1 << P1);
        d[4 * s] = (tmp10 - tmp11) * (1 << P1);
    } else {
        d[0] = icl_fdct_descale(tmp10 + tmp11, P1);
        d[4 * s] = icl_fdct_descale(tmp10 - tmp11, P1);
    }
    int z1 = (tmp12 + tmp13) * F0_541;
    d[2 * s] = icl_fdct_descale(z1 + tmp13 * F0_765, SH);
    d[6 * s] = icl_fdct_descale(z1 + tmp12 * (-F1_847), SH);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F1_175;
    const int t4 = tmp4 * F0_298, t5 = tmp5 * F2_053, t6 = tmp6 * F3_072, t7 = tmp7 * F1_501;
    z1 *= -F0_899;
    z2 *= -F2_562;
    z3 *= -F1_961;
    z4 *= -F0_390;
    z3 += z5;
    z4 += z5;
    d[7 * s] = icl_fdct_descale(t4 + z1 + z3, SH);
    d[5 * s] = icl_fdct_descale(t5 + z2 + z4, SH);
    d[3 * s] = icl_fdct_descale(t6 + z2 + z3, SH);
    d[s] = icl_fdct_descale(t7 + z1 + z4, SH);
}

ICL_PX void icl_fdct_islow(int s[64])
{
#pragma unroll
    for (int r = 0; r < 8; ++r) icl_fdct_islow_1d<true>(s + 8 * r, 1);
#pragma unroll
    for (int c = 0; c < 8; ++c) icl_fdct_islow_1d<false>(s + c, 8);
}

// jcdctmgr.c: the islow divisor is 8 * q (the DCT's output is scaled up by 8); sign-magnitude rounding
ICL_PX int icl_jenc_quantize(int c, int q)
{
    const int q8 = q << 3;
    return c < 0 ? -((-c + (q8 >> 1)) / q8) : (c + (q8 >> 1)) / q8;
}

// samples -> the block's 64 quantised coefficients in zig-zag order
ICL_PX void icl_jenc_block_coefs(int s[64], const uint16_t *qt, int16_t *zz)
{
    icl_fdct_islow(s);
#pragma unroll
    for (int k = 0; k < 64; ++k) zz[k] = (int16_t)icl_jenc_quantize(s[icl_zigzag[k]], qt[icl_zigzag[k]]);
}

// ---- jchuff.c encode_one_block: sink.put(value, nbits), nbits <= 16, the most significant bit first ----
ICL_PX int icl_jenc_nbits(int v)
{
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}
template <class Coef, class Sink>
ICL_PX void icl_jenc_encode_block(const Coef &zz, int dc_diff, const icl_jenc_tables &T, int dc_tbl, int ac_tbl, Sink &sink)
{
    int t = dc_diff, t2 = dc_diff;
    if (t < 0) { t = -t; --t2; }
    int nb = icl_jenc_nbits(t);
    sink.put(T.code[dc_tbl][nb], T.size[dc_tbl][nb]);
    if (nb) sink.put((uint32_t)t2 & ((1u << nb) - 1), nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        t = zz(k);
        if (t == 0) { ++run; continue; }
        while (run > 15) {
            sink.put(T.code[ac_tbl][0xF0], T.size[ac_tbl][0xF0]);
            run -= 16;
        }
        t2 = t;
        if (t < 0) { t = -t; --t2; }
        nb = icl_jenc_nbits(t);
        const int sym = (run << 4) + nb;
        sink.put(T.code[ac_tbl][sym], T.size[ac_tbl][sym]);
        sink.put((uint32_t)t2 & ((1u << nb) - 1), nb);
        run = 0;
    }
    if (run > 0) sink.put(T.code[ac_tbl][0], T.size[ac_tbl][0]);
}
struct icl_jenc_count_sink { // the coded length of a block
    uint32_t bits = 0;
    ICL_PX void put(uint32_t, int n) { bits += (uint32_t)n; }
};

// Where the DC prediction of block k of MCU m comes from: the previous block of the same component in scan order (block index
// within the image's 6-per-MCU list), or -1 at the start of the scan.  A dummy's own DC is that of its predecessor.
ICL_PX int64_t icl_jenc_dc_pred_block(int64_t m, int k)
{
    if (k == 0) return m == 0 ? -1 : (m - 1) * 6 + 3;
    if (k < 4) return m * 6 + k - 1;
    return m == 0 ? -1 : (m - 1) * 6 + k;
}

// host only (jpeg_encode.hip): tables of a quality 1..100, the 623-byte header of a w x h file
void icl_jenc_make_tables(int quality, icl_jenc_tables &T);
void icl_jenc_write_header(const icl_jenc_tables &T, int w, int h, uint8_t *out);
