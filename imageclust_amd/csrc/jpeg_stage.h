// jpeg_stage.h -- the two stages of the host JPEG decoder (jpeg_decode.hip) and the GPU rebuild of stage B (jpeg_gpu.hip).
//
// Stage A parses the file and runs the entropy decoder: what it leaves is everything the pixel rebuild needs.  Stage B is
// the integer pixel work: dequantisation, the islow IDCT, fancy chroma upsampling and the YCbCr->RGB conversion.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "icl_common.h"

#define ICL_JPEG_MAX_PIXELS (64LL << 20)

struct icl_jpeg_component {
    int id = 0, h = 1, v = 1, tq = 0;
    int wblocks = 0, hblocks = 0; // padded to whole MCUs
    int dw = 0, dh = 0;           // downsampled_width / _height (real samples)
    std::vector<int16_t> coefs;   // wblocks*hblocks blocks of 64, natural order, NOT dequantised
    void swap_from(icl_jpeg_component &o)
    {
        id = o.id; h = o.h; v = o.v; tq = o.tq;
        wblocks = o.wblocks; hblocks = o.hblocks; dw = o.dw; dh = o.dh;
        coefs.swap(o.coefs);
    }
};

struct icl_jpeg_coefs {
    int W = 0, H = 0, ncomp = 0;
    int orient = 1;       // EXIF orientation 1..8
    bool is_rgb = false;  // Adobe transform 0, or component ids 'R' 'G' 'B' without an Adobe marker: no colour conversion
    uint16_t qt[3][64];   // each component's quantisation table, natural order, as it stood after the last scan
    icl_jpeg_component comp[3];
};

// Stage A.  Every check of a hostile file is made here; on success J holds a decodable image (1 or 3 components,
// 4:4:4 / 4:2:2 / 4:2:0, at most ICL_JPEG_MAX_PIXELS).  J may be reused across calls (its coefficient arrays keep their capacity).
int icl_jpeg_stage_a(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, icl_jpeg_coefs &J);
// Stage B on the host: interleaved RGB, W*H*3 (before the EXIF orientation).
int icl_jpeg_stage_b(icl_ctx *ctx, const icl_jpeg_coefs &J, const char *path, std::vector<uint8_t> &rgb);

// resnet.hip: the host ingest path the batched file pipeline falls back to, and the resize tables it shares with the GPU
int icl_read_image_host(icl_ctx *ctx, const char *path, std::vector<uint8_t> &rgb, int &w, int &h);
void icl_apply_exif_orientation(std::vector<uint8_t> &rgb, int &w, int &h, int orient);
void icl_resize_u8_host(const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh);
void icl_resize_coeffs(int dn, int sn, int32_t *ofs, int16_t *al); // cv::resize INTER_LINEAR source offsets + 11-bit weights
