// jpeg_stage.h -- the two stages of the host JPEG decoder (jpeg_decode.hip), the GPU rebuild of stage B (jpeg_gpu.hip) and the
// host ingest path around them (image_io.hip).
//
// Stage A parses the file and runs the entropy decoder: what it leaves is everything the pixel rebuild needs.  Stage B is
// the integer pixel work: dequantisation, the islow IDCT, fancy chroma upsampling and the YCbCr->RGB conversion (ingest_pixels.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "icl_common.h"
#include "jpeg_entropy.h"

#define ICL_JPEG_MAX_PIXELS (64LL << 20)

struct icl_jpeg_component {
    int id = 0, h = 1, v = 1, tq = 0;
    int wblocks = 0, hblocks = 0; // padded to whole MCUs
    int dw = 0, dh = 0;           // downsampled_width / _height (real samples)
    std::vector<int16_t> coefs;   // wblocks*hblocks blocks of 64, natural order, NOT dequantised
};

struct icl_jpeg_coefs {
    int W = 0, H = 0, ncomp = 0;
    int orient = 1;       // EXIF orientation 1..8
    bool is_rgb = false;  // Adobe transform 0, or component ids 'R' 'G' 'B' without an Adobe marker: no colour conversion
    uint16_t qt[3][64];   // each component's quantisation table, natural order, as it stood after the last scan
    icl_jpeg_component comp[3];
};

// Stage A.  Every check of a hostile file is made here; on success J holds a decodable image (1 or 3 components,
// luma 1x1 / 2x1 / 2x2 / 1x2 / 4x1 / 1x4 over 1x1 chroma, at most ICL_JPEG_MAX_PIXELS).  J may be reused across calls: the scans decode
// straight into its coefficient arrays, which keep their capacity whether a call succeeds or fails.  After a failure J holds whatever
// the parser had read by then (frame geometry included); only a successful call leaves a J to read, and
// then comp[0 .. ncomp-1] alone: a component at index ncomp or above is unspecified (it may hold an earlier file's).
int icl_jpeg_stage_a(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, icl_jpeg_coefs &J);
// Stage B on the host: interleaved RGB, W*H*3 (before the EXIF orientation).
int icl_jpeg_stage_b(icl_ctx *ctx, const icl_jpeg_coefs &J, const char *path, std::vector<uint8_t> &rgb);

// Stage A then stage B (the host decoder in one call).  orient receives the EXIF orientation (1..8; 1 when absent).
int icl_jpeg_decode(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, std::vector<uint8_t> &rgb, int &W, int &H, int &orient);

// Stage A0: what a host worker does for a JPEG whose entropy decoder runs on the GPU (jpeg_huff_gpu.hip) -- the marker loop of stage A,
// stopped at the first scan: frame, tables in force, restart interval and the unstuffed entropy-coded segment, cut at its RSTn markers.
struct icl_jpeg_a0 {
    icl_je_scan scan;       // geometry; the placement fields are left to the caller
    icl_je_table tables[6]; // component c: DC table, AC table
    std::vector<icl_je_interval> intervals;
    std::vector<uint8_t> stream; // scan.nsub subsequences of scan.sub_bits bits (every interval zero-padded to whole subsequences)
};
// qualifies = false (with ICL_OK or an error code): the file takes the usual route (stage A or the host decoders), which also produces
// its status and message.  Qualifying: SOF0 / SOF1, one scan with all components in frame order.  On success J holds everything stage A
// leaves except the coefficients (their arrays are empty).
int icl_jpeg_stage_a0(const uint8_t *data, size_t len, const char *path, int sub_bits, icl_jpeg_coefs &J, icl_jpeg_a0 &A, bool &qualifies);
// The GPU decoder's schedule as a plain host loop over subsequences (the same decode step and checks, jpeg_entropy.h): launches x
// workgroups x rounds, then the chain / cleanliness check, then (accepted images only) the coefficients as stage A leaves them.
// rounds receives the largest number of rounds a workgroup needed until no entry state changed.
void icl_je_host_decode(const icl_jpeg_a0 &A, std::vector<int16_t> coefs[3], bool &accepted, int &rounds);

// jpeg_huff_gpu.hip: the decode of one slab's scans on the GPU.  d_scans[nscans] (placement fields filled: offsets into d_payload, sub_first,
// wg_first ascending, coef_off into d_coef) -> d_accepted[nscans], and the accepted images' coefficients in d_coef (zero-filled by the caller).
struct icl_je_slab {
    const icl_je_scan *d_scans;
    int nscans;
    const uint8_t *d_payload;
    int64_t payload_bytes;
    icl_je_sub *d_sub;
    int64_t nsub_cap;
    uint32_t *d_bound; // 2 arrays of 2 * nwg_cap words: the workgroups' last exit states of alternate launches
    int64_t nwg_cap, total_wgs;
    int32_t *d_accepted;
    int16_t *d_coef;
    int64_t coef_elems;
};
int icl_je_decode_slab(icl_ctx *ctx, hipStream_t st, const icl_je_slab &s);

// image_io.hip: the host ingest path.  The batched file path (jpeg_gpu.hip) reads and sniffs files, and decodes what the GPU does not
// take, through it; the icl_embed_file batcher (embed_file.hip) reads and resizes through it.
enum { ICL_IMAGE_EMPTY = -2, ICL_IMAGE_UNREADABLE = -1, ICL_IMAGE_PPM = 0, ICL_IMAGE_PNG = 1, ICL_IMAGE_JPEG = 2 };
// Opens path and tells its format by the first bytes (PNG signature, JPEG SOI; anything else goes to the PPM reader).  A PNG or
// JPEG is read whole into `file`.  ICL_IMAGE_UNREADABLE: the file cannot be opened, or a PNG / JPEG cannot be read whole.
int icl_image_file_read(const char *path, std::vector<uint8_t> &file);
// The bytes of a source (ingest_src, icl_common.h) and their format: a file through icl_image_file_read (data / len then point into
// `file`), a memory source by the same sniffing rule on the caller's buffer, which data / len then name as they stand (no copy;
// ICL_IMAGE_EMPTY for data == NULL or bytes <= 0).
int icl_image_src_read(const ingest_src &src, std::vector<uint8_t> &file, const uint8_t *&data, size_t &len);
// IMRead(IMReadColor) of what icl_image_src_read returned: interleaved RGB, w*h*3, the EXIF orientation applied.  Every status
// code and message of the host path comes from here; name (ingest_src_name) is what the messages call the source.
int icl_image_decode(icl_ctx *ctx, const ingest_src &src, const char *name, int fmt, const uint8_t *data, size_t len, std::vector<uint8_t> &rgb, int &w, int &h);
// read + decode + cv::resize to the 224x224x3 u8 image (icl_load_image_224, icl_load_image_224_mem)
int icl_read_image_224(icl_ctx *ctx, const ingest_src &src, uint8_t *out);
void icl_apply_exif_orientation(std::vector<uint8_t> &rgb, int &w, int &h, int orient);
void icl_resize_bilinear_u8(const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh);
void icl_resize_coeffs(int dn, int sn, int32_t *ofs, int16_t *al); // cv::resize INTER_LINEAR source offsets + 11-bit weights

// jpeg_encode.hip: the host JPEG encoder (arithmetic and tables: jpeg_encode_pixels.h) and the two-call delivery of a finished file
struct icl_jenc_tables;
void icl_jenc_encode_host(const uint8_t *rgb, int w, int h, const icl_jenc_tables &T, std::vector<uint8_t> &out);
int64_t icl_jenc_bound(int w, int h);
int icl_deliver_bytes(const std::vector<uint8_t> &file, uint8_t *out, int64_t cap, int64_t *bytes, const char *what);
// jpeg_encode.hip: resizeImageIfNeeded (rekognition.go:173-259).  The size rule for an oriented image of R rows and C columns, quirk
// included (false: newW or newH < 1); the whole host route for one source (info[6]: imageclust.h), which the batched call
// (jpeg_gpu.hip) also takes for what the GPU does not.
constexpr int ICL_DOWNSIZE_QUALITY = 95;
bool icl_downsize_dims(int R, int C, int max_dim, int &newW, int &newH);
int icl_downsize_dims_checked(const char *name, int w, int h, int max_dim, int &nw, int &nh); // ... of a w x h image; ICL_ERR_ARG names the sizes
int icl_src_bytes(const ingest_src &src, const char *name, std::vector<uint8_t> &file, const uint8_t *&data, size_t &len); // a source's bytes as they stand
int icl_downsize_src(const ingest_src &src, int64_t max_bytes, int max_dim, std::vector<uint8_t> &out, int32_t *info);
// jpeg_encode_gpu.hip: one batch of the GPU encoder (ctx->mu held, device selected): image i is d_rgb + items[i].rgb_off; the files
// land in the encoder's own device buffer *d_files, file i at off[i] .. off[i + 1] (valid until the next batch).  A batch holds at most
// icl_jenc_max_batch_blocks() blocks (icl_jenc_blocks of each image) and icl_jenc_max_batch_images() images.  Returns with the stream
// synchronised.
struct icl_jenc_item {
    int64_t rgb_off;
    int32_t w, h;
};
int64_t icl_jenc_max_batch_blocks();
int64_t icl_jenc_max_batch_images();
int64_t icl_jenc_blocks(int w, int h);
int icl_jenc_run(icl_ctx *ctx, const uint8_t *d_rgb, const icl_jenc_item *items, int64_t n, int quality, const uint8_t **d_files, std::vector<int64_t> &off);
