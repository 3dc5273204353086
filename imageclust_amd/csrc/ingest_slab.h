// ingest_slab.h -- what the kernels of the batched file path (jpeg_gpu.hip, png_gpu.hip) read about one output row of a slab.
#pragma once
#include "icl_common.h"
#include "png_inflate.h"

constexpr int ICL_OUTW = ICL_IMG_W, ICL_OUTH = ICL_IMG_H;
// (KIND_JSTREAM: a JPEG as bit stream; the kernels see it as KIND_JPEG.  KIND_PSTREAM: a PNG as zlib stream, png_gpu.hip.)
enum { KIND_FAILED = 0, KIND_JPEG = 1, KIND_HOST = 2, KIND_JSTREAM = 3, KIND_PSTREAM = 4 };

struct ingest_image {
    int32_t kind;
    int32_t W, H;   // decoded size
    int32_t ow, oh; // size after the EXIF orientation (the resize's source)
    int32_t orient, ncomp, hs, vs, is_rgb, area;
    int32_t cw, chh;          // chroma samples per row / rows (dw, dh of components 1 and 2)
    int32_t ystride, yrows;   // luma plane: wblocks*8 x hblocks*8
    int32_t cstride, crows;   // chroma planes
    int32_t pad_;
    int64_t yplane, cplane[2]; // byte offsets in the plane scratch (KIND_PSTREAM: yplane is where the image's scanlines go)
    int64_t host_off;          // KIND_HOST: byte offset of the finished image in the payload; KIND_PSTREAM: of its icl_png_desc
    int32_t xofs[ICL_OUTW], yofs[ICL_OUTH];
    int16_t xa[ICL_OUTW * 2], ya[ICL_OUTH * 2];
};

// A KIND_PSTREAM row's descriptor, once everything a kernel relies on has been checked against the buffers' extents: descriptor and
// stream inside the payload, `want` bytes of scanlines inside the scratch, a geometry that agrees with itself.  NULL otherwise.
__host__ __device__ inline const icl_png_desc *icl_png_job(const ingest_image &I, const uint8_t *payload, int64_t payload_bytes, int64_t scratch_bytes)
{
    if (I.kind != KIND_PSTREAM || I.host_off < 0 || (I.host_off & 15) || I.host_off + (int64_t)sizeof(icl_png_desc) > payload_bytes) return nullptr;
    const icl_png_desc *D = (const icl_png_desc *)(payload + I.host_off);
    if (D->zbytes < 6 || I.host_off + (int64_t)sizeof(icl_png_desc) + (((int64_t)D->zbytes + 15) & ~(int64_t)15) > payload_bytes) return nullptr;
    if (D->want < 1 || I.yplane < 0 || (I.yplane & 15) || I.yplane + D->want > scratch_bytes) return nullptr;
    const int ch = D->ctype == 0 ? 1 : D->ctype == 2 ? 3 : D->ctype == 3 ? 1 : D->ctype == 4 ? 2 : D->ctype == 6 ? 4 : 0;
    const bool depth_ok = D->depth == 1 || D->depth == 2 || D->depth == 4 || D->depth == 8 || D->depth == 16;
    if (ch == 0 || !depth_ok || D->w < 1 || D->h < 1 || D->w > 65535 || D->h > 65535 || D->w != I.W || D->h != I.H) return nullptr;
    const int64_t bits = (int64_t)ch * D->depth, rowb = ((int64_t)D->w * bits + 7) / 8, bpp = bits >= 8 ? bits / 8 : 1;
    if (D->rowb != rowb || D->bpp != bpp || D->want != (int64_t)D->h * (rowb + 1) || D->npal < 0 || D->npal > 256) return nullptr;
    return D;
}

// png_gpu.hip: the PNG rows of an uploaded slab into their scanlines in the scratch -- inflate, Adler-32, and (stages >= 2) unfilter +
// palette check.  d_ok[i] (one per row of the slab; 0 for rows that are no PNG) tells which images the GPU accepts.
int icl_png_decode_slab(icl_ctx *ctx, hipStream_t st, const ingest_image *d_imgs, int nimg, const uint8_t *d_payload, int64_t payload_bytes, uint8_t *d_scratch,
                        int64_t scratch_bytes, int32_t *d_ok, int stages);
