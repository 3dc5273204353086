// image_io.hip -- host-side image ingest: PreprocessImage (/root/reference/internal/embeddings/embeddings.go:46-116), i.e.
// gocv.IMRead(IMReadColor) for the formats this build decodes (JPEG: jpeg_decode.hip, PNG: png_decode.hip, binary PPM here),
// cv::imread's EXIF orientation, the OpenCV-compatible 8-bit resize to 224x224 and the RGB/255 NCHW blob.  The pixel arithmetic
// lives in ingest_pixels.h, shared with the GPU rebuild of the batched file path (jpeg_gpu.hip), which also calls the file
// reader, the orientation and the resize (tables) below (jpeg_stage.h).
#include "icl_common.h"
#include "ingest_pixels.h"
#include "jpeg_stage.h"

#include <cmath>
#include <cstring>
#include <memory>

bool icl_is_png(const uint8_t *data, size_t len); // png_decode.hip
int icl_png_decode(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, std::vector<uint8_t> &rgb, int &W, int &H);

extern "C" int icl_preprocess_u8(const uint8_t *hwc, float *nchw)
{
    if (!hwc || !nchw) return ICL_ERR_ARG;
    const float sc = (float)(1.0 / 255.0);
    for (int y = 0; y < ICL_IMG_H; ++y)
        for (int x = 0; x < ICL_IMG_W; ++x)
            for (int c = 0; c < 3; ++c) nchw[((size_t)c * ICL_IMG_H + y) * ICL_IMG_W + x] = (float)hwc[((size_t)y * ICL_IMG_W + x) * 3 + c] * sc;
    return ICL_OK;
}

// source offsets and 11-bit weights of one axis of cv::resize(INTER_LINEAR) (float / double arithmetic: jpeg_gpu.hip uploads these
// host-computed tables rather than recomputing them on the device)
void icl_resize_coeffs(int dn, int sn, int32_t *ofs, int16_t *al)
{
    const double scale = (double)sn / dn;
    for (int d = 0; d < dn; ++d) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = (int)std::floor(f);
        f -= s;
        if (s < 0) { f = 0; s = 0; }
        if (s >= sn - 1) { f = 0; s = sn - 1; }
        ofs[d] = s;
        al[(size_t)d * 2] = (short)std::lrint((1.f - f) * 2048.f);
        al[(size_t)d * 2 + 1] = (short)std::lrint(f * 2048.f);
    }
}

// cv::resize(INTER_LINEAR) for 8-bit RGB images: half-pixel centres, 11-bit fixed-point coefficients, OpenCV's two-pass rounding,
// or INTER_AREA for an exact 2x2 decimation (embeddings.go:69 resizes every image to 224x224)
void icl_resize_bilinear_u8(const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh)
{
    const int cn = 3;
    if (icl_resize_is_area(sw, sh, dw, dh)) {
        for (int y = 0; y < dh; ++y) {
            const uint8_t *r0 = src + (size_t)(2 * y) * sw * cn, *r1 = r0 + (size_t)sw * cn;
            for (int x = 0; x < dw; ++x)
                for (int c = 0; c < cn; ++c)
                    dst[((size_t)y * dw + x) * cn + c] = icl_area_mean(r0[(2 * x) * cn + c], r0[(2 * x + 1) * cn + c], r1[(2 * x) * cn + c], r1[(2 * x + 1) * cn + c]);
        }
        return;
    }
    std::vector<int32_t> xofs((size_t)dw), yofs((size_t)dh);
    std::vector<int16_t> xa((size_t)dw * 2), ya((size_t)dh * 2);
    icl_resize_coeffs(dw, sw, xofs.data(), xa.data());
    icl_resize_coeffs(dh, sh, yofs.data(), ya.data());
    for (int dy = 0; dy < dh; ++dy) {
        const int sy = yofs[(size_t)dy], sy1 = std::min(sy + 1, sh - 1);
        const uint8_t *r0 = src + (size_t)sy * sw * cn, *r1 = src + (size_t)sy1 * sw * cn;
        const int b0 = ya[(size_t)dy * 2], b1 = ya[(size_t)dy * 2 + 1];
        for (int dx = 0; dx < dw; ++dx) {
            const int sx = xofs[(size_t)dx], sx1 = std::min(sx + 1, sw - 1);
            const int a0 = xa[(size_t)dx * 2], a1 = xa[(size_t)dx * 2 + 1];
            for (int c = 0; c < cn; ++c)
                dst[((size_t)dy * dw + dx) * cn + c] = icl_resize_linear(r0[sx * cn + c], r0[sx1 * cn + c], r1[sx * cn + c], r1[sx1 * cn + c], a0, a1, b0, b1);
        }
    }
}

// the two byte sources of the PPM reader: a file read as it goes, or a memory source's buffer (never read past its end)
struct ppm_file {
    FILE *f;
    int get() { return fgetc(f); }
    bool holds(size_t) const { return true; } // (the read tells)
    bool read(uint8_t *dst, size_t n) { return fread(dst, 1, n, f) == n; }
};
struct ppm_mem {
    const uint8_t *p, *end;
    int get() { return p < end ? (int)*p++ : EOF; }
    bool holds(size_t n) const { return (size_t)(end - p) >= n; }
    bool read(uint8_t *dst, size_t n)
    {
        if (!holds(n)) return false;
        memcpy(dst, p, n);
        p += n;
        return true;
    }
};

template <class S> static bool ppm_parse(S &s, std::vector<uint8_t> &rgb, int &w, int &h)
{
    auto token = [&](int &v) -> bool {
        int c;
        do {
            c = s.get();
            if (c == '#')
                while (c != '\n' && c != EOF) c = s.get();
        } while (c == ' ' || c == '\n' || c == '\r' || c == '\t');
        if (c < '0' || c > '9') return false;
        v = 0;
        while (c >= '0' && c <= '9') {
            if (v > (1 << 24)) return false; // (far above every accepted value: no overflow on a long run of digits)
            v = v * 10 + (c - '0');
            c = s.get();
        }
        return true;
    };
    int maxv = 0;
    bool ok = s.get() == 'P' && s.get() == '6' && token(w) && token(h) && token(maxv) && maxv == 255 && w > 0 && h > 0 && w <= 16384 && h <= 16384 &&
              s.holds((size_t)w * h * 3);
    if (ok) {
        rgb.resize((size_t)w * h * 3);
        ok = s.read(rgb.data(), rgb.size());
    }
    return ok;
}

static int read_ppm(icl_ctx *ctx, const ingest_src &src, const char *name, const uint8_t *data, size_t len, std::vector<uint8_t> &rgb, int &w, int &h)
{
    bool ok;
    if (src.path) {
        FILE *f = fopen(src.path, "rb");
        if (!f) return icl_fail(ctx, ICL_ERR_IO, "failed to read image: %s. The image file might be corrupt or unreadable", name); // embeddings.go:52
        ppm_file s{f};
        ok = ppm_parse(s, rgb, w, h);
        fclose(f);
    } else {
        ppm_mem s{data, data + len};
        ok = ppm_parse(s, rgb, w, h);
    }
    if (!ok) return icl_fail(ctx, ICL_ERR_IO, "failed to read image: %s. Only JPEG (Huffman; baseline or progressive), PNG and binary PPM (P6, maxval 255) are decoded by this build", name);
    return ICL_OK;
}

// cv::imread rotates / mirrors the decoded pixels by the file's EXIF orientation (icl_exif_source, ingest_pixels.h)
void icl_apply_exif_orientation(std::vector<uint8_t> &rgb, int &w, int &h, int orient)
{
    if (orient <= 1 || orient > 8) return;
    const int sw = w, sh = h;
    const bool swap = icl_exif_swaps_axes(orient);
    const int dw = swap ? sh : sw, dh = swap ? sw : sh;
    std::vector<uint8_t> out((size_t)dw * dh * 3);
    for (int y = 0; y < dh; ++y)
        for (int x = 0; x < dw; ++x) {
            int sx, sy;
            icl_exif_source(orient, sw, sh, x, y, sx, sy);
            memcpy(&out[((size_t)y * dw + x) * 3], &rgb[((size_t)sy * sw + sx) * 3], 3);
        }
    rgb.swap(out);
    w = dw;
    h = dh;
}

// the format rule of files and memory sources alike, on the first (up to) 8 bytes
static int sniff_format(const uint8_t *magic, size_t got)
{
    if (got == 8 && icl_is_png(magic, 8)) return ICL_IMAGE_PNG;
    if (got >= 2 && magic[0] == 0xFF && magic[1] == 0xD8) return ICL_IMAGE_JPEG;
    return ICL_IMAGE_PPM;
}

int icl_image_file_read(const char *path, std::vector<uint8_t> &file)
{
    std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(path, "rb"), fclose);
    if (!f) return ICL_IMAGE_UNREADABLE;
    unsigned char magic[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const size_t got = fread(magic, 1, 8, f.get());
    const int fmt = sniff_format(magic, got);
    if (fmt == ICL_IMAGE_PPM) return fmt; // read_ppm parses the file itself
    fseek(f.get(), 0, SEEK_END);
    const long sz = ftell(f.get());
    fseek(f.get(), 0, SEEK_SET);
    file.resize((size_t)std::max<long>(sz, 0));
    return sz > 0 && fread(file.data(), 1, file.size(), f.get()) == file.size() ? fmt : ICL_IMAGE_UNREADABLE;
}

const char *ingest_src_name(const ingest_src &s, char *buf, size_t cap)
{
    if (s.path) return s.path;
    snprintf(buf, cap, "image %lld (in memory, %lld bytes)", (long long)s.index, (long long)(s.data && s.bytes > 0 ? s.bytes : 0));
    return buf;
}

int icl_image_src_read(const ingest_src &src, std::vector<uint8_t> &file, const uint8_t *&data, size_t &len)
{
    data = nullptr;
    len = 0;
    if (src.path) {
        const int fmt = icl_image_file_read(src.path, file);
        data = file.data();
        len = file.size();
        return fmt;
    }
    if (!src.data || src.bytes <= 0) return ICL_IMAGE_EMPTY;
    data = src.data;
    len = (size_t)src.bytes;
    return sniff_format(data, std::min<size_t>(len, 8));
}

int icl_image_decode(icl_ctx *ctx, const ingest_src &src, const char *name, int fmt, const uint8_t *data, size_t len, std::vector<uint8_t> &rgb, int &w, int &h)
{
    switch (fmt) {
    case ICL_IMAGE_PNG: return icl_png_decode(ctx, data, len, name, rgb, w, h);
    case ICL_IMAGE_JPEG: {
        int orient = 1;
        ICL_TRY(icl_jpeg_decode(ctx, data, len, name, rgb, w, h, orient));
        icl_apply_exif_orientation(rgb, w, h, orient);
        return ICL_OK;
    }
    case ICL_IMAGE_PPM: return read_ppm(ctx, src, name, data, len, rgb, w, h);
    case ICL_IMAGE_EMPTY: return icl_fail(ctx, ICL_ERR_IO, "failed to read image: %s. empty image buffer", name);
    default: return icl_fail(ctx, ICL_ERR_IO, "failed to read image: %s. The image file might be corrupt or unreadable", name); // embeddings.go:52
    }
}

// IMRead(IMReadColor) of embeddings.go:50
static int read_image(icl_ctx *ctx, const ingest_src &src, std::vector<uint8_t> &rgb, int &w, int &h)
{
    std::vector<uint8_t> file;
    const uint8_t *data;
    size_t len;
    char nbuf[96];
    const int fmt = icl_image_src_read(src, file, data, len);
    return icl_image_decode(ctx, src, ingest_src_name(src, nbuf, sizeof nbuf), fmt, data, len, rgb, w, h);
}

int icl_read_image_224(icl_ctx *ctx, const ingest_src &src, uint8_t *out)
{
    std::vector<uint8_t> px;
    int w = 0, h = 0;
    ICL_TRY(read_image(ctx, src, px, w, h));
    icl_resize_bilinear_u8(px.data(), w, h, out, ICL_IMG_W, ICL_IMG_H);
    return ICL_OK;
}

// No C++ exception may cross the C ABI (cgo / ctypes would terminate the host process): the ingest entry points allocate
// buffers whose sizes come from files (no_throw: icl_common.h).
static int decode_image(const ingest_src &src, uint8_t *rgb, int64_t cap_bytes, int32_t *w, int32_t *h, const char *what)
{
    return no_throw(nullptr, what, [&]() -> int {
        std::vector<uint8_t> px;
        int iw = 0, ih = 0;
        ICL_TRY(read_image(nullptr, src, px, iw, ih));
        *w = iw;
        *h = ih;
        if (rgb) {
            if (cap_bytes < (int64_t)px.size()) return icl_fail(nullptr, ICL_ERR_ARG, "%s: buffer too small", what);
            memcpy(rgb, px.data(), px.size());
        }
        return ICL_OK;
    });
}

extern "C" int icl_decode_image_file(const char *path, uint8_t *rgb, int64_t cap_bytes, int32_t *w, int32_t *h)
{
    if (!path || !w || !h) return icl_fail(nullptr, ICL_ERR_ARG, "icl_decode_image_file: bad argument");
    return decode_image(ingest_src{path, nullptr, 0, 0}, rgb, cap_bytes, w, h, "icl_decode_image_file");
}

extern "C" int icl_decode_image_mem(const uint8_t *data, int64_t bytes, uint8_t *rgb, int64_t cap_bytes, int32_t *w, int32_t *h)
{
    if (!w || !h) return icl_fail(nullptr, ICL_ERR_ARG, "icl_decode_image_mem: bad argument");
    return decode_image(ingest_src{nullptr, data, bytes, 0}, rgb, cap_bytes, w, h, "icl_decode_image_mem");
}

extern "C" int icl_load_image_224(const char *path, uint8_t *out)
{
    if (!path || !out) return icl_fail(nullptr, ICL_ERR_ARG, "icl_load_image_224: bad argument");
    return no_throw(nullptr, "icl_load_image_224", [&]() -> int { return icl_read_image_224(nullptr, ingest_src{path, nullptr, 0, 0}, out); });
}

extern "C" int icl_load_image_224_mem(const uint8_t *data, int64_t bytes, uint8_t *out)
{
    if (!out) return icl_fail(nullptr, ICL_ERR_ARG, "icl_load_image_224_mem: bad argument");
    return no_throw(nullptr, "icl_load_image_224_mem", [&]() -> int { return icl_read_image_224(nullptr, ingest_src{nullptr, data, bytes, 0}, out); });
}

// Test hook without a GPU: the quantised coefficients of a JPEG by host stage A (sub_bits == 0), or by stage A0 + the GPU entropy
// decoder's schedule run as a host loop (jpeg_entropy.h, icl_je_host_decode).
extern "C" int icl_jpeg_coefs_file_host(const char *path, int sub_bits, int16_t *coefs, int64_t cap, int64_t *need, int32_t *info)
{
    if (!path || !need || !info || sub_bits < 0) return icl_fail(nullptr, ICL_ERR_ARG, "icl_jpeg_coefs_file_host: bad argument");
    return no_throw(nullptr, "icl_jpeg_coefs_file_host", [&]() -> int {
        std::vector<uint8_t> file;
        if (icl_image_file_read(path, file) != ICL_IMAGE_JPEG) return icl_fail(nullptr, ICL_ERR_IO, "icl_jpeg_coefs_file_host: %s is not a readable JPEG", path);
        icl_jpeg_coefs J;
        std::vector<int16_t> own[3];
        const std::vector<int16_t> *cf[3] = {&own[0], &own[1], &own[2]};
        int rounds = 0, nsub = 0, nint = 0, state = 1;
        if (sub_bits == 0) {
            ICL_TRY(icl_jpeg_stage_a(nullptr, file.data(), file.size(), path, J));
            for (int c = 0; c < 3; ++c) cf[c] = &J.comp[c].coefs;
        } else {
            icl_jpeg_a0 A;
            bool qualifies = false, accepted = false;
            const int rc = icl_jpeg_stage_a0(file.data(), file.size(), path, sub_bits, J, A, qualifies);
            if (rc == ICL_ERR_ARG) return icl_fail(nullptr, rc, "icl_jpeg_coefs_file_host: sub_bits must be a multiple of 32, at least 64");
            if (!qualifies) {
                state = -1;
            } else {
                icl_je_host_decode(A, own, accepted, rounds);
                state = accepted ? 1 : 0;
                nsub = (int)A.scan.nsub;
                nint = A.scan.nintervals;
            }
        }
        int64_t total = 0;
        info[0] = state;
        info[1] = state == -1 ? 0 : J.ncomp;
        for (int c = 0; c < 3; ++c) {
            const int64_t nb = state == 1 && c < J.ncomp ? (int64_t)J.comp[c].wblocks * J.comp[c].hblocks : 0;
            info[2 + c] = (int32_t)nb;
            total += nb * 64;
        }
        info[5] = rounds;
        info[6] = nsub;
        info[7] = nint;
        *need = total;
        if (coefs && cap >= total) {
            int64_t at = 0;
            for (int c = 0; c < 3; ++c) {
                const int64_t ne = (int64_t)info[2 + c] * 64;
                if (ne && (int64_t)cf[c]->size() != ne) return icl_fail(nullptr, ICL_ERR_IO, "icl_jpeg_coefs_file_host: inconsistent coefficient count");
                if (ne) memcpy(coefs + at, cf[c]->data(), (size_t)ne * 2);
                at += ne;
            }
        }
        return ICL_OK;
    });
}

// cv::resize on an arbitrary u8 RGB image (the resize step of PreprocessImage alone; tests pin it to hand-derived vectors)
extern "C" int icl_resize_u8(const uint8_t *src, int32_t sw, int32_t sh, uint8_t *dst, int32_t dw, int32_t dh)
{
    if (!src || !dst || sw < 1 || sh < 1 || dw < 1 || dh < 1) return icl_fail(nullptr, ICL_ERR_ARG, "icl_resize_u8: bad argument");
    return no_throw(nullptr, "icl_resize_u8", [&]() -> int {
        icl_resize_bilinear_u8(src, sw, sh, dst, dw, dh);
        return ICL_OK;
    });
}

// PreprocessImage(imagePath) (embeddings.go:46-116): file -> the 1x3x224x224 fp32 NCHW blob.
static int preprocess(const ingest_src &src, float *nchw, const char *what)
{
    return no_throw(nullptr, what, [&]() -> int {
        std::vector<uint8_t> img((size_t)ICL_IMG_BYTES);
        ICL_TRY(icl_read_image_224(nullptr, src, img.data()));
        return icl_preprocess_u8(img.data(), nchw);
    });
}

extern "C" int icl_preprocess_file(const char *path, float *nchw)
{
    if (!path || !nchw) return icl_fail(nullptr, ICL_ERR_ARG, "icl_preprocess_file: bad argument");
    return preprocess(ingest_src{path, nullptr, 0, 0}, nchw, "icl_preprocess_file");
}

extern "C" int icl_preprocess_mem(const uint8_t *data, int64_t bytes, float *nchw)
{
    if (!nchw) return icl_fail(nullptr, ICL_ERR_ARG, "icl_preprocess_mem: bad argument");
    return preprocess(ingest_src{nullptr, data, bytes, 0}, nchw, "icl_preprocess_mem");
}
