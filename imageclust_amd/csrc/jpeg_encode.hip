// jpeg_encode.hip -- the host JPEG encoder: what cv::imwrite(".jpg") / libjpeg's defaults write for an 8-bit RGB image (baseline SOF0,
// YCbCr 4:2:0, Annex K Huffman tables, islow DCT, JFIF 1.01).  The arithmetic is jpeg_encode_pixels.h, shared with the GPU encoder
// (jpeg_encode_gpu.hip); this file adds what only the host needs: the tables of a quality, the header, the byte writer -- and the
// downsizer built on it, resizeImageIfNeeded (rekognition.go:173-259), behind icl_downsize_image_file / _mem.  (It lives here and not in
// image_io.hip so that the decoders still link without the encoder.)
#include "icl_common.h"
#include "jpeg_encode_pixels.h"
#include "jpeg_stage.h"

#include <cstring>
#include <memory>

namespace {

// T.81 Annex K.1 (natural order)
const uint8_t base_luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                               14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t base_chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 Annex K.3: code counts per length 1..16, then the symbols in code order
const uint8_t dc_luma_bits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t dc_chroma_bits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t ac_luma_bits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t ac_luma_vals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
    0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
    0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
    0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t ac_chroma_bits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t ac_chroma_vals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
    0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
    0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct huff_spec {
    const uint8_t *bits, *vals;
    int nvals;
};
const huff_spec specs[4] = {{dc_luma_bits, dc_vals, 12}, {ac_luma_bits, ac_luma_vals, 162}, {dc_chroma_bits, dc_vals, 12}, {ac_chroma_bits, ac_chroma_vals, 162}};

// jchuff.c jpeg_make_c_derived_tbl: canonical codes in order of length
void derive(const huff_spec &s, uint16_t *code, uint8_t *size)
{
    memset(code, 0, 256 * sizeof(uint16_t));
    memset(size, 0, 256);
    unsigned c = 0;
    int p = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < s.bits[l - 1]; ++i, ++p) {
            code[s.vals[p]] = (uint16_t)c++;
            size[s.vals[p]] = (uint8_t)l;
        }
        c <<= 1;
    }
}

// the entropy-coded segment's byte writer: a 0x00 behind every 0xFF byte, the last partial byte padded with 1 bits
struct byte_sink {
    std::vector<uint8_t> &out;
    uint64_t acc = 0;
    int nacc = 0;
    void put(uint32_t v, int n)
    {
        acc = (acc << n) | v;
        nacc += n;
        while (nacc >= 8) {
            const uint8_t b = (uint8_t)(acc >> (nacc - 8));
            out.push_back(b);
            if (b == 0xFF) out.push_back(0);
            nacc -= 8;
        }
    }
    void flush()
    {
        if (nacc) put((1u << (8 - nacc)) - 1, 8 - nacc);
    }
};

} // namespace

void icl_jenc_make_tables(int quality, icl_jenc_tables &T)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality; // jpeg_quality_scaling
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const long v = ((long)(t ? base_chroma : base_luma)[i] * s + 50) / 100;
            T.qt[t][i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v)); // force_baseline
        }
    for (int t = 0; t < 4; ++t) derive(specs[t], T.code[t], T.size[t]);
}

void icl_jenc_write_header(const icl_jenc_tables &T, int w, int h, uint8_t *out)
{
    uint8_t *p = out;
    auto put = [&](std::initializer_list<int> l) {
        for (int b : l) *p++ = (uint8_t)b;
    };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int k = 0; k < 64; ++k) *p++ = (uint8_t)T.qt[t][icl_zigzag[k]];
    }
    put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    static const int ids[4] = {0x00, 0x10, 0x01, 0x11}; // libjpeg writes DC then AC of table 0, then of table 1
    for (int t = 0; t < 4; ++t) {
        const huff_spec &s = specs[t];
        put({0xFF, 0xC4, 0, 19 + s.nvals, ids[t]});
        memcpy(p, s.bits, 16);
        p += 16;
        memcpy(p, s.vals, (size_t)s.nvals);
        p += s.nvals;
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    static_assert(ICL_JENC_HEADER == 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 14, "header size");
}

void icl_jenc_encode_host(const uint8_t *rgb, int w, int h, const icl_jenc_tables &T, std::vector<uint8_t> &out)
{
    const icl_jenc_geom g = icl_jenc_geometry(w, h);
    out.clear();
    out.reserve((size_t)ICL_JENC_HEADER + (size_t)g.mw * g.mh * 96 + 16);
    out.resize((size_t)ICL_JENC_HEADER);
    icl_jenc_write_header(T, w, h, out.data());
    byte_sink sink{out};
    int pred[3] = {0, 0, 0};
    int s[64];
    int16_t zz[64];
    for (int my = 0; my < g.mh; ++my)
        for (int mx = 0; mx < g.mw; ++mx)
            for (int k = 0; k < 6; ++k) {
                const int c = k < 4 ? 0 : k - 3;
                if (icl_jenc_is_dummy(g, mx, my, k)) {
                    memset(zz, 0, sizeof zz);
                    zz[0] = (int16_t)pred[c];
                } else {
                    icl_jenc_block_samples(rgb, g, mx, my, k, s);
                    icl_jenc_block_coefs(s, T.qt[c ? 1 : 0], zz);
                }
                icl_jenc_encode_block([&](int i) { return (int)zz[i]; }, zz[0] - pred[c], T, c ? ICL_JENC_DC1 : ICL_JENC_DC0, c ? ICL_JENC_AC1 : ICL_JENC_AC0, sink);
                pred[c] = zz[0];
            }
    sink.flush();
    out.push_back(0xFF);
    out.push_back(0xD9);
}

static bool jenc_size_ok(int64_t w, int64_t h) { return w >= 1 && h >= 1 && w <= 65535 && h <= 65535; }

int64_t icl_jenc_bound(int w, int h)
{
    const icl_jenc_geom g = icl_jenc_geometry(w, h);
    return (int64_t)ICL_JENC_HEADER + 2 + (int64_t)g.mw * g.mh * 6 * (ICL_JENC_BLOCK_BITS / 8) * 2 + 2;
}

extern "C" int64_t icl_jpeg_encode_bound(int32_t w, int32_t h) { return jenc_size_ok(w, h) ? icl_jenc_bound(w, h) : 0; }

// the two-call convention of the encoder and the downsizer: the size always, the bytes when there is room for them
int icl_deliver_bytes(const std::vector<uint8_t> &file, uint8_t *out, int64_t cap, int64_t *bytes, const char *what)
{
    *bytes = (int64_t)file.size();
    if (!out) return ICL_OK;
    if (cap < (int64_t)file.size()) return icl_fail(nullptr, ICL_ERR_ARG, "%s: buffer too small (%lld bytes needed)", what, (long long)file.size());
    memcpy(out, file.data(), file.size());
    return ICL_OK;
}

extern "C" int icl_jpeg_encode_rgb(const uint8_t *rgb, int32_t w, int32_t h, int32_t quality, uint8_t *out, int64_t cap, int64_t *bytes)
{
    if (!rgb || !bytes) return icl_fail(nullptr, ICL_ERR_ARG, "icl_jpeg_encode_rgb: bad argument");
    if (!jenc_size_ok(w, h)) return icl_fail(nullptr, ICL_ERR_ARG, "icl_jpeg_encode_rgb: %d x %d is outside 1..65535", (int)w, (int)h);
    if (quality < 1 || quality > 100) return icl_fail(nullptr, ICL_ERR_ARG, "icl_jpeg_encode_rgb: quality %d is outside 1..100", (int)quality);
    return no_throw(nullptr, "icl_jpeg_encode_rgb", [&]() -> int {
        icl_jenc_tables T;
        icl_jenc_make_tables(quality, T);
        std::vector<uint8_t> file;
        icl_jenc_encode_host(rgb, w, h, T, file);
        return icl_deliver_bytes(file, out, cap, bytes, "icl_jpeg_encode_rgb");
    });
}

// ---- resizeImageIfNeeded (rekognition.go:173-259) ----
// gocv's Size() is [rows, cols]; the reference reads it as (width, height), so its "aspect ratio" is cols / rows and the long side it
// picks is the other one.  Go's float64 arithmetic and int() truncation, restated in double.
bool icl_downsize_dims(int R, int C, int max_dim, int &newW, int &newH)
{
    const double ratio = (double)C / (double)R;
    // (the other side never exceeds max_dim: ratio < 1 in the first branch, >= 1 in the second; the clamp keeps the cast defined whatever comes in)
    auto trunc = [](double v) { return v >= 2147483647.0 ? 2147483647 : (v >= 1.0 ? (int)v : 0); };
    if (R > C) {
        newW = max_dim;
        newH = trunc((double)max_dim * ratio);
    } else {
        newH = max_dim;
        newW = trunc((double)max_dim / ratio);
    }
    return newW >= 1 && newH >= 1;
}

int icl_downsize_dims_checked(const char *name, int w, int h, int max_dim, int &nw, int &nh)
{
    if (!icl_downsize_dims(h, w, max_dim, nw, nh) || nw > 65535 || nh > 65535)
        return icl_fail(nullptr, ICL_ERR_ARG, "failed to resize image: %s. %d x %d at max_dim %d gives %d x %d", name, w, h, max_dim, nw, nh);
    return ICL_OK;
}

// the bytes of a source as they stand (the passthrough never decodes them)
int icl_src_bytes(const ingest_src &src, const char *name, std::vector<uint8_t> &file, const uint8_t *&data, size_t &len)
{
    if (!src.path) {
        if (!src.data || src.bytes <= 0) return icl_fail(nullptr, ICL_ERR_IO, "failed to read image: %s. empty image buffer", name);
        data = src.data;
        len = (size_t)src.bytes;
        return ICL_OK;
    }
    std::unique_ptr<FILE, int (*)(FILE *)> f(fopen(src.path, "rb"), fclose);
    if (!f) return icl_fail(nullptr, ICL_ERR_IO, "failed to read image: %s. The image file might be corrupt or unreadable", name);
    fseek(f.get(), 0, SEEK_END);
    const long sz = ftell(f.get());
    fseek(f.get(), 0, SEEK_SET);
    file.resize((size_t)std::max<long>(sz, 0));
    if (sz < 0 || fread(file.data(), 1, file.size(), f.get()) != file.size())
        return icl_fail(nullptr, ICL_ERR_IO, "failed to read image: %s. The image file might be corrupt or unreadable", name);
    data = file.data();
    len = file.size();
    return ICL_OK;
}

int icl_downsize_src(const ingest_src &src, int64_t max_bytes, int max_dim, std::vector<uint8_t> &out, int32_t *info)
{
    char nbuf[96];
    const char *name = ingest_src_name(src, nbuf, sizeof nbuf);
    int32_t inf[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> file;
    const uint8_t *data = nullptr;
    size_t len = 0;
    ICL_TRY(icl_src_bytes(src, name, file, data, len));
    if ((int64_t)len <= max_bytes) { // :182-184
        out.assign(data, data + len);
        inf[0] = 1;
        if (info) memcpy(info, inf, sizeof inf);
        return ICL_OK;
    }
    std::vector<uint8_t> px;
    int w = 0, h = 0;
    const ingest_src mem{nullptr, data, (int64_t)len, src.index}; // (read once: the decoders take the bytes just measured)
    std::vector<uint8_t> unused;
    const uint8_t *d2;
    size_t l2;
    const int fmt = icl_image_src_read(mem, unused, d2, l2); // (a memory source: the format by its first bytes, nothing copied)
    ICL_TRY(icl_image_decode(nullptr, mem, name, fmt, data, len, px, w, h));
    int nw = 0, nh = 0;
    ICL_TRY(icl_downsize_dims_checked(name, w, h, max_dim, nw, nh));
    icl_jenc_tables T;
    icl_jenc_make_tables(ICL_DOWNSIZE_QUALITY, T);
    std::vector<uint8_t> small((size_t)nw * nh * 3);
    icl_resize_bilinear_u8(px.data(), w, h, small.data(), nw, nh);
    icl_jenc_encode_host(small.data(), nw, nh, T, out);
    inf[1] = w;
    inf[2] = h;
    inf[5] = 1;
    if ((int64_t)out.size() > max_bytes && nw / 2 >= 1 && nh / 2 >= 1) { // :239-256: once more at half the size, returned whatever its size
        nw /= 2;
        nh /= 2;
        small.resize((size_t)nw * nh * 3);
        icl_resize_bilinear_u8(px.data(), w, h, small.data(), nw, nh);
        icl_jenc_encode_host(small.data(), nw, nh, T, out);
        inf[5] = 2;
    }
    inf[3] = nw;
    inf[4] = nh;
    if (info) memcpy(info, inf, sizeof inf);
    return ICL_OK;
}

static int downsize_image(const ingest_src &src, int64_t max_bytes, int32_t max_dim, uint8_t *out, int64_t cap, int64_t *bytes, int32_t *info, const char *what)
{
    if (!bytes || max_bytes < 0 || max_dim < 1) return icl_fail(nullptr, ICL_ERR_ARG, "%s: bad argument", what);
    return no_throw(nullptr, what, [&]() -> int {
        std::vector<uint8_t> file;
        ICL_TRY(icl_downsize_src(src, max_bytes, max_dim, file, info));
        return icl_deliver_bytes(file, out, cap, bytes, what);
    });
}

extern "C" int icl_downsize_image_file(const char *path, int64_t max_bytes, int32_t max_dim, uint8_t *out, int64_t cap, int64_t *bytes, int32_t *info)
{
    if (!path) return icl_fail(nullptr, ICL_ERR_ARG, "icl_downsize_image_file: bad argument");
    return downsize_image(ingest_src{path, nullptr, 0, 0}, max_bytes, max_dim, out, cap, bytes, info, "icl_downsize_image_file");
}

extern "C" int icl_downsize_image_mem(const uint8_t *data, int64_t in_bytes, int64_t max_bytes, int32_t max_dim, uint8_t *out, int64_t cap, int64_t *bytes, int32_t *info)
{
    return downsize_image(ingest_src{nullptr, data, in_bytes, 0}, max_bytes, max_dim, out, cap, bytes, info, "icl_downsize_image_mem");
}
