// jpeg_decode.hip -- host-only JPEG decoder (baseline and progressive) for the image-ingest step of the hot path.
//
// Replaces gocv.IMRead(imagePath, IMReadColor) in PreprocessImage
//   (/root/reference/internal/embeddings/embeddings.go:50), i.e. OpenCV imgcodecs -> libjpeg(-turbo) with its default
// settings: integer "islow" IDCT, "fancy" (triangle) chroma upsampling and the fixed-point YCbCr->RGB tables.  Those
// three algorithms are public (IJG libjpeg: jidctint.c, jdsample.c, jdcolor.c) and are restated in ingest_pixels.h so that
// decoded pixels are bit-identical to libjpeg-turbo's (checked against Pillow's bundled libjpeg-turbo in
// tests/test_jpeg_decode.py).  Supported: 8-bit baseline / extended sequential (SOF0, SOF1) and PROGRESSIVE (SOF2:
// spectral selection + successive approximation, ITU T.81 annex G) Huffman streams, interleaved or one scan per
// component, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 / 4:1:1 sampling (luma 1x1, 2x1, 2x2, 1x2, 4x1 or 1x4 over 1x1 chroma),
// restart intervals, JFIF / Adobe-transform markers.
// Every scan decodes into per-component coefficient arrays; dequantisation + IDCT run once after the last scan.
// Two stages (jpeg_stage.h): stage A parses the file and runs the entropy decoder (every check of a hostile file is made
// here); stage B dequantises, runs the IDCT, upsamples the chroma and converts the colour.  jpeg_gpu.hip runs stage B on the GPU
// with the same per-sample rules (ingest_pixels.h).
// Arithmetic coding, lossless, 12-bit, CMYK and every other sampling (4:1:0, subsampled luma, ...) return ICL_ERR_UNSUPPORTED.
#include "icl_common.h"
#include "ingest_pixels.h"
#include "jpeg_entropy.h"
#include "jpeg_stage.h"

#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

namespace {

struct huff_table {
    bool present = false;
    uint8_t bits[17] = {0};
    uint8_t vals[256] = {0};
    int mincode[17], maxcode[18], valptr[17];
    uint16_t fast[512]; // 9-bit lookahead: (length << 8) | symbol, 0 = not resolvable in 9 bits
    void build()
    {
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = k;
            mincode[l] = code;
            code += bits[l];
            k += bits[l];
            maxcode[l] = bits[l] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        memset(fast, 0, sizeof fast);
        code = 0;
        k = 0;
        for (int l = 1; l <= 9; ++l) {
            for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
                const int lo = code << (9 - l), hi = lo + (1 << (9 - l));
                for (int c = lo; c < hi; ++c) fast[c] = (uint16_t)((l << 8) | vals[k]);
            }
            code <<= 1;
        }
    }
};

struct bit_reader {
    const uint8_t *p, *end;
    uint32_t acc = 0;
    int nbits = 0;
    bool hit_marker = false;
    void fill()
    {
        while (nbits <= 24) {
            int b = 0;
            if (!hit_marker && p < end) {
                b = *p++;
                if (b == 0xFF) {
                    if (p < end && *p == 0x00) ++p;                 // stuffed zero
                    else { hit_marker = true; --p; b = 0; }         // a real marker: feed zeros from here on
                }
            }
            acc |= (uint32_t)b << (24 - nbits);
            nbits += 8;
        }
    }
    int peek(int n) { fill(); return (int)(acc >> (32 - n)); }
    void skip(int n) { acc <<= n; nbits -= n; }
    int get(int n)
    {
        if (n == 0) return 0;
        const int v = peek(n);
        skip(n);
        return v;
    }
    void reset() { acc = 0; nbits = 0; hit_marker = false; }
};

inline int huff_decode(bit_reader &br, const huff_table &t)
{
    const int look = br.peek(9);
    const uint16_t f = t.fast[look];
    if (f) {
        br.skip(f >> 8);
        return f & 0xff;
    }
    int code = br.peek(16), l = 10;
    for (; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (t.maxcode[l] >= 0 && c <= t.maxcode[l] && c >= t.mincode[l]) {
            br.skip(l);
            return t.vals[t.valptr[l] + c - t.mincode[l]];
        }
    }
    return -1;
}

inline int extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// IJG jidctint.c jpeg_idct_islow (ingest_pixels.h) on one block.  coef is dequantised, natural order.
void idct_islow(const int *coef, uint8_t *out, int stride)
{
    int ws[64], px[8];
    for (int c = 0; c < 8; ++c) {
        const int *in = coef + c;
        if (!(in[8] | in[16] | in[24] | in[32] | in[40] | in[48] | in[56])) { // all AC terms zero: the column is dc << PASS1_BITS
            const int dc = in[0] * (1 << ICL_IDCT_P1);
            for (int r = 0; r < 8; ++r) ws[c + 8 * r] = dc;
            continue;
        }
        icl_idct_islow_col(in, ws + c);
    }
    for (int r = 0; r < 8; ++r) {
        icl_idct_islow_row(ws + 8 * r, px);
        uint8_t *o = out + (size_t)r * stride;
        for (int k = 0; k < 8; ++k) o[k] = (uint8_t)px[k];
    }
}

void copy_table(const huff_table &t, icl_je_table &o)
{
    memcpy(o.fast, t.fast, sizeof o.fast);
    memcpy(o.mincode, t.mincode, sizeof o.mincode);
    memcpy(o.maxcode, t.maxcode, sizeof o.maxcode);
    memcpy(o.valptr, t.valptr, sizeof o.valptr);
    memcpy(o.vals, t.vals, sizeof o.vals);
    o.mincode[0] = o.maxcode[0] = o.valptr[0] = 0; // (index 0 is never built, never read)
}

// The entropy-coded segment as bit_reader::fill sees it: FF 00 -> FF; an RSTn ends an interval; the first FF followed by anything else
// (or the end of the data) ends the segment.  Every interval is padded with zeros to whole subsequences of sb bytes.  Returns where
// the segment ended.
const uint8_t *split_stream(const uint8_t *q, const uint8_t *e, size_t sb, icl_jpeg_a0 &A)
{
    std::vector<uint8_t> &st = A.stream;
    st.clear();
    A.intervals.clear();
    st.reserve((size_t)(e - q) + sb);
    size_t istart = 0;
    uint32_t first_sub = 0;
    auto close_interval = [&]() {
        const size_t nbytes = st.size() - istart;
        const size_t nsub = std::max<size_t>(1, (nbytes + sb - 1) / sb);
        A.intervals.push_back(icl_je_interval{first_sub, (uint32_t)(nbytes * 8)});
        first_sub += (uint32_t)nsub;
        st.resize(istart + nsub * sb, 0);
        istart = st.size();
    };
    for (;;) {
        const uint8_t *ff = q < e ? (const uint8_t *)memchr(q, 0xFF, (size_t)(e - q)) : nullptr;
        if (!ff) {
            if (q < e) st.insert(st.end(), q, e);
            q = e;
            break;
        }
        st.insert(st.end(), q, ff);
        q = ff;
        if (q + 1 < e && q[1] == 0x00) {
            st.push_back(0xFF);
            q += 2;
        } else if (q + 1 < e && q[1] >= 0xD0 && q[1] <= 0xD7) {
            close_interval();
            q += 2;
        } else {
            break;
        }
    }
    close_interval();
    A.scan.nsub = first_sub;
    return q;
}

} // namespace

constexpr int A0_NOT_QUALIFIED = -1; // stage A0's parser on a file the GPU entropy decoder does not take (stage_a below)
static int jpeg_stage_a_impl(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, icl_jpeg_coefs &J, icl_jpeg_a0 *a0 = nullptr, int sub_bits = 0);
static int jpeg_stage_b_impl(const icl_jpeg_coefs &J, std::vector<uint8_t> &rgb);

// No C++ exception may cross the C ABI (cgo / ctypes would std::terminate the host process): allocation failures become status codes here.
template <class F> static int guarded(icl_ctx *ctx, const char *path, F body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return icl_fail(ctx, ICL_ERR_NOMEM, "failed to read image: %s. Out of host memory while decoding", path);
    } catch (...) {
        return icl_fail(ctx, ICL_ERR_IO, "failed to read image: %s. Decoder error", path);
    }
}

// Decodes a JPEG file held in memory to interleaved RGB.  rgb is resized to w*h*3.
// orient receives the EXIF orientation tag (1..8; 1 when absent): cv::imread applies it after decoding (embeddings.go:50
// passes IMReadColor without IMREAD_IGNORE_ORIENTATION), the caller does the same (image_io.hip icl_apply_exif_orientation).
int icl_jpeg_decode(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, std::vector<uint8_t> &rgb, int &W, int &H, int &orient)
{
    orient = 1;
    return guarded(ctx, path, [&]() -> int {
        icl_jpeg_coefs J;
        const int rc = jpeg_stage_a_impl(ctx, data, len, path, J);
        W = J.W;
        H = J.H;
        if (rc) return rc;
        orient = J.orient;
        return jpeg_stage_b_impl(J, rgb);
    });
}

int icl_jpeg_stage_a(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, icl_jpeg_coefs &J)
{
    J.orient = 1;
    return guarded(ctx, path, [&]() -> int { return jpeg_stage_a_impl(ctx, data, len, path, J); });
}

int icl_jpeg_stage_a0(const uint8_t *data, size_t len, const char *path, int sub_bits, icl_jpeg_coefs &J, icl_jpeg_a0 &A, bool &qualifies)
{
    qualifies = false;
    J.orient = 1;
    if (sub_bits < 64 || sub_bits % 32 != 0 || sub_bits > (1 << 20)) return ICL_ERR_ARG;
    try {
        const int rc = jpeg_stage_a_impl(nullptr, data, len, path, J, &A, sub_bits);
        if (rc == A0_NOT_QUALIFIED) return ICL_OK;
        qualifies = rc == ICL_OK;
        return rc;
    } catch (...) {
        return ICL_ERR_NOMEM;
    }
}

namespace {

struct host_fetch {
    const uint8_t *s;
    size_t nwords;
    uint32_t operator()(uint32_t w) const
    {
        if (w >= nwords) return 0;
        uint32_t v;
        memcpy(&v, s + 4 * (size_t)w, 4);
        return __builtin_bswap32(v);
    }
};

struct host_sink { // coefficients as stage A stores them: natural order, the DC value as (int16_t) of the int predictor
    const icl_je_scan &S;
    std::vector<int16_t> *coefs;
    int64_t first;
    uint32_t pred[3];
    int64_t cur = -1;
    int cur_c = 0;
    int16_t *base = nullptr;
    int16_t *at(uint32_t k)
    {
        if ((int64_t)k != cur) {
            int64_t idx;
            cur = k;
            base = icl_je_block_place(S, first + k, cur_c, idx) ? coefs[cur_c].data() + idx * 64 : nullptr;
        }
        return base;
    }
    void dc(uint32_t k, int, int diff) // the component is the one of the block's place
    {
        if (int16_t *b = at(k)) {
            pred[cur_c] += (uint32_t)diff;
            b[0] = (int16_t)(int32_t)pred[cur_c];
        }
    }
    void ac(uint32_t k, int z, int v)
    {
        if (int16_t *b = at(k)) b[icl_zigzag[z & 63]] = (int16_t)v;
    }
};

} // namespace

void icl_je_host_decode(const icl_jpeg_a0 &A, std::vector<int16_t> coefs[3], bool &accepted, int &rounds)
{
    const icl_je_scan &S = A.scan;
    const uint32_t nsub = S.nsub, sb = (uint32_t)S.sub_bits;
    const int nluma = S.ncomp == 1 ? 1 : S.hs * S.vs;
    accepted = false;
    rounds = 0;
    if (nsub == 0 || A.intervals.empty() || A.stream.size() < (size_t)nsub * (sb / 8)) return;
    host_fetch fetch{A.stream.data(), A.stream.size() / 4};
    std::vector<icl_je_sub> sub(nsub);
    std::vector<uint32_t> ivl(nsub);
    for (size_t k = 0; k < A.intervals.size(); ++k) {
        const uint32_t a = A.intervals[k].first_sub, b = k + 1 < A.intervals.size() ? A.intervals[k + 1].first_sub : nsub;
        for (uint32_t i = a; i < b && i < nsub; ++i) ivl[i] = (uint32_t)k;
    }
    auto decode = [&](uint32_t i, auto &sink) {
        const icl_je_interval &I = A.intervals[ivl[i]];
        const uint32_t j = i - I.first_sub, start = j * sb, end = std::min<uint64_t>((uint64_t)start + sb, I.nbits);
        icl_je_result r;
        icl_je_decode_sub(A.tables, S.ncomp, nluma, S.bpm, S.uniform != 0, fetch, I.first_sub * (sb / 32), I.nbits, start, (uint32_t)end, sub[i].entry_p, sub[i].entry_bz, r, sink);
        sub[i].exit_p = r.p;
        sub[i].exit_bz = r.bz;
        sub[i].n = r.n;
        sub[i].flags = r.flags;
        for (int q = 0; q < 6; ++q) sub[i].dcsum[q] = r.dcsum[q];
    };
    // ---- the synchronisation launches: workgroups of ICL_JE_WG subsequences, rounds inside, boundaries between launches ----
    const uint32_t nwg = (nsub + ICL_JE_WG - 1) / ICL_JE_WG;
    std::vector<uint32_t> bound[2] = {std::vector<uint32_t>(2 * (size_t)nwg), std::vector<uint32_t>(2 * (size_t)nwg)};
    std::vector<uint32_t> todo, np, nbz;
    icl_je_no_sink none;
    for (int l = 0; l < ICL_JE_LAUNCHES; ++l)
        for (uint32_t wg = 0; wg < nwg; ++wg) {
            const uint32_t lo = wg * ICL_JE_WG, hi = std::min(nsub, lo + ICL_JE_WG);
            for (uint32_t i = lo; i < hi; ++i) {
                const uint32_t j = i - A.intervals[ivl[i]].first_sub;
                if (l == 0) { // the guess: a block starts at the subsequence's first bit (true for j == 0)
                    sub[i].entry_p = j * sb;
                    sub[i].entry_bz = 0;
                    decode(i, none);
                } else if (i == lo && j > 0 && wg > 0) {
                    const uint32_t p = bound[(l - 1) & 1][2 * (wg - 1)], bz = bound[(l - 1) & 1][2 * (wg - 1) + 1];
                    if (p != sub[i].entry_p || bz != sub[i].entry_bz) {
                        sub[i].entry_p = p;
                        sub[i].entry_bz = bz;
                        decode(i, none);
                    }
                }
            }
            for (int r = 1; r <= ICL_JE_ROUNDS; ++r) {
                todo.clear();
                np.clear();
                nbz.clear();
                for (uint32_t i = lo + 1; i < hi; ++i)
                    if (i != A.intervals[ivl[i]].first_sub && (sub[i].entry_p != sub[i - 1].exit_p || sub[i].entry_bz != sub[i - 1].exit_bz)) {
                        todo.push_back(i);
                        np.push_back(sub[i - 1].exit_p);
                        nbz.push_back(sub[i - 1].exit_bz);
                    }
                if (todo.empty()) break;
                rounds = std::max(rounds, r);
                for (size_t t = 0; t < todo.size(); ++t) {
                    sub[todo[t]].entry_p = np[t];
                    sub[todo[t]].entry_bz = nbz[t];
                }
                for (uint32_t i : todo) decode(i, none);
            }
            bound[l & 1][2 * wg] = sub[hi - 1].exit_p;
            bound[l & 1][2 * wg + 1] = sub[hi - 1].exit_bz;
        }
    // ---- check + prefix sums ----
    bool ok = icl_je_scan_ok(S);
    int64_t blocks = 0;
    uint32_t pred[3] = {0, 0, 0};
    for (uint32_t i = 0; i < nsub && ok; ++i) {
        const uint32_t k = ivl[i];
        const icl_je_interval &I = A.intervals[k];
        const uint32_t j = i - I.first_sub;
        if (j == 0) pred[0] = pred[1] = pred[2] = 0;
        sub[i].first_block = (uint32_t)blocks;
        for (int c = 0; c < 3; ++c) sub[i].dcpred[c] = (int32_t)pred[c];
        ok = ok && blocks < ((int64_t)1 << 31) && icl_je_sub_ok(S, k, j, sub[i], i ? sub[i - 1].exit_p : 0, i ? sub[i - 1].exit_bz : 0);
        const bool last = i + 1 == nsub || ivl[i + 1] != k;
        if (last) ok = ok && icl_je_interval_end_ok(I.nbits, sub[i]);
        blocks += sub[i].n;
        for (int q = 0; q < S.bpm && q < 6; ++q) pred[icl_je_phase_comp(S.ncomp, nluma, S.bpm, sub[i].first_block, q)] += (uint32_t)sub[i].dcsum[q];
    }
    ok = ok && icl_je_total_ok(S, blocks);
    if (!ok) return;
    // ---- write pass ----
    for (int c = 0; c < 3; ++c) coefs[c].assign(c < S.ncomp ? (size_t)S.wblocks[c] * S.hblocks[c] * 64 : 0, 0);
    for (uint32_t i = 0; i < nsub; ++i) {
        host_sink sink{S, coefs, (int64_t)sub[i].first_block, {(uint32_t)sub[i].dcpred[0], (uint32_t)sub[i].dcpred[1], (uint32_t)sub[i].dcpred[2]}};
        decode(i, sink);
    }
    accepted = true;
}

// stage A0 + host loop on a file in memory (the sanitizer harness under scratch/asan_jpeg/): 1 accepted, 0 rejected, -1 does not qualify
int icl_jpeg_entropy_host_check(const uint8_t *data, size_t len, const char *path)
{
    try {
        icl_jpeg_coefs J;
        icl_jpeg_a0 A;
        std::vector<int16_t> coefs[3];
        bool qualifies = false, accepted = false;
        int rounds = 0;
        (void)icl_jpeg_stage_a0(data, len, path, ICL_JE_SUB_BITS, J, A, qualifies);
        if (!qualifies) return -1;
        icl_je_host_decode(A, coefs, accepted, rounds);
        return accepted ? 1 : 0;
    } catch (...) {
        return -1;
    }
}

int icl_jpeg_stage_b(icl_ctx *ctx, const icl_jpeg_coefs &J, const char *path, std::vector<uint8_t> &rgb)
{
    return guarded(ctx, path, [&]() -> int { return jpeg_stage_b_impl(J, rgb); });
}

// EXIF (APP1 "Exif\0\0" + TIFF header): orientation tag 0x0112 of IFD0, 1..8; anything malformed reads as 1.
static int exif_orientation(const uint8_t *s, size_t sl)
{
    if (sl < 14 || memcmp(s, "Exif\0\0", 6) != 0) return 1;
    const uint8_t *t = s + 6;
    const size_t tl = sl - 6;
    const bool le = t[0] == 'I' && t[1] == 'I', be = t[0] == 'M' && t[1] == 'M';
    if (!le && !be) return 1;
    auto u16 = [&](size_t o) -> unsigned { return le ? (unsigned)(t[o] | (t[o + 1] << 8)) : (unsigned)((t[o] << 8) | t[o + 1]); };
    auto u32 = [&](size_t o) -> unsigned {
        return le ? (unsigned)t[o] | ((unsigned)t[o + 1] << 8) | ((unsigned)t[o + 2] << 16) | ((unsigned)t[o + 3] << 24)
                  : ((unsigned)t[o] << 24) | ((unsigned)t[o + 1] << 16) | ((unsigned)t[o + 2] << 8) | (unsigned)t[o + 3];
    };
    if (u16(2) != 42) return 1;
    const size_t ifd = u32(4);
    if (ifd + 2 > tl) return 1;
    const unsigned nent = u16(ifd);
    for (unsigned e = 0; e < nent; ++e) {
        const size_t o = ifd + 2 + (size_t)e * 12;
        if (o + 12 > tl) return 1;
        if (u16(o) == 0x0112) {
            const unsigned v = u16(o + 8); // type SHORT, count 1: the value sits in the first two bytes of the value field
            return (u16(o + 2) == 3 && v >= 1 && v <= 8) ? (int)v : 1;
        }
    }
    return 1;
}

namespace {

// Where the marker loop goes on after a scan: the next real marker (FF followed by anything but 00, RSTn or another FF) at or after q,
// or the last byte when there is none.  split_stream ends the entropy-coded segment earlier or at the same place, at the first FF not
// followed by 00 or RSTn: from there this search also passes FF FF fill bytes and whatever a damaged file holds before its next marker.
const uint8_t *ecs_end(const uint8_t *q, const uint8_t *end)
{
    while (q + 1 < end && !(q[0] == 0xFF && q[1] != 0x00 && !(q[1] >= 0xD0 && q[1] <= 0xD7) && q[1] != 0xFF)) ++q;
    return q;
}

// a validated scan header: the frame's components it carries, its spectral band and successive-approximation bits
struct scan_header {
    int ns = 0, sc[3] = {0, 0, 0};
    int Ss = 0, Se = 0, Ah = 0, Al = 0;
};

// what a scan header sets for a frame component, and its DC predictor
struct comp_scan {
    int td = 0, ta = 0;
    int pred = 0;
};

// The entropy decoder of one scan.  One block of the scan into the coefficient array, by the scan's kind (T.81 F.2.2 sequential, G.1.2
// progressive; the AC refinement pass follows the structure of IJG jdphuff.c decode_mcu_AC_refine); false: corrupt data.
struct scan_state {
    bit_reader br;
    const huff_table *dc, *ac; // the four tables of each class
    int Ss, Se, Al;
    int eobrun = 0;

    bool sequential(comp_scan &k, int16_t *cf)
    {
        const int t = huff_decode(br, dc[k.td]);
        if (t < 0 || t > 15) return false;
        k.pred += t ? extend(br.get(t), t) : 0;
        cf[0] = (int16_t)k.pred;
        for (int i = 1; i < 64;) {
            const int rs = huff_decode(br, ac[k.ta]);
            if (rs < 0) return false;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r == 15) { i += 16; continue; }
                break;
            }
            i += r;
            if (i > 63) return false;
            cf[icl_zigzag[i]] = (int16_t)extend(br.get(sz), sz);
            ++i;
        }
        return true;
    }
    bool dc_first(comp_scan &k, int16_t *cf)
    {
        const int t = huff_decode(br, dc[k.td]);
        if (t < 0 || t > 15) return false;
        k.pred += t ? extend(br.get(t), t) : 0;
        cf[0] = (int16_t)(k.pred * (1 << Al));
        return true;
    }
    bool dc_refine(comp_scan &, int16_t *cf) // one more bit
    {
        if (br.get(1)) cf[0] = (int16_t)(cf[0] | (1 << Al));
        return true;
    }
    bool ac_first(comp_scan &k, int16_t *cf)
    {
        if (eobrun > 0) { --eobrun; return true; }
        for (int i = Ss; i <= Se;) {
            const int rs = huff_decode(br, ac[k.ta]);
            if (rs < 0) return false;
            const int r = rs >> 4, sz = rs & 15;
            if (sz == 0) {
                if (r == 15) { i += 16; continue; }
                eobrun = (1 << r) - 1;
                if (r) eobrun += br.get(r);
                break;
            }
            i += r;
            if (i > Se) return false;
            cf[icl_zigzag[i]] = (int16_t)(extend(br.get(sz), sz) * (1 << Al));
            ++i;
        }
        return true;
    }
    bool ac_refine(comp_scan &k, int16_t *cf)
    {
        const int p1 = 1 << Al, m1 = -(1 << Al);
        int i = Ss;
        auto refine = [&](int16_t &c) {
            if (br.get(1) && (c & p1) == 0) c = (int16_t)(c + (c >= 0 ? p1 : m1));
        };
        if (eobrun == 0) {
            for (; i <= Se; ++i) {
                const int rs = huff_decode(br, ac[k.ta]);
                if (rs < 0) return false;
                int r = rs >> 4, sv = rs & 15;
                if (sv) {
                    if (sv != 1) return false;
                    sv = br.get(1) ? p1 : m1;
                } else if (r != 15) { // EOBr: the rest of this block (and eobrun-1 more) only gets correction bits
                    eobrun = 1 << r;
                    if (r) eobrun += br.get(r);
                    break;
                }
                // skip r ZERO-history coefficients (ZRL: 16), refining the non-zero ones passed on the way
                for (; i <= Se; ++i) {
                    int16_t &c = cf[icl_zigzag[i]];
                    if (c != 0) refine(c);
                    else if (--r < 0) break;
                }
                if (sv) {
                    if (i > Se) return false;
                    cf[icl_zigzag[i]] = (int16_t)sv;
                }
            }
        }
        if (eobrun > 0) {
            for (; i <= Se; ++i) {
                int16_t &c = cf[icl_zigzag[i]];
                if (c != 0) refine(c);
            }
            --eobrun;
        }
        return true;
    }
};

// Stage A: markers, tables, frame and scan headers, and every scan's entropy-coded data into J.comp[c].coefs.  The parser owns what
// holds from one marker to the next; each marker's member reads its segment (s, sl) alone.  Frame geometry, W / H and the orientation
// go to J as they are read (no caller reads J after a failure); ncomp, qt and is_rgb are committed at the end.
// a0 != nullptr: stage A0.  The same marker loop, but the first scan of a file the GPU entropy decoder takes is not decoded:
// its tables, geometry and unstuffed stream go to *a0.  Returns A0_NOT_QUALIFIED for every other file.
struct stage_a {
    icl_ctx *ctx; // the call: where messages go, what they call the image, its bytes, where the result goes
    const char *path;
    const uint8_t *data;
    size_t len;
    icl_jpeg_coefs &J;
    icl_jpeg_a0 *a0;
    int sub_bits;
    // what holds from one marker to the next
    uint16_t qt[4][64];
    bool qt_ok[4] = {false, false, false, false};
    huff_table dc[4], ac[4];
    comp_scan comp[3];
    int ncomp = 0, restart = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0, nscans = 0;
    bool have_sof = false, adobe = false, progressive = false;
    int adobe_transform = -1;

    int fail(int code, const char *what) const { return icl_fail(ctx, code, "failed to read image: %s. %s", path, what); }

    int dqt(const uint8_t *s, size_t sl)
    {
        size_t i = 0;
        while (i < sl) {
            const int pq = s[i] >> 4, tq = s[i] & 15;
            ++i;
            if (tq > 3 || i + (pq ? 128 : 64) > sl) return fail(ICL_ERR_IO, "Bad quantization table");
            for (int k = 0; k < 64; ++k) {
                qt[tq][icl_zigzag[k]] = pq ? (uint16_t)((s[i] << 8) | s[i + 1]) : s[i];
                i += pq ? 2 : 1;
            }
            qt_ok[tq] = true;
        }
        return ICL_OK;
    }

    int dht(const uint8_t *s, size_t sl)
    {
        size_t i = 0;
        while (i + 17 <= sl) {
            const int tc = s[i] >> 4, th = s[i] & 15;
            if (tc > 1 || th > 3) return fail(ICL_ERR_IO, "Bad Huffman table");
            huff_table &t = tc ? ac[th] : dc[th];
            int total = 0;
            t.bits[0] = 0;
            for (int l = 1; l <= 16; ++l) { t.bits[l] = s[i + l]; total += t.bits[l]; }
            i += 17;
            if (total > 256 || i + total > sl) return fail(ICL_ERR_IO, "Bad Huffman table");
            // the counts must form a prefix code (as IJG jdhuff.c checks): at every length the codes handed out so
            // far fit in l bits -- otherwise build()'s lookahead index runs past fast[512] (over-subscribed table)
            for (int l = 1, code = 0; l <= 16; ++l) {
                code += t.bits[l];
                if (code > (1 << l)) return fail(ICL_ERR_IO, "Bad Huffman table");
                code <<= 1;
            }
            memcpy(t.vals, s + i, (size_t)total);
            i += total;
            t.present = true;
            t.build();
        }
        return ICL_OK;
    }

    int sof(int m, const uint8_t *s, size_t sl) // SOF0 / SOF1 / SOF2
    {
        int &W = J.W, &H = J.H;
        icl_jpeg_component *k = J.comp;
        if (have_sof) return fail(ICL_ERR_IO, "Second frame header");
        if (sl < 6 || s[0] != 8) return fail(ICL_ERR_UNSUPPORTED, "Only 8-bit JPEG is decoded");
        progressive = m == 0xC2;
        H = (s[1] << 8) | s[2];
        W = (s[3] << 8) | s[4];
        ncomp = s[5];
        if ((ncomp != 1 && ncomp != 3) || sl < (size_t)(6 + 3 * ncomp) || W <= 0 || H <= 0 || W > 32768 || H > 32768)
            return fail(ICL_ERR_UNSUPPORTED, "Only 1- or 3-component JPEG is decoded");
        // sizes come from the file: bound what they make us allocate (coefficients + planes + RGB, ~11 B per pixel)
        if ((int64_t)W * H > ICL_JPEG_MAX_PIXELS) return fail(ICL_ERR_UNSUPPORTED, "JPEG larger than 64 Mpixel is not decoded");
        for (int c = 0; c < ncomp; ++c) {
            k[c].id = s[6 + 3 * c];
            k[c].h = s[7 + 3 * c] >> 4;
            k[c].v = s[7 + 3 * c] & 15;
            k[c].tq = s[8 + 3 * c];
        }
        if (ncomp == 1) k[0].h = k[0].v = 1;
        if (ncomp == 3 && !(k[1].h == 1 && k[1].v == 1 && k[2].h == 1 && k[2].v == 1 && icl_luma_sampling_ok(k[0].h, k[0].v))) {
            char what[160];
            snprintf(what, sizeof what, "Sampling %dx%d,%dx%d,%dx%d is not decoded (only luma 1x1, 2x1, 2x2, 1x2, 4x1 or 1x4 over 1x1 chroma)", k[0].h, k[0].v,
                     k[1].h, k[1].v, k[2].h, k[2].v);
            return fail(ICL_ERR_UNSUPPORTED, what);
        }
        for (int c = 0; c < ncomp; ++c) {
            hmax = std::max(hmax, k[c].h);
            vmax = std::max(vmax, k[c].v);
        }
        mcux = (W + 8 * hmax - 1) / (8 * hmax);
        mcuy = (H + 8 * vmax - 1) / (8 * vmax);
        for (int c = 0; c < ncomp; ++c) {
            k[c].wblocks = mcux * k[c].h;
            k[c].hblocks = mcuy * k[c].v;
            k[c].dw = (W * k[c].h + hmax - 1) / hmax;
            k[c].dh = (H * k[c].v + vmax - 1) / vmax;
            if (!a0) k[c].coefs.assign((size_t)k[c].wblocks * k[c].hblocks * 64, 0);
        }
        have_sof = true;
        return ICL_OK;
    }

    void dri(const uint8_t *s, size_t sl)
    {
        if (sl >= 2) restart = (s[0] << 8) | s[1];
    }
    void app1(const uint8_t *s, size_t sl) // the first APP1/Exif segment decides, as in OpenCV's ExifReader
    {
        if (J.orient == 1) J.orient = exif_orientation(s, sl);
    }
    void app14(const uint8_t *s, size_t sl)
    {
        if (sl >= 12 && !memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
    }

    // SOS: one scan (a baseline file has one or ncomp of them, a progressive file many).  The entropy-coded segment follows the header
    // at s + sl; next receives the marker that ended it.
    int sos(const uint8_t *s, size_t sl, const uint8_t *&next)
    {
        if (!have_sof) return fail(ICL_ERR_IO, "Scan before frame header");
        if (sl < 1) return fail(ICL_ERR_IO, "Bad scan header");
        scan_header h;
        h.ns = s[0];
        if (h.ns < 1 || h.ns > ncomp || sl < (size_t)(1 + 2 * h.ns + 3)) return fail(ICL_ERR_IO, "Bad scan header");
        for (int i = 0; i < h.ns; ++i) {
            int ci = -1;
            for (int c = 0; c < ncomp; ++c)
                if (J.comp[c].id == s[1 + 2 * i]) ci = c;
            if (ci < 0) return fail(ICL_ERR_IO, "Bad scan component");
            comp[ci].td = s[2 + 2 * i] >> 4;
            comp[ci].ta = s[2 + 2 * i] & 15;
            h.sc[i] = ci;
        }
        h.Ss = s[1 + 2 * h.ns];
        h.Se = s[2 + 2 * h.ns];
        h.Ah = s[3 + 2 * h.ns] >> 4;
        h.Al = s[3 + 2 * h.ns] & 15;
        if (progressive) {
            const bool ok = h.Ss <= h.Se && h.Se <= 63 && h.Al <= 13 && (h.Ss == 0 ? h.Se == 0 : h.ns == 1) && (h.Ah == 0 || h.Ah == h.Al + 1);
            if (!ok) return fail(ICL_ERR_IO, "Bad progressive scan parameters");
        } else if (h.Ss != 0 || h.Se != 63 || h.Ah != 0 || h.Al != 0) {
            return fail(ICL_ERR_IO, "Bad sequential scan parameters");
        }
        for (int i = 0; i < h.ns; ++i) {
            comp_scan &k = comp[h.sc[i]];
            const bool need_dc = h.Ss == 0 && h.Ah == 0, need_ac = h.Se > 0;
            if (k.td > 3 || k.ta > 3 || (need_dc && !dc[k.td].present) || (need_ac && !ac[k.ta].present)) return fail(ICL_ERR_IO, "Missing table");
            k.pred = 0;
        }
        const int rc = a0 ? capture_scan(h, s + sl, next) : decode_scan(h, s + sl, next);
        if (rc == ICL_OK) ++nscans;
        return rc;
    }

    // stage A0: one sequential scan that carries all components in frame order, or the file takes the usual route
    int capture_scan(const scan_header &h, const uint8_t *ecs, const uint8_t *&next)
    {
        if (progressive || nscans > 0 || h.ns != ncomp || len >= ((size_t)1 << 28)) return A0_NOT_QUALIFIED;
        for (int i = 0; i < h.ns; ++i)
            if (h.sc[i] != i) return A0_NOT_QUALIFIED;
        icl_je_scan &S = a0->scan;
        S = icl_je_scan();
        S.ncomp = ncomp;
        S.hs = J.comp[0].h;
        S.vs = J.comp[0].v;
        S.bpm = ncomp == 1 ? 1 : S.hs * S.vs + 2;
        S.mcux = mcux;
        S.mcuy = mcuy;
        S.restart = restart;
        S.sub_bits = sub_bits;
        for (int c = 0; c < ncomp; ++c) {
            S.wblocks[c] = J.comp[c].wblocks;
            S.hblocks[c] = J.comp[c].hblocks;
            copy_table(dc[comp[c].td], a0->tables[2 * c]);
            copy_table(ac[comp[c].ta], a0->tables[2 * c + 1]);
        }
        S.uniform = ncomp == 3 ? 1 : 0;
        for (int c = 1; c < ncomp; ++c)
            if (memcmp(&a0->tables[0], &a0->tables[2 * c], sizeof(icl_je_table)) || memcmp(&a0->tables[1], &a0->tables[2 * c + 1], sizeof(icl_je_table))) S.uniform = 0;
        const uint8_t *q = split_stream(ecs, data + len, (size_t)sub_bits / 8, *a0);
        S.nintervals = (int32_t)a0->intervals.size();
        next = ecs_end(q, data + len);
        return ICL_OK;
    }

    // the decoder of the scan's kind, chosen once, over all its blocks
    int decode_scan(const scan_header &h, const uint8_t *ecs, const uint8_t *&next)
    {
        scan_state S{bit_reader{ecs, data + len}, dc, ac, h.Ss, h.Se, h.Al};
        int rc;
        if (!progressive) rc = walk<&scan_state::sequential>(h, S);
        else if (h.Ss == 0) rc = h.Ah == 0 ? walk<&scan_state::dc_first>(h, S) : walk<&scan_state::dc_refine>(h, S);
        else rc = h.Ah == 0 ? walk<&scan_state::ac_first>(h, S) : walk<&scan_state::ac_refine>(h, S);
        if (rc == ICL_OK) next = ecs_end(S.br.p, data + len);
        return rc;
    }

    // The scan's MCUs in order, with the restart step between intervals.  An interleaved scan (ns > 1) walks the frame's MCUs, h x v
    // blocks of each component; a scan of one component walks that component's own block raster, one block per "MCU".
    template <bool (scan_state::*Block)(comp_scan &, int16_t *)> int walk(const scan_header &h, scan_state &S)
    {
        const bool own = h.ns == 1;
        const icl_jpeg_component &k0 = J.comp[h.sc[0]];
        const int ny = own ? (k0.dh + 7) / 8 : mcuy, nx = own ? (k0.dw + 7) / 8 : mcux;
        int rst_left = restart;
        for (int my = 0; my < ny; ++my)
            for (int mx = 0; mx < nx; ++mx) {
                if (restart && rst_left == 0) {
                    if (!next_interval(S)) return fail(ICL_ERR_IO, "Missing restart marker");
                    rst_left = restart;
                }
                for (int i = 0; i < h.ns; ++i) {
                    icl_jpeg_component &k = J.comp[h.sc[i]];
                    const int bh = own ? 1 : k.v, bw = own ? 1 : k.h;
                    for (int by = 0; by < bh; ++by)
                        for (int bx = 0; bx < bw; ++bx)
                            if (!(S.*Block)(comp[h.sc[i]], k.coefs.data() + ((size_t)(my * bh + by) * k.wblocks + (mx * bw + bx)) * 64))
                                return fail(ICL_ERR_IO, "Corrupt JPEG data");
                }
                if (restart) --rst_left;
            }
        return ICL_OK;
    }

    bool next_interval(scan_state &S) // byte-align, expect RSTn
    {
        const uint8_t *q = S.br.p;
        while (q + 1 < S.br.end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
        if (q + 1 >= S.br.end) return false;
        S.br.p = q + 2;
        S.br.reset();
        for (int c = 0; c < ncomp; ++c) comp[c].pred = 0;
        S.eobrun = 0;
        return true;
    }

    int run()
    {
        if (len < 4 || data[0] != 0xFF || data[1] != 0xD8) return fail(ICL_ERR_IO, "Not a JPEG stream");
        if (a0)
            for (int c = 0; c < 3; ++c) J.comp[c].coefs.clear(); // stage A0 leaves no coefficients
        J.W = J.H = 0;
        size_t pos = 2;
        while (pos + 4 <= len) {
            if (data[pos] != 0xFF) { ++pos; continue; }
            const int m = data[pos + 1];
            if (m == 0xFF) { ++pos; continue; }
            pos += 2;
            if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
            if (m == 0xD9) break;
            if (pos + 2 > len) break;
            const size_t seglen = ((size_t)data[pos] << 8) | data[pos + 1];
            if (seglen < 2 || pos + seglen > len) return fail(ICL_ERR_IO, "The image file might be corrupt or unreadable");
            const uint8_t *s = data + pos + 2, *next = data + pos + seglen;
            const size_t sl = seglen - 2;
            int rc = ICL_OK;
            switch (m) {
            case 0xDB: rc = dqt(s, sl); break;
            case 0xC4: rc = dht(s, sl); break;
            case 0xC0: case 0xC1: case 0xC2: rc = sof(m, s, sl); break;
            case 0xDD: dri(s, sl); break;
            case 0xE1: app1(s, sl); break;
            case 0xEE: app14(s, sl); break;
            case 0xDA: rc = sos(s, sl, next); break;
            default:
                if (m >= 0xC3 && m <= 0xCF && m != 0xC8 && m != 0xCC)
                    rc = fail(ICL_ERR_UNSUPPORTED, "Lossless / hierarchical / arithmetic-coded JPEG is not decoded by this build");
            }
            if (rc) return rc;
            pos = (size_t)(next - data);
        }
        if (!have_sof || nscans == 0) return fail(ICL_ERR_IO, "The image file might be corrupt or unreadable");
        for (int c = 0; c < ncomp; ++c) {
            if (J.comp[c].tq > 3 || !qt_ok[J.comp[c].tq]) return fail(ICL_ERR_IO, "Missing table");
            memcpy(J.qt[c], qt[J.comp[c].tq], sizeof J.qt[c]); // the table as it stands after the last scan (what dequantisation uses)
        }
        J.ncomp = ncomp;
        J.is_rgb = ncomp == 3 && ((adobe && adobe_transform == 0) || (!adobe && J.comp[0].id == 'R' && J.comp[1].id == 'G' && J.comp[2].id == 'B'));
        return ICL_OK;
    }
};

} // namespace

static int jpeg_stage_a_impl(icl_ctx *ctx, const uint8_t *data, size_t len, const char *path, icl_jpeg_coefs &J, icl_jpeg_a0 *a0, int sub_bits)
{
    return stage_a{ctx, path, data, len, J, a0, sub_bits}.run();
}

// Stage B: dequantise + inverse DCT (once, after the last scan), chroma upsampling, colour conversion.
static int jpeg_stage_b_impl(const icl_jpeg_coefs &J, std::vector<uint8_t> &rgb)
{
    const int W = J.W, H = J.H, ncomp = J.ncomp;
    std::vector<uint8_t> plane[3]; // wblocks*8 x hblocks*8 per component
    for (int c = 0; c < ncomp; ++c) {
        const icl_jpeg_component &k = J.comp[c];
        const size_t stride = (size_t)k.wblocks * 8;
        plane[c].assign(stride * k.hblocks * 8, 0);
        int coef[64];
        for (int by = 0; by < k.hblocks; ++by)
            for (int bx = 0; bx < k.wblocks; ++bx) {
                const int16_t *cf = k.coefs.data() + ((size_t)by * k.wblocks + bx) * 64;
                for (int i = 0; i < 64; ++i) coef[i] = cf[i] * J.qt[c][i];
                idct_islow(coef, plane[c].data() + (size_t)by * 8 * stride + (size_t)bx * 8, (int)stride);
            }
    }
    const icl_jpeg_component *comp = J.comp;
    rgb.assign((size_t)W * H * 3, 0);
    if (ncomp == 1) {
        const size_t stride = (size_t)comp[0].wblocks * 8;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const uint8_t g = plane[0][y * stride + x];
                uint8_t *o = &rgb[((size_t)y * W + x) * 3];
                o[0] = o[1] = o[2] = g;
            }
        return ICL_OK;
    }
    // chroma upsampling (jdsample.c rules of ingest_pixels.h, one output row at a time) and colour conversion (jdcolor.c), or
    // pass-through for Adobe transform 0
    const int hs = comp[0].h, vs = comp[0].v, dw = comp[1].dw, dh = comp[1].dh;
    const size_t ystride = (size_t)comp[0].wblocks * 8, cstride = (size_t)comp[1].wblocks * 8;
    std::vector<uint8_t> up[2] = {std::vector<uint8_t>((size_t)W + 1), std::vector<uint8_t>((size_t)W + 1)}; // 2 * dw <= W + 1
    std::vector<int> cs((size_t)dw);
    for (int y = 0; y < H; ++y) {
        for (int c = 0; c < 2; ++c) {
            const uint8_t *pl = plane[c + 1].data();
            uint8_t *o = up[c].data();
            if (hs == 1 && vs == 1) {
                memcpy(o, pl + (size_t)y * cstride, (size_t)W);
            } else if (hs == 2 && vs == 1) {
                const uint8_t *p = pl + (size_t)y * cstride;
                auto col = [&](int k) { return (int)p[k]; };
                for (int i = 0; i < dw; ++i) {
                    o[2 * i] = (uint8_t)icl_fancy_h2<1>(col, dw, 2 * i);
                    o[2 * i + 1] = (uint8_t)icl_fancy_h2<1>(col, dw, 2 * i + 1);
                }
            } else if (hs != 2) { // 1x2, 4x1, 1x4: no horizontal filter, the per-sample rule as the GPU applies it
                for (int x = 0; x < W; ++x) o[x] = (uint8_t)icl_fancy_upsample(pl, (int64_t)cstride, dw, dh, hs, vs, x, y);
            } else {
                int r0, r1;
                icl_fancy_rows(y, dh, r0, r1);
                const uint8_t *p0 = pl + (size_t)r0 * cstride, *p1 = pl + (size_t)r1 * cstride;
                for (int i = 0; i < dw; ++i) cs[(size_t)i] = icl_fancy_colsum(p0[i], p1[i]);
                auto col = [&](int k) { return cs[(size_t)k]; };
                for (int i = 0; i < dw; ++i) {
                    o[2 * i] = (uint8_t)icl_fancy_h2<2>(col, dw, 2 * i);
                    o[2 * i + 1] = (uint8_t)icl_fancy_h2<2>(col, dw, 2 * i + 1);
                }
            }
        }
        const uint8_t *Yr = plane[0].data() + (size_t)y * ystride;
        uint8_t *o = &rgb[(size_t)y * W * 3];
        for (int x = 0; x < W; ++x, o += 3) {
            const int Y = Yr[x], cb = up[0][(size_t)x], cr = up[1][(size_t)x];
            if (J.is_rgb) {
                o[0] = (uint8_t)Y; o[1] = (uint8_t)cb; o[2] = (uint8_t)cr;
            } else {
                int R, G, B;
                icl_ycc_to_rgb(Y, cb, cr, R, G, B);
                o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
            }
        }
    }
    return ICL_OK;
}
