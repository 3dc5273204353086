// png_inflate.h -- the arithmetic of the GPU PNG route (png_gpu.hip), shared with its host rehearsal (png_decode.hip,
// icl_png_raw_file_host): DEFLATE (RFC 1951) with the legality rules of the host decoder's inflate_exact, Adler-32 by position-weighted
// chunks, the five scanline filters (PNG 9.2) one pixel at a time, the palette-index check, and the sample-to-RGB rule of
// cv::imread(IMREAD_COLOR).  Everything is __host__ __device__, integer only, and uses no HIP type: the kernels and the host loop run
// the same functions over the same schedule, so what the host loop shows (tests/test_png_gpu_schedule_cpu.py, and the sanitised
// stand-alone program) is what the kernels do.
//
// The inflate schedule.  One wave of ICL_PNG_LANES lanes per image and icl_png_lds in LDS: the 32 KiB window as a ring, a 2 KiB window
// onto the input, the primary lookup tables (10 bits literal / length, 8 bits distance) with the canonical count / symbol arrays behind
// them for longer codes, and the decoder's state.  Each round lane 0 decodes (icl_png_decode_step) until something needs the wave: a
// match, a piece of a stored block, new tables, more input, a flush -- one record -- and the wave executes it.  Literals go straight
// into the ring.  A match is read completely (src = at - d + (i mod d) for d < len) into a staging row before it is written, so no
// lane reads a byte another lane has just replaced, whatever the ring's wrap does.  Whenever 4 KiB are pending, the ring is flushed
// to the image's scratch in 16-byte pieces; matches never read global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#define ICL_PNG_HD __host__ __device__ inline

constexpr int ICL_PNG_LANES = 64;
constexpr int ICL_PNG_RING = 32768;       // the DEFLATE window
constexpr int ICL_PNG_INWIN = 2048;       // input bytes held in LDS: [in_hi - 2048, in_hi)
constexpr int ICL_PNG_INPIECE = 1024;     // ... loaded 16 bytes per lane at a time
constexpr int ICL_PNG_FLUSH = 4096;       // pending output at which the ring is flushed
constexpr int ICL_PNG_STORED_PIECE = 4096; // bytes of a stored block per record
constexpr int ICL_PNG_LIT_BITS = 10, ICL_PNG_DIST_BITS = 8;
constexpr int ICL_PNG_HDR_NEED = 768;     // input bytes a block header may use (dynamic: 14 + 19 x 3 + 316 x 14 bits < 600 bytes)
constexpr uint32_t ICL_ADLER_MOD = 65521u;
constexpr int ICL_ADLER_CHUNK = 2048;     // (<= 5552: a chunk's sums cannot overflow 32 bits before their modulo)

// What the host places in front of a PNG's zlib stream in the slab's payload (a multiple of 16 bytes; the stream follows, whole:
// the two header bytes, the DEFLATE blocks, the Adler-32 trailer).
struct icl_png_desc {
    int32_t w, h, depth, ctype;
    int32_t rowb, bpp; // bytes of a scanline without its filter byte; filter distance
    int32_t npal, zbytes;
    int64_t want; // h * (1 + rowb)
    uint32_t adler, pad_;
    uint8_t pal[768];
};
static_assert(sizeof(icl_png_desc) % 16 == 0, "the stream behind the descriptor starts on a 16-byte boundary");

struct alignas(16) icl_png_v16 {
    uint32_t x[4];
};

enum { ICL_PNG_REC_NONE = 0, ICL_PNG_REC_MATCH, ICL_PNG_REC_STORED, ICL_PNG_REC_TABLES, ICL_PNG_REC_INPUT, ICL_PNG_REC_DONE, ICL_PNG_REC_FAIL };
enum { ICL_PNG_PH_HDR = 0, ICL_PNG_PH_CODES, ICL_PNG_PH_STORED, ICL_PNG_PH_DONE };
// coverage counters (icl_png_raw_file_host's info[5..11])
enum { ICL_PNG_COV_STORED = 0, ICL_PNG_COV_FIXED, ICL_PNG_COV_DYNAMIC, ICL_PNG_COV_MAXLEN, ICL_PNG_COV_MAXDIST, ICL_PNG_COV_OVERLAP, ICL_PNG_COV_WRAPS, ICL_PNG_NCOV };

struct alignas(16) icl_png_lds {
    uint32_t ring[ICL_PNG_RING / 4];
    uint32_t inwin[ICL_PNG_INWIN / 4];
    uint16_t lit_tab[1 << ICL_PNG_LIT_BITS], dist_tab[1 << ICL_PNG_DIST_BITS]; // symbol | code length << 9; 0: longer than the index
    uint16_t lcount[16], lsym[288], dcount[16], dsym[32];                        // canonical codes: codes per length, symbols by (length, value)
    uint16_t ccount[16], csym[19], offs[16];                                     // the code-length code; huff_build's running offsets
    uint8_t lens[320], cl[19], stage[264];
    // the decoder's state: lane 0 writes it, the wave reads it behind a barrier
    uint64_t acc;
    int32_t nbits;
    int32_t phase, last, stored_left, failed, ok;
    int32_t rec, rec_len, rec_dist;
    int64_t rec_at, rec_src;
    int64_t pos, in_hi, end, zbytes; // next stream byte to enter acc; bytes loaded so far; first byte of the trailer; stream bytes
    int64_t out, flushed, want;
    int32_t cov[ICL_PNG_NCOV];
};

inline constexpr uint16_t icl_png_lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
inline constexpr uint8_t icl_png_lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
inline constexpr uint16_t icl_png_dbase[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                               193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
inline constexpr uint8_t icl_png_dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
inline constexpr uint8_t icl_png_clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

ICL_PNG_HD uint8_t *icl_png_ringb(icl_png_lds &L) { return (uint8_t *)L.ring; }

// ---- bit input (lane 0): LSB first; bytes at or behind `end` read as zero, and a symbol that used one of them is an overrun.  The
// reader's state lives in registers while lane 0 decodes (icl_png_bits) and in icl_png_lds between its steps. ----
struct icl_png_bits {
    uint64_t acc;
    int32_t nbits;
    int64_t pos;
};
ICL_PNG_HD uint32_t icl_png_in_byte(const icl_png_lds &L, int64_t p)
{
    if (p < 0 || p >= L.end || p >= L.in_hi || p < L.in_hi - ICL_PNG_INWIN) return 0;
    return ((const uint8_t *)L.inwin)[p & (ICL_PNG_INWIN - 1)];
}
ICL_PNG_HD void icl_png_refill(const icl_png_lds &L, icl_png_bits &B)
{
    while (B.nbits <= 56) {
        B.acc |= (uint64_t)icl_png_in_byte(L, B.pos) << B.nbits;
        ++B.pos;
        B.nbits += 8;
    }
}
ICL_PNG_HD uint32_t icl_png_take(icl_png_bits &B, int k) // k <= 16 <= nbits
{
    const uint32_t v = (uint32_t)B.acc & ((1u << k) - 1u);
    B.acc >>= k;
    B.nbits -= k;
    return v;
}
ICL_PNG_HD bool icl_png_overrun(const icl_png_lds &L, const icl_png_bits &B) { return B.pos * 8 - B.nbits > L.end * 8; }

// ---- canonical Huffman codes, as the host decoder builds and walks them ----
// returns 0: complete code, > 0: incomplete, < 0: over-subscribed
ICL_PNG_HD int icl_png_huff_build(uint16_t *count, uint16_t *symbol, uint16_t *offs, const uint8_t *len, int n)
{
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[len[s] & 15];
    if (count[0] == n) return 0; // no codes at all: complete by convention, decoding any symbol fails
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= count[l];
        if (left < 0) return left;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int s = 0; s < n; ++s)
        if (len[s] & 15) symbol[offs[len[s] & 15]++] = (uint16_t)s;
    return left;
}
// the walk over the low `maxl` bits of `bits` (first bit of the code lowest); returns the symbol and its length, or -1
ICL_PNG_HD int icl_png_huff_walk(uint32_t bits, int maxl, const uint16_t *count, const uint16_t *symbol, int nsym, int &len)
{
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= maxl; ++l) {
        code |= (int)((bits >> (l - 1)) & 1u);
        const int cnt = count[l];
        if (code - cnt < first) {
            const int at = index + (code - first);
            len = l;
            return at >= 0 && at < nsym ? symbol[at] : -1;
        }
        index += cnt;
        first += cnt;
        first <<= 1;
        code <<= 1;
    }
    len = maxl;
    return -1;
}
// one entry of a primary table: index i is the next `bits` bits of the stream
ICL_PNG_HD uint16_t icl_png_table_entry(uint32_t i, int bits, const uint16_t *count, const uint16_t *symbol, int nsym)
{
    int len = 0;
    const int s = icl_png_huff_walk(i, bits, count, symbol, nsym, len);
    return s < 0 ? (uint16_t)0 : (uint16_t)(s | (len << 9));
}
// REC_TABLES, all lanes: the primary tables from the canonical arrays lane 0 has built
ICL_PNG_HD void icl_png_fill_tables(icl_png_lds &L, int lane)
{
    for (int i = lane; i < (1 << ICL_PNG_LIT_BITS); i += ICL_PNG_LANES) L.lit_tab[i] = icl_png_table_entry((uint32_t)i, ICL_PNG_LIT_BITS, L.lcount, L.lsym, 288);
    for (int i = lane; i < (1 << ICL_PNG_DIST_BITS); i += ICL_PNG_LANES) L.dist_tab[i] = icl_png_table_entry((uint32_t)i, ICL_PNG_DIST_BITS, L.dcount, L.dsym, 32);
}
// one symbol from acc (at least 15 bits there): the primary table, or the canonical walk for a longer code
ICL_PNG_HD int icl_png_symbol(icl_png_lds &L, icl_png_bits &B, const uint16_t *tab, int tbits, const uint16_t *count, const uint16_t *symbol, int nsym)
{
    const uint32_t e = tab[(uint32_t)B.acc & ((1u << tbits) - 1u)];
    int len = (int)(e >> 9), s = (int)(e & 511u);
    if (len == 0) s = icl_png_huff_walk((uint32_t)B.acc & 0x7fffu, 15, count, symbol, nsym, len);
    icl_png_take(B, len);
    if (s >= 0 && len > L.cov[ICL_PNG_COV_MAXLEN]) L.cov[ICL_PNG_COV_MAXLEN] = len;
    return s;
}

ICL_PNG_HD void icl_png_state_init(icl_png_lds &L, int64_t zbytes, int64_t want)
{
    L.acc = 0;
    L.nbits = 0;
    L.phase = ICL_PNG_PH_HDR;
    L.last = 0;
    L.stored_left = 0;
    L.failed = 0;
    L.ok = 0;
    L.rec = ICL_PNG_REC_NONE;
    L.rec_len = L.rec_dist = 0;
    L.rec_at = L.rec_src = 0;
    L.pos = 2; // behind the zlib header
    L.in_hi = 0;
    L.zbytes = zbytes;
    L.end = zbytes - 4;
    L.out = L.flushed = 0;
    L.want = want;
    for (int i = 0; i < ICL_PNG_NCOV; ++i) L.cov[i] = 0;
}

// the header of a dynamic block (RFC 1951 3.2.7) into lens / the canonical arrays; false: illegal
ICL_PNG_HD bool icl_png_dynamic_header(icl_png_lds &L, icl_png_bits &B)
{
    icl_png_refill(L, B);
    const int nlen = (int)icl_png_take(B, 5) + 257, ndist = (int)icl_png_take(B, 5) + 1, ncode = (int)icl_png_take(B, 4) + 4;
    if (icl_png_overrun(L, B) || nlen > 286 || ndist > 30) return false;
    for (int i = 0; i < 19; ++i) L.cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        icl_png_refill(L, B);
        L.cl[icl_png_clorder[i]] = (uint8_t)icl_png_take(B, 3);
    }
    if (icl_png_overrun(L, B)) return false;
    if (icl_png_huff_build(L.ccount, L.csym, L.offs, L.cl, 19) != 0) return false; // the code-length code must be complete
    int idx = 0;
    while (idx < nlen + ndist) {
        icl_png_refill(L, B);
        int len = 0;
        const int sym = icl_png_huff_walk((uint32_t)B.acc & 0x7fffu, 15, L.ccount, L.csym, 19, len);
        icl_png_take(B, len);
        if (sym < 0 || icl_png_overrun(L, B)) return false;
        if (sym < 16) {
            L.lens[idx++] = (uint8_t)sym;
        } else {
            int rep, val = 0;
            if (sym == 16) {
                if (idx == 0) return false;
                val = L.lens[idx - 1];
                rep = 3 + (int)icl_png_take(B, 2);
            } else if (sym == 17) {
                rep = 3 + (int)icl_png_take(B, 3);
            } else {
                rep = 11 + (int)icl_png_take(B, 7);
            }
            if (icl_png_overrun(L, B) || idx + rep > nlen + ndist) return false;
            while (rep--) L.lens[idx++] = (uint8_t)val;
        }
    }
    if (L.lens[256] == 0) return false; // no end-of-block code
    // over-subscribed codes are errors; an incomplete code is only legal as ONE code of length 1
    const int el = icl_png_huff_build(L.lcount, L.lsym, L.offs, L.lens, nlen);
    if (el < 0 || (el > 0 && !(L.lcount[1] == 1 && nlen - L.lcount[0] == 1))) return false;
    const int ed = icl_png_huff_build(L.dcount, L.dsym, L.offs, L.lens + nlen, ndist);
    if (ed < 0 || (ed > 0 && !(L.dcount[1] == 1 && ndist - L.dcount[0] == 1))) return false;
    return true;
}

// Lane 0: decode until the wave is needed; the record is in L.rec*.  Every call consumes input, produces output, asks for input that
// exists, or fails (REC_NONE: output is pending a flush, or a run of empty blocks went by) -- so the caller's loop is bounded by the
// stream's bits plus `want`.
#define ICL_PNG_BAD                  \
    do {                             \
        L.failed = 1;                \
        L.rec = ICL_PNG_REC_FAIL;    \
        return;                      \
    } while (0)
ICL_PNG_HD void icl_png_decode_regs(icl_png_lds &L, icl_png_bits &B, int64_t &out)
{
    L.rec = ICL_PNG_REC_NONE;
    if (L.failed) {
        L.rec = ICL_PNG_REC_FAIL;
        return;
    }
    uint8_t *ring = icl_png_ringb(L);
    for (int guard = 0; guard < 2 * ICL_PNG_FLUSH; ++guard) {
        if (L.phase == ICL_PNG_PH_DONE) {
            L.ok = out == L.want ? 1 : 0;
            L.rec = ICL_PNG_REC_DONE;
            return;
        }
        if (out - L.flushed >= ICL_PNG_FLUSH) return; // (REC_NONE: the caller flushes)
        if (L.in_hi < L.zbytes && L.in_hi - B.pos < (L.phase == ICL_PNG_PH_HDR ? ICL_PNG_HDR_NEED : 16)) {
            const int64_t skip = B.pos & ~(int64_t)(ICL_PNG_INPIECE - 1); // behind a stored block the window moves up to the reader
            if (L.in_hi < skip) L.in_hi = skip;
            L.rec = ICL_PNG_REC_INPUT;
            return;
        }
        if (L.phase == ICL_PNG_PH_STORED) {
            const int n = L.stored_left < ICL_PNG_STORED_PIECE ? L.stored_left : ICL_PNG_STORED_PIECE;
            L.rec = ICL_PNG_REC_STORED;
            L.rec_len = n;
            L.rec_src = B.pos;
            L.rec_at = out;
            B.pos += n;
            out += n;
            L.stored_left -= n;
            if (L.stored_left == 0) L.phase = L.last ? ICL_PNG_PH_DONE : ICL_PNG_PH_HDR;
            return;
        }
        icl_png_refill(L, B);
        if (L.phase == ICL_PNG_PH_HDR) {
            L.last = (int)icl_png_take(B, 1);
            const int type = (int)icl_png_take(B, 2);
            if (icl_png_overrun(L, B)) ICL_PNG_BAD;
            if (type == 0) {
                ++L.cov[ICL_PNG_COV_STORED];
                B.pos -= B.nbits / 8; // to the next byte boundary: the whole bytes still in acc go back
                B.acc = 0;
                B.nbits = 0;
                if (L.end - B.pos < 4) ICL_PNG_BAD;
                const uint32_t len = icl_png_in_byte(L, B.pos) | (icl_png_in_byte(L, B.pos + 1) << 8);
                const uint32_t nlen = icl_png_in_byte(L, B.pos + 2) | (icl_png_in_byte(L, B.pos + 3) << 8);
                B.pos += 4;
                if ((len ^ 0xffffu) != nlen || L.end - B.pos < (int64_t)len || out + (int64_t)len > L.want) ICL_PNG_BAD;
                L.stored_left = (int)len;
                L.phase = len ? ICL_PNG_PH_STORED : (L.last ? ICL_PNG_PH_DONE : ICL_PNG_PH_HDR);
                continue;
            }
            if (type == 1) { // fixed codes (3.2.6)
                ++L.cov[ICL_PNG_COV_FIXED];
                int s = 0;
                for (; s < 144; ++s) L.lens[s] = 8;
                for (; s < 256; ++s) L.lens[s] = 9;
                for (; s < 280; ++s) L.lens[s] = 7;
                for (; s < 288; ++s) L.lens[s] = 8;
                icl_png_huff_build(L.lcount, L.lsym, L.offs, L.lens, 288);
                for (s = 0; s < 30; ++s) L.lens[s] = 5;
                icl_png_huff_build(L.dcount, L.dsym, L.offs, L.lens, 30);
            } else if (type == 2) {
                ++L.cov[ICL_PNG_COV_DYNAMIC];
                if (!icl_png_dynamic_header(L, B)) ICL_PNG_BAD;
            } else {
                ICL_PNG_BAD;
            }
            L.phase = ICL_PNG_PH_CODES;
            L.rec = ICL_PNG_REC_TABLES;
            return;
        }
        // ICL_PNG_PH_CODES: one symbol (at most 15 + 5 + 15 + 13 of the >= 57 bits in acc)
        int sym = icl_png_symbol(L, B, L.lit_tab, ICL_PNG_LIT_BITS, L.lcount, L.lsym, 288);
        if (sym < 0 || icl_png_overrun(L, B)) ICL_PNG_BAD;
        if (sym < 256) {
            if (out >= L.want) ICL_PNG_BAD;
            ring[out & (ICL_PNG_RING - 1)] = (uint8_t)sym;
            ++out;
        } else if (sym == 256) {
            L.phase = L.last ? ICL_PNG_PH_DONE : ICL_PNG_PH_HDR;
        } else {
            sym -= 257;
            if (sym >= 29) ICL_PNG_BAD;
            const int len = icl_png_lbase[sym] + (int)icl_png_take(B, icl_png_lext[sym]);
            const int ds = icl_png_symbol(L, B, L.dist_tab, ICL_PNG_DIST_BITS, L.dcount, L.dsym, 32);
            if (ds < 0 || ds >= 30) ICL_PNG_BAD;
            const int d = icl_png_dbase[ds] + (int)icl_png_take(B, icl_png_dext[ds]);
            if (icl_png_overrun(L, B) || (int64_t)d > out || out + len > L.want) ICL_PNG_BAD;
            if (d > L.cov[ICL_PNG_COV_MAXDIST]) L.cov[ICL_PNG_COV_MAXDIST] = d;
            if (d < len) ++L.cov[ICL_PNG_COV_OVERLAP];
            if ((out & (ICL_PNG_RING - 1)) + len > ICL_PNG_RING) ++L.cov[ICL_PNG_COV_WRAPS];
            L.rec = ICL_PNG_REC_MATCH;
            L.rec_len = len;
            L.rec_dist = d;
            L.rec_at = out;
            out += len;
            return;
        }
        continue;
    }
}

#undef ICL_PNG_BAD
ICL_PNG_HD void icl_png_decode_step(icl_png_lds &L)
{
    icl_png_bits B = {L.acc, L.nbits, L.pos};
    int64_t out = L.out;
    icl_png_decode_regs(L, B, out);
    L.acc = B.acc;
    L.nbits = B.nbits;
    L.pos = B.pos;
    L.out = out;
}

// ---- what the wave does with a record ----
// REC_INPUT, all lanes: the next 1 KiB of the stream into the window.  z is 16-byte aligned; bytes behind zbytes load as zero.
ICL_PNG_HD void icl_png_fill_input(icl_png_lds &L, const uint8_t *z, int lane)
{
    const int64_t o = L.in_hi + (int64_t)lane * 16;
    icl_png_v16 v = {{0, 0, 0, 0}};
    if (o + 16 <= L.zbytes) {
        v = *(const icl_png_v16 *)(z + o);
    } else {
        for (int k = 0; k < 16; ++k)
            if (o + k < L.zbytes) v.x[k >> 2] |= (uint32_t)z[o + k] << (8 * (k & 3));
    }
    uint32_t *w = L.inwin + ((o & (ICL_PNG_INWIN - 1)) >> 2);
    w[0] = v.x[0];
    w[1] = v.x[1];
    w[2] = v.x[2];
    w[3] = v.x[3];
}
// REC_MATCH, all lanes, two steps with a barrier between: the whole source into the staging row, then the staging row into the ring
ICL_PNG_HD void icl_png_match_read(icl_png_lds &L, int lane)
{
    const uint8_t *ring = icl_png_ringb(L);
    const int len = L.rec_len, d = L.rec_dist;
    const int64_t from = L.rec_at - d;
    for (int i = lane; i < len; i += ICL_PNG_LANES) L.stage[i] = ring[(from + (d < len ? i % d : i)) & (ICL_PNG_RING - 1)];
}
ICL_PNG_HD void icl_png_match_write(icl_png_lds &L, int lane)
{
    uint8_t *ring = icl_png_ringb(L);
    for (int i = lane; i < L.rec_len; i += ICL_PNG_LANES) ring[(L.rec_at + i) & (ICL_PNG_RING - 1)] = L.stage[i];
}
// REC_STORED, all lanes: a piece of a stored block from the stream (lane 0 has checked it lies in front of the trailer) into the ring
ICL_PNG_HD void icl_png_stored_copy(icl_png_lds &L, const uint8_t *z, int lane)
{
    uint8_t *ring = icl_png_ringb(L);
    for (int i = lane; i < L.rec_len; i += ICL_PNG_LANES) {
        const int64_t s = L.rec_src + i;
        ring[(L.rec_at + i) & (ICL_PNG_RING - 1)] = s >= 0 && s < L.end ? z[s] : (uint8_t)0;
    }
}
// all lanes: ring bytes [L.flushed, hi) to dst (16-byte aligned; L.flushed is a multiple of 16; hi <= want = dst's extent)
ICL_PNG_HD void icl_png_flush(icl_png_lds &L, uint8_t *dst, int64_t hi, int lane)
{
    const int64_t lo = L.flushed, whole = lo + ((hi - lo) & ~(int64_t)15);
    for (int64_t p = lo + (int64_t)lane * 16; p < whole; p += ICL_PNG_LANES * 16) {
        const uint32_t *r = L.ring + ((p & (ICL_PNG_RING - 1)) >> 2);
        icl_png_v16 v;
        v.x[0] = r[0];
        v.x[1] = r[1];
        v.x[2] = r[2];
        v.x[3] = r[3];
        *(icl_png_v16 *)(dst + p) = v;
    }
    const uint8_t *ring = icl_png_ringb(L);
    for (int64_t p = whole + lane; p < hi; p += ICL_PNG_LANES) dst[p] = ring[p & (ICL_PNG_RING - 1)];
}

// The schedule: the kernel calls it with its own lane (lane0 = threadIdx.x, lane1 = lane0 + 1) and __syncthreads as `sync`; the host
// rehearsal with lanes 0 .. 64 and a no-op.  z: the zlib stream (16-byte aligned, zbytes >= 6); dst: `want` bytes, 16-byte aligned.
// Afterwards L.ok says whether the final block ended with exactly `want` bytes written from a legal stream.
template <class Sync> ICL_PNG_HD void icl_png_inflate_run(icl_png_lds &L, const uint8_t *z, int64_t zbytes, uint8_t *dst, int64_t want, int lane0, int lane1, Sync sync)
{
    if (lane0 == 0) icl_png_state_init(L, zbytes, want);
    sync();
    const int64_t rounds = 4 * (zbytes * 8 + want) + 64;
    for (int64_t it = 0; it < rounds; ++it) {
        if (lane0 == 0) icl_png_decode_step(L);
        sync();
        const int rec = L.rec;
        if (rec == ICL_PNG_REC_FAIL) break;
        if (rec == ICL_PNG_REC_INPUT) {
            for (int lane = lane0; lane < lane1; ++lane) icl_png_fill_input(L, z, lane);
            sync();
            if (lane0 == 0) L.in_hi += ICL_PNG_INPIECE;
            sync();
            continue;
        }
        if (rec == ICL_PNG_REC_TABLES) {
            for (int lane = lane0; lane < lane1; ++lane) icl_png_fill_tables(L, lane);
        } else if (rec == ICL_PNG_REC_MATCH) {
            for (int lane = lane0; lane < lane1; ++lane) icl_png_match_read(L, lane);
            sync();
            for (int lane = lane0; lane < lane1; ++lane) icl_png_match_write(L, lane);
        } else if (rec == ICL_PNG_REC_STORED) {
            for (int lane = lane0; lane < lane1; ++lane) icl_png_stored_copy(L, z, lane);
        }
        sync();
        const bool done = rec == ICL_PNG_REC_DONE;
        if (done || L.out - L.flushed >= ICL_PNG_FLUSH) {
            const int64_t hi = done ? L.out : (L.out & ~(int64_t)15);
            for (int lane = lane0; lane < lane1; ++lane) icl_png_flush(L, dst, hi, lane);
            sync();
            if (lane0 == 0) L.flushed = hi;
            sync();
        }
        if (done) break;
    }
}

// ---- Adler-32 (RFC 1950) by chunks: a = 1 + sum p[i], b = n + sum (n - i) p[i], so a chunk [s, s + m) of an n-byte buffer adds
// (sum p, sum (m - j) p[s + j] + (n - s - m) * sum p) whatever the other chunks hold ----
ICL_PNG_HD void icl_adler_chunk(const uint8_t *p, int m /* <= ICL_ADLER_CHUNK */, int64_t after /* n - s - m */, uint32_t &sa, uint32_t &sb)
{
    uint32_t a = 0, b = 0;
    for (int j = 0; j < m; ++j) {
        a += p[j];
        b += (uint32_t)(m - j) * p[j];
    }
    a %= ICL_ADLER_MOD;
    sa = (sa + a) % ICL_ADLER_MOD;
    sb = (uint32_t)((sb + (uint64_t)(after % ICL_ADLER_MOD) * a + b) % ICL_ADLER_MOD);
}
ICL_PNG_HD uint32_t icl_adler_finish(uint32_t sa, uint32_t sb, int64_t n)
{
    const uint32_t a = (1u + sa % ICL_ADLER_MOD) % ICL_ADLER_MOD, b = (uint32_t)((n % ICL_ADLER_MOD + sb % ICL_ADLER_MOD) % ICL_ADLER_MOD);
    return (b << 16) | a;
}

// ---- scanline filters (PNG 9.2), one pixel of up to 8 bytes packed into a uint64 (byte k in bits 8k..8k+7): x the filtered bytes,
// a the pixel to the left, b the one above, c above-left (zero outside the image) ----
ICL_PNG_HD uint64_t icl_png_unfilter_px(int ft, int bpp, uint64_t x, uint64_t a, uint64_t b, uint64_t c)
{
    uint64_t o = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (k < bpp) {
            const int xv = (int)((x >> (8 * k)) & 255u), av = (int)((a >> (8 * k)) & 255u), bv = (int)((b >> (8 * k)) & 255u), cv = (int)((c >> (8 * k)) & 255u);
            int pr = 0;
            if (ft == 1) pr = av;
            else if (ft == 2) pr = bv;
            else if (ft == 3) pr = (av + bv) >> 1;
            else if (ft == 4) {
                const int p = av + bv - cv, pa = p > av ? p - av : av - p, pb = p > bv ? p - bv : bv - p, pc = p > cv ? p - cv : cv - p;
                pr = (pa <= pb && pa <= pc) ? av : (pb <= pc ? bv : cv);
            }
            o |= (uint64_t)((xv + pr) & 255) << (8 * k);
        }
    }
    return o;
}
ICL_PNG_HD uint64_t icl_png_load_px(const uint8_t *p, int bpp)
{
    uint64_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < bpp) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
ICL_PNG_HD void icl_png_store_px(uint8_t *p, int bpp, uint64_t v)
{
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < bpp) p[k] = (uint8_t)(v >> (8 * k));
}
// colour type 3: does byte `bi` of an unfiltered row hold an index >= npal at a pixel of the image (x < w)?
ICL_PNG_HD bool icl_png_pal_bad(uint32_t v, int64_t bi, int w, int depth, int npal)
{
    if (depth == 8) return (int)v >= npal;
    const int per = 8 / depth;
    bool bad = false;
    for (int s = 0; s < per; ++s) {
        const int64_t x = bi * per + s;
        const int idx = (int)((v >> (8 - depth * (s + 1))) & ((1u << depth) - 1u));
        if (x < w && idx >= npal) bad = true;
    }
    return bad;
}

// ---- a sample to RGB as cv::imread(IMREAD_COLOR) delivers it: alpha dropped, 16-bit samples cut to the high byte, grey 1 / 2 / 4 bits
// scaled by 255 / (2^depth - 1), palette looked up.  cur: the unfiltered scanline behind its filter byte; pal: 256 x 3 bytes. ----
ICL_PNG_HD void icl_png_sample_rgb(const uint8_t *cur, int64_t x, int ctype, int depth, const uint8_t *pal, int &R, int &G, int &B)
{
    const int step = depth == 16 ? 2 : 1;
    if (ctype == 2 || ctype == 6) {
        const uint8_t *sp = cur + x * (ctype == 2 ? 3 : 4) * step;
        R = sp[0];
        G = sp[step];
        B = sp[2 * step];
    } else if (ctype == 4 || (ctype == 0 && depth >= 8)) {
        R = G = B = cur[x * (ctype == 4 ? 2 : 1) * step];
    } else { // packed samples: grey 1 / 2 / 4 bits or palette indices 1 / 2 / 4 / 8 bits
        uint32_t v;
        if (depth == 8) v = cur[x];
        else {
            const int64_t bit = x * depth;
            v = ((uint32_t)cur[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);
        }
        if (ctype == 3) {
            R = pal[v * 3];
            G = pal[v * 3 + 1];
            B = pal[v * 3 + 2];
        } else {
            R = G = B = (int)(v * (255u / ((1u << depth) - 1u)));
        }
    }
}
