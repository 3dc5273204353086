// jpeg_entropy.h -- the entropy decoder of a baseline JPEG scan cut into subsequences, shared by the GPU kernels
// (jpeg_huff_gpu.hip) and a plain host loop (jpeg_decode.hip: the rehearsal without a GPU, and the sanitizer target).
//
// A restart interval (or the whole scan) of the UNSTUFFED bit stream is cut into subsequences of sub_bits bits.  One thread decodes
// one subsequence from an entry state (bit position in the interval, block index within the MCU, zig-zag index) to an exit state and
// counts the blocks it completes (the self-synchronising scheme of Weissenberger & Schmidt).  Threads start from a guess and
// take over their predecessor's exit state for some rounds; afterwards an image is ACCEPTED only if the chain is consistent
// (entry[0] is the known start, entry[i + 1] == exit[i], exit[i] computed from entry[i]) and the stream is clean.  By induction
// over i an accepted chain is the sequential decode, whatever the guesses were; everything else is redone by host stage A.
// Integer arithmetic only, no allocation: everything here is __host__ __device__.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "ingest_pixels.h"

constexpr int ICL_JE_SUB_BITS = 1024; // subsequence size of the pipeline (a multiple of 32; DESIGN.md 4 "Entropy decoding on the GPU")
constexpr int ICL_JE_WG = 256;        // subsequences (threads) per workgroup
// Synchronisation launches (rounds that cross workgroups are separate launches).  After launch l the first l workgroups of an interval
// are right by construction; the others are right once their guessed chain has met the true one, which needs the preceding workgroup's
// last exit state to be right after launch 1 (its 256 subsequences are 32 KiB of stream; code words, zig-zag index and -- through the
// components' different tables -- the block-within-MCU index meet within a few subsequences) and launch 2 to carry it over.  The third
// launch is margin: it tolerates one workgroup whose last thread had not met the true chain.  Files whose components all use the same
// tables can never meet in the block-within-MCU index; for them that index is not part of the state at all (icl_je_scan::uniform).
constexpr int ICL_JE_LAUNCHES = 3;
constexpr int ICL_JE_ROUNDS = ICL_JE_WG - 1; // rounds inside a workgroup (it stops earlier once no entry state changes)

enum { ICL_JE_ERR = 1, ICL_JE_SHORT = 2 }; // flags of a decoded subsequence: invalid data / the next symbol does not fit in the interval

// huff_table of jpeg_decode.hip in POD form: the 9-bit lookahead plus mincode / maxcode / valptr
struct icl_je_table {
    uint16_t fast[512]; // (length << 8) | symbol, 0 = not resolvable in 9 bits
    int32_t mincode[17], maxcode[18], valptr[17];
    uint8_t vals[256];
};

struct icl_je_interval {
    uint32_t first_sub; // index of the interval's first subsequence in the image (the stream pads every interval to whole subsequences)
    uint32_t nbits;     // unstuffed bits of the interval
};

// one image's scan.  The geometry comes from stage A0 (jpeg_decode.hip); the placement fields are filled by whoever lays the buffers out.
struct icl_je_scan {
    int32_t ncomp, hs, vs, bpm; // components, luma sampling, blocks per MCU
    int32_t mcux, mcuy;
    int32_t restart;    // MCUs per restart interval, 0 = none
    int32_t nintervals; // intervals found by the host scan of the stream
    int32_t sub_bits;
    uint32_t nsub; // subsequences of the image
    int32_t wblocks[3], hblocks[3];
    int32_t uniform; // every component decodes with the same DC and the same AC table: the block-within-MCU index stays 0 in the state
    int32_t pad_;
    int64_t coef_off[3];   // element offset of each component's dense int16 coefficients (natural order, 64 per block)
    int64_t stream_off;    // byte offset of the stream (nsub * sub_bits / 8 bytes)
    int64_t tables_off;    // byte offset of icl_je_table[2 * ncomp]: component c's DC table, then its AC table
    int64_t intervals_off; // byte offset of icl_je_interval[nintervals]
    int64_t sub_first;     // index of the image's first icl_je_sub in the state array
    int64_t wg_first;      // index of the image's first workgroup in the launch
};

// state of one subsequence between the launches
struct icl_je_sub {
    uint32_t entry_p, entry_bz; // bz = block-within-MCU | zig-zag index << 8
    uint32_t exit_p, exit_bz;
    uint32_t n, flags;     // blocks completed, ICL_JE_*
    int32_t dcsum[6];      // sum of the DC differences decoded here, by block phase: [q] holds the blocks k = q, q + bpm, .. since entry
    uint32_t first_block;  // decode-order index of the block in progress at entry (prefix sum of n)
    int32_t dcpred[3];     // DC predictor of each component at entry (segmented prefix sum of dcsum, reset at every interval)
};

struct icl_je_result {
    uint32_t p, bz, n, flags;
    int32_t dcsum[6];
};

// the component of phase q of a subsequence whose first block is first_block (interval starts are whole MCUs, so the index within
// the MCU is the decode-order index modulo bpm)
ICL_PX int icl_je_phase_comp(int ncomp, int nluma, int bpm, uint32_t first_block, int q);

ICL_PX int icl_je_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

ICL_PX int icl_je_comp_of(int ncomp, int nluma, uint32_t blk) { return ncomp == 1 ? 0 : ((int)blk < nluma ? 0 : ((int)blk == nluma ? 1 : 2)); }

struct icl_je_no_sink {
    ICL_PX void dc(uint32_t, int, int) {}
    ICL_PX void ac(uint32_t, int, int) {}
};

// Decodes the symbols that START in [entry p, sub_end) of one interval; a symbol is taken only if all its bits lie inside the
// interval (nbits), so nothing beyond the interval's last byte is ever used.  fetch(w) returns the 32 bits of stream word w (most
// significant bit first) and must be safe for every w; base_word is the interval's first word.  sink.dc(k, c, diff) / sink.ac(k, z, v)
// receive the values of the k-th block since entry (k = 0: the block in progress at entry; c is the component the STATE implies, which
// a sink that knows the block's place does not need).  uniform: all components share their tables, the state's block index stays 0.  The rules are those of decode_block
// (jpeg_decode.hip, sequential): same tables, same extension, same run / EOB / ZRL handling, same rejections.
template <class Fetch, class Sink>
ICL_PX void icl_je_decode_sub(const icl_je_table *T, int ncomp, int nluma, int bpm, bool uniform, Fetch &fetch, uint32_t base_word, uint32_t nbits, uint32_t sub_start,
                              uint32_t sub_end, uint32_t p, uint32_t bz, icl_je_result &out, Sink &sink)
{
    uint32_t blk = bz & 255u, z = bz >> 8, n = 0, flags = 0;
    uint32_t d0 = 0, d1 = 0, d2 = 0, d3 = 0, d4 = 0, d5 = 0; // DC sums per phase (scalars: an array indexed at run time would live in scratch on the GPU)
    uint32_t ph = 0;                                         // n % bpm
    if (uniform) blk = 0;
    // a symbol is at most 31 bits: a predecessor that stopped at its own end hands over p in [sub_start, sub_start + 30]
    if (blk >= (uint32_t)bpm || z > 63u || p < sub_start || p > sub_start + 30u || p > nbits) flags = ICL_JE_ERR;
    while (!flags && p < sub_end) {
        const int c = uniform ? 0 : icl_je_comp_of(ncomp, nluma, blk);
        const icl_je_table &t = T[2 * c + (z ? 1 : 0)];
        const uint32_t w = base_word + (p >> 5), o = p & 31u;
        const uint32_t hi = fetch(w), lo = fetch(w + 1);
        const uint32_t bits = o ? (hi << o) | (lo >> (32u - o)) : hi;
        const uint32_t avail = nbits - p;
        uint32_t len = 0, sym = 0;
        const uint32_t f = t.fast[bits >> 23];
        if (f) {
            len = f >> 8;
            sym = f & 255u;
        } else {
            const int code = (int)(bits >> 16);
            for (int l = 10; l <= 16; ++l) {
                const int cc = code >> (16 - l);
                if (t.maxcode[l] >= 0 && cc <= t.maxcode[l] && cc >= t.mincode[l]) {
                    sym = t.vals[(t.valptr[l] + cc - t.mincode[l]) & 255];
                    len = (uint32_t)l;
                    break;
                }
            }
            if (!len) { // no code: an error, unless the bits that would decide it lie beyond the interval
                flags = avail < 16u ? ICL_JE_SHORT : ICL_JE_ERR;
                break;
            }
        }
        if (z == 0) { // DC: category, then that many bits
            if (sym > 15u) { flags = ICL_JE_ERR; break; }
            if (len + sym > avail) { flags = ICL_JE_SHORT; break; }
            const int diff = sym ? icl_je_extend((int)((bits << len) >> (32u - sym)), (int)sym) : 0;
            switch (ph) {
            case 0: d0 += (uint32_t)diff; break;
            case 1: d1 += (uint32_t)diff; break;
            case 2: d2 += (uint32_t)diff; break;
            case 3: d3 += (uint32_t)diff; break;
            case 4: d4 += (uint32_t)diff; break;
            default: d5 += (uint32_t)diff; break;
            }
            sink.dc(n, c, diff);
            p += len + sym;
            z = 1;
            continue;
        }
        const uint32_t r = sym >> 4, sz = sym & 15u;
        if (sz == 0) {
            if (len > avail) { flags = ICL_JE_SHORT; break; }
            p += len;
            if (r == 15u && z + 16u < 64u) { z += 16u; continue; } // ZRL inside the block
            z = 64; // EOB, or a ZRL that runs past the last coefficient: the block is complete
        } else {
            if (z + r > 63u) { flags = ICL_JE_ERR; break; }
            if (len + sz > avail) { flags = ICL_JE_SHORT; break; }
            z += r;
            sink.ac(n, (int)z, icl_je_extend((int)((bits << len) >> (32u - sz)), (int)sz));
            p += len + sz;
            ++z;
        }
        if (z >= 64u) {
            z = 0;
            ++n;
            ph = ph + 1u == (uint32_t)bpm ? 0u : ph + 1u;
            if (!uniform) blk = blk + 1u == (uint32_t)bpm ? 0u : blk + 1u;
        }
    }
    if (flags & ICL_JE_ERR) { // a usable guess for the successor; the flag rejects the image if this result stays in the chain
        p = sub_end;
        blk = z = 0;
    }
    out.p = p;
    out.bz = blk | (z << 8);
    out.n = n;
    out.flags = flags;
    out.dcsum[0] = (int32_t)d0;
    out.dcsum[1] = (int32_t)d1;
    out.dcsum[2] = (int32_t)d2;
    out.dcsum[3] = (int32_t)d3;
    out.dcsum[4] = (int32_t)d4;
    out.dcsum[5] = (int32_t)d5;
}

ICL_PX int icl_je_phase_comp(int ncomp, int nluma, int bpm, uint32_t first_block, int q)
{
    return icl_je_comp_of(ncomp, nluma, (first_block + (uint32_t)q) % (uint32_t)bpm);
}

// ---- the chain / cleanliness check ----

ICL_PX int64_t icl_je_total_mcus(const icl_je_scan &S) { return (int64_t)S.mcux * S.mcuy; }

// the interval count of the host scan is ceil(MCUs / restart)
ICL_PX bool icl_je_scan_ok(const icl_je_scan &S)
{
    const int64_t m = icl_je_total_mcus(S);
    if (S.ncomp != 1 && S.ncomp != 3) return false;
    if (S.bpm != (S.ncomp == 1 ? 1 : S.hs * S.vs + 2) || S.mcux < 1 || S.mcuy < 1 || S.restart < 0 || S.nintervals < 1) return false;
    return (int64_t)S.nintervals == (S.restart ? (m + S.restart - 1) / S.restart : 1);
}

// subsequence j of interval k: its entry is the known start state (and the blocks before it are those of k whole intervals), or
// its predecessor's exit; what it decoded holds no error
ICL_PX bool icl_je_sub_ok(const icl_je_scan &S, int64_t k, uint32_t j, const icl_je_sub &s, uint32_t prev_exit_p, uint32_t prev_exit_bz)
{
    if (s.flags & ICL_JE_ERR) return false;
    if (j == 0) return s.entry_p == 0 && s.entry_bz == 0 && (int64_t)s.first_block == k * (int64_t)S.restart * S.bpm;
    return s.entry_p == prev_exit_p && s.entry_bz == prev_exit_bz;
}

// the last subsequence of an interval: the decode stopped between two MCUs, inside the interval's last byte
ICL_PX bool icl_je_interval_end_ok(uint32_t nbits, const icl_je_sub &s) { return s.exit_bz == 0 && s.exit_p <= nbits && nbits - s.exit_p < 8u; }

// all blocks of the image: with every interval start checked by icl_je_sub_ok, every interval then holds exactly its MCUs
ICL_PX bool icl_je_total_ok(const icl_je_scan &S, int64_t blocks) { return blocks == icl_je_total_mcus(S) * S.bpm; }

// where the b-th block in decode order lives: component, block index in the component's raster.  false: outside the image.
ICL_PX bool icl_je_block_place(const icl_je_scan &S, int64_t b, int &c, int64_t &idx)
{
    if (b < 0 || b >= icl_je_total_mcus(S) * S.bpm) return false;
    const int64_t m = b / S.bpm;
    const int q = (int)(b - m * S.bpm), nluma = S.ncomp == 1 ? 1 : S.hs * S.vs;
    const int64_t my = m / S.mcux, mx = m - my * S.mcux;
    int h = 1, v = 1, bx = 0, by = 0;
    c = icl_je_comp_of(S.ncomp, nluma, (uint32_t)q);
    if (c == 0 && S.ncomp == 3) {
        h = S.hs;
        v = S.vs;
        by = q / h;
        bx = q - by * h;
    }
    const int64_t X = mx * h + bx, Y = my * v + by;
    if (X >= S.wblocks[c] || Y >= S.hblocks[c]) return false;
    idx = Y * S.wblocks[c] + X;
    return true;
}
