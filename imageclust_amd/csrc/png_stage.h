// png_stage.h -- host stage P0 of the PNG reader (png_decode.hip): the parse step that icl_png_decode and the GPU route of the batched
// file path (jpeg_gpu.hip, png_gpu.hip) share, the rule that says which files the GPU route takes, and the host rehearsal of the
// kernels' schedule behind icl_png_raw_file_host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "png_inflate.h"

struct icl_png_pass { // one reduced image of the stream (PNG 8.2): the whole image, or an Adam7 pass
    uint32_t xs, ys, dx, dy, pw, ph;
    size_t rowb, off;
};

struct icl_png_parsed {
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = 0, interlace = 0, npal = 0, channels = 0;
    uint8_t pal[256][3];
    size_t bits_px = 0, bpp = 0;
    icl_png_pass passes[7];
    int npass = 0;
    size_t want = 0; // bytes the zlib stream must inflate to: every pass's rows, each with its filter byte
};

// The chunk walk: signature, lengths, CRC-32, IHDR legality, PLTE, IDAT concatenation, IEND, the zlib header, the pass geometry and
// `want`.  The IDAT bodies are APPENDED to z (the zlib stream is z[z0 ..) for the z0 = z.size() of the call).  Returns NULL, or what
// icl_png_decode's message says is wrong with the file.
const char *icl_png_parse(const uint8_t *data, size_t len, icl_png_parsed &P, std::vector<uint8_t> &z);

// What the GPU route takes: not Adam7-interlaced, descriptor + stream within one slab's payload, `want` within the slab's scratch.
constexpr int64_t ICL_PNG_PAYLOAD_CAP = 128ll << 20; // (= jpeg_gpu.hip's SLAB_PAYLOAD)
constexpr int64_t ICL_PNG_WANT_CAP = 512ll << 20;    // (<= jpeg_gpu.hip's SLAB_SCRATCH)
static inline bool icl_png_qualifies(const icl_png_parsed &P, size_t zbytes)
{
    return !P.interlace && zbytes >= 6 && (int64_t)sizeof(icl_png_desc) + (((int64_t)zbytes + 15) & ~(int64_t)15) <= ICL_PNG_PAYLOAD_CAP && (int64_t)P.want <= ICL_PNG_WANT_CAP;
}
// the descriptor of a qualifying file (z: its zlib stream)
void icl_png_describe(const icl_png_parsed &P, const uint8_t *z, size_t zbytes, icl_png_desc &D);

// The kernels' schedule as a host loop over png_inflate.h (no GPU): inflate + Adler-32 (stage 0), then the banded, skewed unfilter and the
// palette check (stage 1), then the sample-to-RGB rule on every pixel (stage 2).  raw receives the stage's bytes when state is 1.
// info[12]: state (1 accepted, 0 rejected, -1 does not qualify), w, h, depth, colour type, stored / fixed / dynamic blocks, longest code
// length, largest distance, matches with distance < length, matches whose destination wraps the ring.
void icl_png_host_schedule(const uint8_t *data, size_t len, int stage, std::vector<uint8_t> &raw, int32_t info[12]);
