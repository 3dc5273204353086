// jpeg_huff_gpu.hip -- the entropy decoder of baseline JPEG scans on the GPU (ICL_ENTROPY_GPU; the pipeline around it is jpeg_gpu.hip).
//
// One thread per subsequence of ICL_JE_SUB_BITS bits of an image's unstuffed stream, ICL_JE_WG subsequences per workgroup; a workgroup
// stages its part of the stream (coalesced 16-byte loads, rows padded by one word so that 64 lanes walking 64 rows hit 64 banks) and the
// image's Huffman tables in LDS.  The decode step and every acceptance rule are those of jpeg_entropy.h, which the host loop
// (icl_je_host_decode) shares.
//   jpeg_huff_sync_kernel   x ICL_JE_LAUNCHES: decode from a guessed entry state, then take over the predecessor's exit state for as many
//                           rounds as entry states change (at most ICL_JE_ROUNDS).  A workgroup's first thread takes the exit state the
//                           preceding workgroup published in the PREVIOUS launch (two alternating arrays): no workgroup waits for another.
//   jpeg_huff_check_kernel  one workgroup per image: chain and cleanliness check -> accepted flag; prefix sum of completed blocks (every
//                           subsequence's first output block) and the DC predictors as a segmented prefix sum per component in decode
//                           order, reset at every restart interval.
//   jpeg_huff_write_kernel  accepted images only: decode once more from the validated entry states and store the coefficients, natural
//                           order, dense int16 (the buffer is zero-filled before: blocks end at their EOB).
// Every offset and count a kernel takes from a descriptor or derives from stream bytes is checked against its buffer.
#include "icl_common.h"
#include "jpeg_entropy.h"
#include "jpeg_stage.h"

namespace {

constexpr int SUB_WORDS = ICL_JE_SUB_BITS / 32;
constexpr int ROW = SUB_WORDS + 1;             // LDS row stride in words
constexpr int STAGE_ROWS = ICL_JE_WG + 1;      // one more subsequence: the last thread's final symbol may end in it
constexpr int TABLE_WORDS = (int)(sizeof(icl_je_table) / 4);
static_assert(sizeof(icl_je_table) % 4 == 0 && ICL_JE_SUB_BITS % 128 == 0 && ICL_JE_WG == 256, "layout");

struct lds_fetch {
    const uint32_t *words;
    uint32_t first_word; // stream word held at words[0]
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const
    {
        const uint32_t x = w - first_word;
        if (x >= (uint32_t)(STAGE_ROWS * SUB_WORDS)) return 0;
        return __builtin_bswap32(words[(x / SUB_WORDS) * ROW + (x % SUB_WORDS)]);
    }
};

// what a thread of the decode kernels knows after the common prologue
struct sub_view {
    bool wg_ok;  // the descriptor is usable (uniform over the workgroup)
    bool active; // this thread owns a subsequence with a consistent interval
    int scan;
    uint32_t i, j; // subsequence in the image, in its interval
    int64_t k;     // interval
    uint32_t base_word, nbits, start, end;
    uint32_t wgl;  // workgroup within the image
};

__device__ __forceinline__ bool scan_usable(const icl_je_scan &S, int64_t payload_bytes, int64_t nsub_cap, int64_t nwg_cap)
{
    if (S.sub_bits != ICL_JE_SUB_BITS || (S.ncomp != 1 && S.ncomp != 3) || S.nsub < 1 || S.nintervals < 1) return false;
    if (S.ncomp == 3 && !icl_luma_sampling_ok(S.hs, S.vs)) return false;
    if (S.bpm != (S.ncomp == 1 ? 1 : S.hs * S.vs + 2)) return false;
    const int64_t nwg = ((int64_t)S.nsub + ICL_JE_WG - 1) / ICL_JE_WG;
    if (S.tables_off < 0 || (S.tables_off & 3) || S.tables_off + (int64_t)(2 * S.ncomp) * (int64_t)sizeof(icl_je_table) > payload_bytes) return false;
    if (S.intervals_off < 0 || (S.intervals_off & 3) || S.intervals_off + (int64_t)S.nintervals * (int64_t)sizeof(icl_je_interval) > payload_bytes) return false;
    if (S.stream_off < 0 || (S.stream_off & 15) || S.stream_off + (int64_t)S.nsub * (ICL_JE_SUB_BITS / 8) > payload_bytes) return false;
    return S.sub_first >= 0 && S.sub_first + (int64_t)S.nsub <= nsub_cap && S.wg_first >= 0 && S.wg_first + nwg <= nwg_cap;
}

// workgroup -> image, tables and stream rows into LDS, subsequence -> interval
__device__ __forceinline__ sub_view wg_prologue(const icl_je_scan *__restrict__ scans, int nscans, const uint8_t *__restrict__ payload, int64_t payload_bytes,
                                                int64_t nsub_cap, int64_t nwg_cap, icl_je_table *T, uint32_t *words)
{
    sub_view V = {};
    int lo = 0, hi = nscans - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (scans[mid].wg_first <= (int64_t)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    V.scan = lo;
    const icl_je_scan &S = scans[lo];
    const int64_t wgl = (int64_t)blockIdx.x - S.wg_first;
    V.wg_ok = scan_usable(S, payload_bytes, nsub_cap, nwg_cap) && wgl >= 0 && wgl * ICL_JE_WG < (int64_t)S.nsub;
    if (!V.wg_ok) return V;
    V.wgl = (uint32_t)wgl;
    const uint32_t first_sub = V.wgl * ICL_JE_WG, total_words = S.nsub * SUB_WORDS;
    const uint32_t *tw = (const uint32_t *)(payload + S.tables_off);
    for (int x = threadIdx.x; x < 2 * S.ncomp * TABLE_WORDS; x += ICL_JE_WG) ((uint32_t *)T)[x] = tw[x];
    const uint4 *sw = (const uint4 *)(payload + S.stream_off);
    for (uint32_t x = threadIdx.x * 4; x < (uint32_t)(STAGE_ROWS * SUB_WORDS); x += ICL_JE_WG * 4) {
        const uint32_t g = first_sub * SUB_WORDS + x;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g + 3 < total_words) v = sw[g >> 2];
        uint32_t *o = words + (x / SUB_WORDS) * ROW + (x % SUB_WORDS);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
    V.i = first_sub + threadIdx.x;
    if (V.i < S.nsub) {
        const icl_je_interval *iv = (const icl_je_interval *)(payload + S.intervals_off);
        int a = 0, b = S.nintervals - 1;
        while (a < b) {
            const int mid = (a + b + 1) >> 1;
            if (iv[mid].first_sub <= V.i) a = mid;
            else b = mid - 1;
        }
        const uint32_t f = iv[a].first_sub, nx = a + 1 < S.nintervals ? iv[a + 1].first_sub : S.nsub;
        const uint32_t nb = iv[a].nbits;
        // the interval holds this subsequence, and its bits lie inside its subsequences
        if (f <= V.i && V.i < nx && nx <= S.nsub && (uint64_t)nb <= (uint64_t)(nx - f) * ICL_JE_SUB_BITS) {
            V.active = true;
            V.k = a;
            V.j = V.i - f;
            V.base_word = f * SUB_WORDS;
            V.nbits = nb;
            const uint64_t s0 = (uint64_t)V.j * ICL_JE_SUB_BITS;
            V.start = (uint32_t)(s0 < nb ? s0 : nb);
            V.end = (uint32_t)(s0 + ICL_JE_SUB_BITS < nb ? s0 + ICL_JE_SUB_BITS : nb);
        }
    }
    __syncthreads();
    return V;
}

__global__ void __launch_bounds__(ICL_JE_WG) jpeg_huff_sync_kernel(const icl_je_scan *__restrict__ scans, int nscans, const uint8_t *__restrict__ payload,
                                                                   int64_t payload_bytes, icl_je_sub *__restrict__ subs, int64_t nsub_cap,
                                                                   const uint32_t *__restrict__ bound_in, uint32_t *__restrict__ bound_out, int64_t nwg_cap, int launch)
{
    __shared__ icl_je_table T[6];
    __shared__ uint32_t words[STAGE_ROWS * ROW];
    __shared__ uint32_t ex_p[ICL_JE_WG], ex_bz[ICL_JE_WG];
    const sub_view V = wg_prologue(scans, nscans, payload, payload_bytes, nsub_cap, nwg_cap, T, words);
    if (!V.wg_ok) return;
    const icl_je_scan &S = scans[V.scan];
    const int ncomp = S.ncomp, nluma = ncomp == 1 ? 1 : S.hs * S.vs, bpm = S.bpm;
    const bool uniform = S.uniform != 0;
    lds_fetch fetch{words, V.wgl * ICL_JE_WG * SUB_WORDS};
    icl_je_no_sink none;
    icl_je_sub *me = subs + S.sub_first + V.i; // (V.i < nsub <= the image's share of subs when active)
    uint32_t ep = 0, ebz = 0;
    icl_je_result R = {};
    if (V.active) {
        bool run = true;
        if (launch == 0) { // the guess: a block starts at the subsequence's first bit (the truth for the first one of an interval)
            ep = V.start;
        } else {
            ep = me->entry_p;
            ebz = me->entry_bz;
            R.p = me->exit_p;
            R.bz = me->exit_bz;
            R.n = me->n;
            R.flags = me->flags;
#pragma unroll
            for (int q = 0; q < 6; ++q) R.dcsum[q] = me->dcsum[q];
            run = false;
            if (threadIdx.x == 0 && V.j > 0 && V.wgl > 0) { // what the preceding workgroup published in the previous launch
                const uint32_t *b = bound_in + 2 * (S.wg_first + V.wgl - 1);
                if (b[0] != ep || b[1] != ebz) {
                    ep = b[0];
                    ebz = b[1];
                    run = true;
                }
            }
        }
        if (run) icl_je_decode_sub(T, ncomp, nluma, bpm, uniform, fetch, V.base_word, V.nbits, V.start, V.end, ep, ebz, R, none);
    }
    ex_p[threadIdx.x] = R.p;
    ex_bz[threadIdx.x] = R.bz;
    for (int r = 1; r <= ICL_JE_ROUNDS; ++r) {
        __syncthreads();
        uint32_t np = 0, nbz = 0;
        bool ch = false;
        if (V.active && threadIdx.x > 0 && V.j > 0) {
            np = ex_p[threadIdx.x - 1];
            nbz = ex_bz[threadIdx.x - 1];
            ch = np != ep || nbz != ebz;
        }
        if (!__syncthreads_or(ch)) break; // a fixed point: further rounds would change nothing
        if (ch) {
            ep = np;
            ebz = nbz;
            icl_je_decode_sub(T, ncomp, nluma, bpm, uniform, fetch, V.base_word, V.nbits, V.start, V.end, ep, ebz, R, none);
            ex_p[threadIdx.x] = R.p;
            ex_bz[threadIdx.x] = R.bz;
        }
    }
    if (V.i < S.nsub) {
        if (!V.active) R.flags = ICL_JE_ERR;
        me->entry_p = ep;
        me->entry_bz = ebz;
        me->exit_p = R.p;
        me->exit_bz = R.bz;
        me->n = R.n;
        me->flags = R.flags;
#pragma unroll
        for (int q = 0; q < 6; ++q) me->dcsum[q] = R.dcsum[q];
        if (threadIdx.x == ICL_JE_WG - 1 || V.i + 1 == S.nsub) {
            uint32_t *b = bound_out + 2 * (S.wg_first + V.wgl);
            b[0] = R.p;
            b[1] = R.bz;
        }
    }
}

__global__ void __launch_bounds__(ICL_JE_WG) jpeg_huff_check_kernel(const icl_je_scan *__restrict__ scans, int nscans, const uint8_t *__restrict__ payload,
                                                                    int64_t payload_bytes, icl_je_sub *__restrict__ subs, int64_t nsub_cap, int64_t nwg_cap,
                                                                    int32_t *__restrict__ accepted)
{
    __shared__ uint32_t s_n[ICL_JE_WG];
    __shared__ uint32_t s_dc[3][ICL_JE_WG];
    __shared__ uint32_t s_reset[ICL_JE_WG];
    const int img = blockIdx.x;
    if (img >= nscans) return;
    const icl_je_scan &S = scans[img];
    const int t = threadIdx.x;
    if (!scan_usable(S, payload_bytes, nsub_cap, nwg_cap)) {
        if (t == 0) accepted[img] = 0;
        return;
    }
    const icl_je_interval *iv = (const icl_je_interval *)(payload + S.intervals_off);
    icl_je_sub *sub = subs + S.sub_first;
    const uint32_t nsub = S.nsub;
    const int nint = S.nintervals;
    bool ok = icl_je_scan_ok(S);
    // the interval list itself: starts at 0, strictly increasing, every interval's bits inside its subsequences
    for (int k = t; k < nint; k += ICL_JE_WG) {
        const uint32_t f = iv[k].first_sub, nx = k + 1 < nint ? iv[k + 1].first_sub : nsub;
        ok = ok && f < nx && nx <= nsub && (k > 0 || f == 0) && (uint64_t)iv[k].nbits <= (uint64_t)(nx - f) * ICL_JE_SUB_BITS;
    }
    ok = __syncthreads_and(ok);
    if (!ok) { // (uniform) nothing below may trust the list
        if (t == 0) accepted[img] = 0;
        return;
    }
    const uint32_t chunk = (nsub + ICL_JE_WG - 1) / ICL_JE_WG;
    const uint32_t a = min((uint32_t)t * chunk, nsub), b = min(a + chunk, nsub);
    auto interval_of = [&](uint32_t i) {
        int x = 0, y = nint - 1;
        while (x < y) {
            const int mid = (x + y + 1) >> 1;
            if (iv[mid].first_sub <= i) x = mid;
            else y = mid - 1;
        }
        return x;
    };
    const int ncomp = S.ncomp, nluma = ncomp == 1 ? 1 : S.hs * S.vs, bpm = S.bpm; // (bpm is 1, 3, 4 or 6: scan_usable; 4 is 2x1 or 1x2, 6 is 2x2, 4x1 or 1x4)
    __shared__ uint32_t s_total;
    // pass 1: this chunk's blocks; exclusive scan over the 256 chunks
    {
        uint32_t n = 0;
        for (uint32_t i = a; i < b; ++i) n += sub[i].n;
        s_n[t] = n;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t n = 0;
        for (int x = 0; x < ICL_JE_WG; ++x) {
            const uint32_t cn = s_n[x];
            s_n[x] = n;
            n += cn;
        }
        s_total = n; // all blocks of the image
    }
    __syncthreads();
    // pass 2: every subsequence's first block; with it the component of each DC phase: this chunk's DC sums per component (since
    // the last interval start inside the chunk); segmented exclusive scan over the chunks
    {
        uint32_t n = s_n[t], dc[3] = {0, 0, 0}, reset = 0;
        int k = a < b ? interval_of(a) : 0;
        for (uint32_t i = a; i < b; ++i) {
            while (k + 1 < nint && iv[k + 1].first_sub <= i) ++k;
            if (i == iv[k].first_sub) {
                dc[0] = dc[1] = dc[2] = 0;
                reset = 1;
            }
            sub[i].first_block = n;
            for (int q = 0; q < bpm; ++q) {
                const int c = icl_je_phase_comp(ncomp, nluma, bpm, n, q);
                const uint32_t v = (uint32_t)sub[i].dcsum[q];
                dc[0] += c == 0 ? v : 0u;
                dc[1] += c == 1 ? v : 0u;
                dc[2] += c == 2 ? v : 0u;
            }
            n += sub[i].n;
        }
        s_reset[t] = reset;
        for (int c = 0; c < 3; ++c) s_dc[c][t] = dc[c];
    }
    __syncthreads();
    if (t == 0) {
        uint32_t dc[3] = {0, 0, 0};
        for (int x = 0; x < ICL_JE_WG; ++x) {
            const uint32_t cr = s_reset[x];
            for (int c = 0; c < 3; ++c) {
                const uint32_t cd = s_dc[c][x];
                s_dc[c][x] = dc[c];
                dc[c] = cr ? cd : dc[c] + cd;
            }
        }
    }
    __syncthreads();
    // pass 3: the DC predictors of every subsequence, and the checks
    {
        uint32_t dc[3] = {s_dc[0][t], s_dc[1][t], s_dc[2][t]};
        int k = a < b ? interval_of(a) : 0;
        for (uint32_t i = a; i < b; ++i) {
            while (k + 1 < nint && iv[k + 1].first_sub <= i) ++k;
            const uint32_t f = iv[k].first_sub, nx = k + 1 < nint ? iv[k + 1].first_sub : nsub;
            if (i == f) dc[0] = dc[1] = dc[2] = 0;
            const icl_je_sub &s = sub[i]; // (read in place: a copy indexed by the phase would live in scratch)
            for (int c = 0; c < 3; ++c) sub[i].dcpred[c] = (int32_t)dc[c];
            uint32_t pp = 0, pbz = 0;
            if (i > 0) {
                pp = sub[i - 1].exit_p;
                pbz = sub[i - 1].exit_bz;
            }
            ok = ok && icl_je_sub_ok(S, k, i - f, s, pp, pbz);
            if (i + 1 == nx) ok = ok && icl_je_interval_end_ok(iv[k].nbits, s);
            for (int q = 0; q < bpm; ++q) {
                const int c = icl_je_phase_comp(ncomp, nluma, bpm, s.first_block, q);
                const uint32_t v = (uint32_t)s.dcsum[q];
                dc[0] += c == 0 ? v : 0u;
                dc[1] += c == 1 ? v : 0u;
                dc[2] += c == 2 ? v : 0u;
            }
        }
    }
    ok = ok && icl_je_total_ok(S, (int64_t)s_total);
    ok = __syncthreads_and(ok);
    if (t == 0) accepted[img] = ok ? 1 : 0;
}

struct coef_sink { // dense int16, natural order; the DC value is stage A's (int16_t) of the int predictor
    const icl_je_scan &S;
    int16_t *coef;
    int64_t coef_elems;
    int64_t first;
    uint32_t pred0, pred1, pred2; // (scalars: a register array indexed by the component would live in scratch)
    int64_t cur;
    int cur_c;    // the component of the current block (from its place, not from the state)
    int64_t base; // element offset of the current block, -1: outside
    __device__ __forceinline__ int64_t at(uint32_t k)
    {
        if ((int64_t)k != cur) {
            int c = 0;
            int64_t idx;
            cur = k;
            base = -1;
            const bool in = icl_je_block_place(S, first + k, c, idx);
            cur_c = c;
            if (in) {
                const int64_t o = S.coef_off[c] + idx * 64;
                if (S.coef_off[c] >= 0 && o + 64 <= coef_elems) base = o;
            }
        }
        return base;
    }
    __device__ __forceinline__ void dc(uint32_t k, int, int diff)
    {
        const int64_t o = at(k);
        if (o < 0) return;
        const int c = cur_c;
        const uint32_t v = (c == 0 ? pred0 : (c == 1 ? pred1 : pred2)) + (uint32_t)diff;
        if (c == 0) pred0 = v;
        else if (c == 1) pred1 = v;
        else pred2 = v;
        coef[o] = (int16_t)(int32_t)v;
    }
    __device__ __forceinline__ void ac(uint32_t k, int z, int v)
    {
        const int64_t o = at(k);
        if (o >= 0) coef[o + icl_zigzag[z & 63]] = (int16_t)v;
    }
};

__global__ void __launch_bounds__(ICL_JE_WG) jpeg_huff_write_kernel(const icl_je_scan *__restrict__ scans, int nscans, const uint8_t *__restrict__ payload,
                                                                    int64_t payload_bytes, const icl_je_sub *__restrict__ subs, int64_t nsub_cap, int64_t nwg_cap,
                                                                    const int32_t *__restrict__ accepted, int16_t *__restrict__ coef, int64_t coef_elems)
{
    __shared__ icl_je_table T[6];
    __shared__ uint32_t words[STAGE_ROWS * ROW];
    const sub_view V = wg_prologue(scans, nscans, payload, payload_bytes, nsub_cap, nwg_cap, T, words);
    if (!V.wg_ok || !accepted[V.scan] || !V.active) return; // (no barrier below)
    const icl_je_scan &S = scans[V.scan];
    const icl_je_sub &me = subs[S.sub_first + V.i];
    lds_fetch fetch{words, V.wgl * ICL_JE_WG * SUB_WORDS};
    coef_sink sink{S, coef, coef_elems, (int64_t)me.first_block, (uint32_t)me.dcpred[0], (uint32_t)me.dcpred[1], (uint32_t)me.dcpred[2], -1, 0, -1};
    icl_je_result R;
    icl_je_decode_sub(T, S.ncomp, S.ncomp == 1 ? 1 : S.hs * S.vs, S.bpm, S.uniform != 0, fetch, V.base_word, V.nbits, V.start, V.end, me.entry_p, me.entry_bz, R, sink);
}

} // namespace

int icl_je_decode_slab(icl_ctx *ctx, hipStream_t st, const icl_je_slab &s)
{
    if (s.nscans <= 0 || s.total_wgs <= 0) return ICL_OK;
    if (s.total_wgs > s.nwg_cap || s.total_wgs > 0x7fffffff) return icl_fail(ctx, ICL_ERR_ARG, "entropy decode: slab larger than its workspace");
    for (int l = 0; l < ICL_JE_LAUNCHES; ++l) {
        hipLaunchKernelGGL(jpeg_huff_sync_kernel, dim3((unsigned)s.total_wgs), dim3(ICL_JE_WG), 0, st, s.d_scans, s.nscans, s.d_payload, s.payload_bytes, s.d_sub,
                           s.nsub_cap, (const uint32_t *)(s.d_bound + ((l + 1) & 1) * 2 * s.nwg_cap), s.d_bound + (l & 1) * 2 * s.nwg_cap, s.nwg_cap, l);
        ICL_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(jpeg_huff_check_kernel, dim3((unsigned)s.nscans), dim3(ICL_JE_WG), 0, st, s.d_scans, s.nscans, s.d_payload, s.payload_bytes, s.d_sub, s.nsub_cap,
                       s.nwg_cap, s.d_accepted);
    ICL_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(jpeg_huff_write_kernel, dim3((unsigned)s.total_wgs), dim3(ICL_JE_WG), 0, st, s.d_scans, s.nscans, s.d_payload, s.payload_bytes,
                       (const icl_je_sub *)s.d_sub, s.nsub_cap, s.nwg_cap, (const int32_t *)s.d_accepted, s.d_coef, s.coef_elems);
    ICL_HIP(ctx, hipGetLastError());
    return ICL_OK;
}
