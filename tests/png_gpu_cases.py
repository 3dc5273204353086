"""The PNG corpus of the GPU PNG route's tests (tests/test_png_gpu_schedule_cpu.py, test_png_gpu_schedule_asan_cpu.py,
test_png_ingest_gpu.py): generators for every block kind, code shape, match shape, filter, colour type and size the kernels take another
path for, and a small DEFLATE writer that emits exact sequences -- with fixed codes, or with dynamic codes from given lengths -- for
the cases zlib never produces (marked + below).  cases() -> list of dicts: name, data (the PNG's bytes), kind ("clean" / "reject" /
"unqualified"), and for a reject the message icl_decode_image_file gives for it."""
import heapq
import struct
import zlib

import numpy as np

DEFLATE_MSG = "corrupt or truncated DEFLATE stream"
ADLER_MSG = "Adler-32 mismatch"
FILTER_MSG = "unknown scanline filter"
PALETTE_MSG = "palette index out of range"

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CL_LENS = [5] * 16 + [2, 3, 3]  # a complete code-length code: 16 x 2^-5 + 2^-2 + 2 x 2^-3 = 1


# ---- the DEFLATE writer (RFC 1951) ------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, k):  # a k-bit field, least significant bit first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):  # a Huffman code (value, length), most significant bit first
        v, k = c
        self.put(int(format(v, "0%db" % k)[::-1], 2), k)

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths (an over-subscribed set gives codes nobody decodes)."""
    codes, code = {}, 0
    for k in range(1, 16):
        for s, l in enumerate(lens):
            if l == k:
                codes[s] = (code & ((1 << k) - 1), k)
                code += 1
        code <<= 1
    return codes


def huffman_lens(freq, nsym):
    """Plain Huffman code lengths over the used symbols (at least two, so that the code is complete)."""
    used = [s for s in range(nsym) if freq.get(s, 0)]
    for s in range(nsym):
        if len(used) >= 2:
            break
        if s not in used:
            used.append(s)
    heap = [(freq.get(s, 0) or 1, s, (s,)) for s in used]
    heapq.heapify(heap)
    lens = [0] * nsym
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    assert max(lens) <= 15
    return lens


def length_symbol(n):
    s = max(i for i in range(29) if LBASE[i] <= n)
    if n == 258:
        s = 28
    return 257 + s, LEXT[s], n - LBASE[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DBASE[i] <= d)
    return s, DEXT[s], d - DBASE[s]


def op_symbols(ops):
    """ops: ("lit", bytes) | ("match", length, distance) | ("raw", literal/length symbol, extra bits, extra value[, distance symbol,
    extra bits, extra value]) -> the same as raw symbol tuples."""
    for op in ops:
        if op[0] == "lit":
            for b in op[1]:
                yield (b, 0, 0)
        elif op[0] == "match":
            yield length_symbol(op[1]) + dist_symbol(op[2])
        else:
            yield tuple(op[1:])


def rle_lengths(seq):
    """the code-length alphabet over ONE sequence (literal / length lengths followed by distance lengths, so that a repeat may run
    from the one into the other) -> [(symbol, extra bits, extra value)]"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((17, 3, r - 3) if r <= 10 else (18, 7, r - 11))
            i += r
        elif run >= 4:
            out.append((v, 0, 0))
            r = min(run - 1, 6)
            out.append((16, 2, r - 3))
            i += 1 + r
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def write_block(bw, ops, final, lit_lens=None, dist_lens=None, eob=True):
    """One block with the fixed codes, or (lit_lens given) with dynamic codes of exactly these lengths -- legal or not."""
    bw.put(1 if final else 0, 1)
    if lit_lens is None:
        bw.put(1, 2)
        lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
    else:
        bw.put(2, 2)
        bw.put(len(lit_lens) - 257, 5)
        bw.put(len(dist_lens) - 1, 5)
        bw.put(19 - 4, 4)
        for s in CLORDER:
            bw.put(CL_LENS[s], 3)
        cl = canonical(CL_LENS)
        for s, k, v in rle_lengths(list(lit_lens) + list(dist_lens)):
            bw.code(cl[s])
            bw.put(v, k)
        lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in op_symbols(ops):
        if t[0] not in lit:
            return  # (an illegal table: the header is what the case is about)
        bw.code(lit[t[0]])
        bw.put(t[2], t[1])
        if len(t) > 3:
            bw.code(dist.get(t[3], (0, 1)))
            bw.put(t[5], t[4])
    if eob and 256 in lit:
        bw.code(lit[256])


def dynamic_lens(ops):
    """Huffman lengths for what ops use (+ end of block): (literal / length lengths, distance lengths)"""
    fl, fd = {256: 1}, {}
    for t in op_symbols(ops):
        fl[t[0]] = fl.get(t[0], 0) + 1
        if len(t) > 3:
            fd[t[3]] = fd.get(t[3], 0) + 1
    ll = huffman_lens(fl, 286)
    dl = huffman_lens(fd, 30) if fd else [0]
    while len(ll) > 257 and ll[-1] == 0:
        ll.pop()
    while len(dl) > 1 and dl[-1] == 0:
        dl.pop()
    return ll, dl


class Sim:
    """Collects ops and what they inflate to."""

    def __init__(self):
        self.ops, self.out = [], bytearray()

    def lit(self, b):
        self.ops.append(("lit", bytes(b)))
        self.out += b

    def match(self, n, d):
        assert 3 <= n <= 258 and 1 <= d <= len(self.out) and d <= 32768
        self.ops.append(("match", n, d))
        for _ in range(n):
            self.out.append(self.out[-d])

    def fill_to(self, n, rng, hi=5):
        if n > len(self.out):
            self.lit(rng.integers(0, hi, n - len(self.out), dtype=np.uint8).tobytes())


def zwrap(deflate, raw, adler=None):
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(bytes(raw)) & 0xFFFFFFFF if adler is None else adler)


def zdeflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)  # (raw DEFLATE: zwrap adds header and trailer)
    if sync_at is None:
        return c.compress(bytes(raw)) + c.flush()
    return c.compress(bytes(raw[:sync_at])) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(bytes(raw[sync_at:])) + c.flush()


# ---- PNG framing ------------------------------------------------------------------------------------------------------
def chunk(t, body):
    return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xFFFFFFFF)


def png_of(w, h, depth, ctype, z, extra=b"", interlace=0, idat=0):
    """A PNG around the zlib stream z; idat: bytes per IDAT chunk (0: one chunk)."""
    step = idat or max(1, len(z))
    body = b"".join(chunk(b"IDAT", z[i:i + step]) for i in range(0, len(z), step))
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) + extra + body + chunk(b"IEND", b"")


CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def row_bytes(w, depth, ctype):
    return (w * CHANNELS[ctype] * depth + 7) // 8


def scanlines(w, h, depth, ctype, rng, filters=None, hi=256):
    """Random FILTERED bytes under the given (or random) filter bytes: every such stream is a legal image."""
    rb = row_bytes(w, depth, ctype)
    a = np.zeros((h, rb + 1), np.uint8)
    a[:, 1:] = rng.integers(0, hi, (h, rb), dtype=np.uint8)
    a[:, 0] = rng.integers(0, 5, h, dtype=np.uint8) if filters is None else np.resize(np.asarray(filters, np.uint8), h)
    return a


def photo_raw(w, h, seed):
    """RGB 8-bit photo-like content (a gradient + noise), rows Sub- or Up-filtered; two equal rows in the middle and three blank ones."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    px = np.stack([(x * 2 + y) % 256, (x + y * 3) % 256, (x * y // 7) % 256], 2).astype(np.int32) + rng.integers(0, 6, (h, w, 3))
    px = (px % 256).astype(np.int32)
    if h > 8:
        px[h // 2] = px[h // 2 - 1]
        px[h // 2 + 2:h // 2 + 5] = 0
    rows = px.reshape(h, w * 3)
    a = np.zeros((h, w * 3 + 1), np.uint8)
    for r in range(h):
        if r % 2 == 0 or r == 0:
            a[r, 0] = 1
            a[r, 1:] = (rows[r] - np.r_[np.zeros(3, np.int32), rows[r][:-3]]) & 255
        else:
            a[r, 0] = 2
            a[r, 1:] = (rows[r] - rows[r - 1]) & 255
    return a


def unsampled(n, out=224):
    """a source coordinate the 224-wide INTER_LINEAR resize of n samples never reads"""
    used = set()
    for d in range(out):
        s = int(np.floor((d + 0.5) * n / out - 0.5))
        used |= {min(max(s, 0), n - 1), min(max(s + 1, 0), n - 1)}
    return next(v for v in range(n // 2, n) if v not in used)


def cases():
    out = []

    def add(name, data, kind="clean", message=None):
        out.append({"name": name, "data": data, "kind": kind, "message": message})

    def rgb(name, a, w, h, z=None, **kw):
        add(name, png_of(w, h, 8, 2, z if z is not None else zwrap(zdeflate(a.tobytes()), a.tobytes()), **kw))

    # ---- block kinds: a raw size just over 32 KiB (128 x 100 RGB), so the stored block is longer than the ring
    w, h = 128, 100
    a = photo_raw(w, h, 1)
    raw = a.tobytes()
    assert 32768 < len(raw) < 65536
    rgb("blocks_stored", a, w, h, zwrap(zdeflate(raw, 0), raw))
    rgb("blocks_fixed", a, w, h, zwrap(zdeflate(raw, 6, zlib.Z_FIXED), raw))
    rgb("blocks_dynamic", a, w, h)
    rgb("blocks_sync_flush", a, w, h, zwrap(zdeflate(raw, 6, sync_at=(h // 2) * (w * 3 + 1) + 1), raw))  # between the two equal rows
    rgb("blocks_huffman_only", a, w, h, zwrap(zdeflate(raw, 6, zlib.Z_HUFFMAN_ONLY), raw))
    rgb("blocks_rle", a, w, h, zwrap(zdeflate(raw, 6, zlib.Z_RLE), raw))
    s = photo_raw(16, 16, 2)
    rgb("blocks_idat_1byte", s, 16, 16, idat=1)
    b = photo_raw(160, 140, 3)
    assert b.size > 65536
    rgb("size_over_64k", b, 160, 140)
    rgb("size_over_64k_stored", b, 160, 140, zwrap(zdeflate(b.tobytes(), 0), b.tobytes()))  # two stored blocks
    # ---- codes
    rng = np.random.default_rng(5)
    fib = [1, 1]  # Fibonacci-like weights, each one more than the sum of the two before it: no ties for the code builder to flatten
    while sum(fib) + fib[-1] + fib[-2] + 1 < 16000:  # one block (zlib closes a block after 16383 symbols)
        fib.append(fib[-1] + fib[-2] + 1)
    pool = np.repeat(np.arange(1, len(fib) + 1, dtype=np.uint8), fib)
    gw, gh = pool.size, 1
    body = rng.permutation(pool).reshape(gh, gw)
    g = np.zeros((gh, gw + 1), np.uint8)
    g[:, 1:] = body
    add("codes_15bit", png_of(gw, gh, 8, 0, zwrap(zdeflate(g.tobytes(), 6, zlib.Z_HUFFMAN_ONLY), g.tobytes())))
    # + a dynamic header whose repeat code 16 runs from the literal lengths into the distance lengths
    sim = Sim()
    g2 = scanlines(31, 8, 8, 0, rng, filters=[0], hi=4)
    sim.lit(g2.tobytes()[:100])
    sim.match(20, 32)
    sim.fill_to(g2.size, rng, 4)
    ll = [0] * 286
    for v in (0, 1, 2, 3, 256, 257 + 12, 280, 281, 282, 283, 284, 285):  # twelve codes of lengths 3,3,3,3,4 x 8: complete
        ll[v] = 4
    for v in (0, 1, 2, 3):
        ll[v] = 3
    dl = [4] * 16  # sixteen distance codes of length 4: complete, and equal to the last literal / length lengths
    seq = rle_lengths(ll + dl)
    at = 0
    crosses = False
    for sym, k, v in seq:
        n = 1 if sym < 16 else (v + 3 if sym in (16, 17) else v + 11)
        crosses |= sym == 16 and at < 286 < at + n
        at += n
    assert crosses
    bw = Bits()
    write_block(bw, sim.ops, True, ll, dl)
    add("codes_repeat_across_tables", png_of(31, 8, 8, 0, zwrap(bw.done(), sim.out)))
    # + a single distance code of length 1
    sim = Sim()
    for v in (7, 9, 11):  # three rows of one value each: a literal, then distance 1
        sim.lit(bytes([0, v]))
        sim.match(30, 1)
    ll, _ = dynamic_lens(sim.ops)
    bw = Bits()
    write_block(bw, sim.ops, True, ll, [1])
    add("codes_single_distance", png_of(31, 3, 8, 0, zwrap(bw.done(), sim.out)))
    # ---- matches (+): bytes 0..4 everywhere, so that whatever lands in a filter byte's place is a filter
    sim = Sim()
    sim.fill_to(32768, rng)
    sim.match(258, 32768)
    sim.fill_to(260 * 128, rng)
    bw = Bits()
    write_block(bw, sim.ops, True)
    add("match_distance_32768", png_of(127, 260, 8, 0, zwrap(bw.done(), sim.out)))
    sim = Sim()
    sim.fill_to(65516, rng)
    sim.match(258, 32760)  # source 32756 .. 33014 and destination 65516 .. 65774 both straddle the ring's wrap; 65536 is a flush boundary
    sim.fill_to(515 * 128, rng)
    bw = Bits()
    ll, dl = dynamic_lens(sim.ops)
    write_block(bw, sim.ops, True, ll, dl)
    add("match_straddles_wrap", png_of(127, 515, 8, 0, zwrap(bw.done(), sim.out)))
    # ---- filters: random filtered bytes; every filter at every filter distance and at 1 / 2 / 4 bits
    for bpp, (ct, dp) in {1: (0, 8), 2: (4, 8), 3: (2, 8), 4: (6, 8), 6: (2, 16), 8: (6, 16)}.items():
        f = scanlines(37, 11, dp, ct, rng, filters=[1, 2, 3, 4, 0, 4, 3, 2, 1, 0, 4])
        add("filters_bpp%d" % bpp, png_of(37, 11, dp, ct, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    for dp in (1, 2, 4):
        f = scanlines(37, 11, dp, 0, rng, filters=[4, 3, 2, 1, 0])
        add("filters_grey%d" % dp, png_of(37, 11, dp, 0, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    for ft in (2, 3, 4):
        f = scanlines(5, 3, 8, 2, rng, filters=[ft])
        add("filters_row0_ft%d" % ft, png_of(5, 3, 8, 2, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    f = scanlines(64, 9, 8, 0, rng, filters=[4], hi=3)  # small steps: left = up, up = up-left and all three equal keep happening
    add("filters_paeth_ties", png_of(64, 9, 8, 0, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    for hh in (1, 63, 64, 65, 129):
        ft = rng.integers(0, 5, hh)
        for r, v in ((63, 2), (64, 3), (65, 4), (128, 4)):  # the rows at a band's edge take their values from the row before
            if r < hh:
                ft[r] = v
        f = scanlines(19, hh, 8, 2, rng, filters=ft)
        add("filters_height%d" % hh, png_of(19, hh, 8, 2, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    f = scanlines(1, 65, 8, 2, rng, filters=[4, 3, 2, 1])
    add("filters_width1", png_of(1, 65, 8, 2, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    f = scanlines(301, 203, 8, 2, rng)
    add("filters_random_301x203", png_of(301, 203, 8, 2, zwrap(zdeflate(f.tobytes(), 1), f.tobytes())))
    # ---- colour types and depths
    for ct, dp in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (4, 8), (4, 16), (6, 8), (6, 16)):
        f = scanlines(37, 11, dp, ct, rng)
        add("colour_t%d_d%d" % (ct, dp), png_of(37, 11, dp, ct, zwrap(zdeflate(f.tobytes()), f.tobytes())))
    for dp, npal in ((1, 2), (2, 3), (4, 11), (8, 200), (8, 256)):
        pal = rng.integers(0, 256, npal * 3, dtype=np.uint8).tobytes()
        idx = rng.integers(0, npal, (11, 37))
        bits = ["".join(format(int(t), "0%db" % dp) for t in idx[y]) for y in range(11)]
        bits = [t + "1" * (-len(t) % 8) for t in bits]  # padding bits set: they are no pixels
        f = b"".join(b"\0" + int(t, 2).to_bytes(len(t) // 8, "big") for t in bits)
        add("colour_palette_d%d_n%d" % (dp, npal), png_of(37, 11, dp, 3, zwrap(zdeflate(f), f), extra=chunk(b"PLTE", pal)))
    f = scanlines(37, 11, 8, 3, rng)
    add("colour_palette_filtered", png_of(37, 11, 8, 3, zwrap(zdeflate(f.tobytes()), f.tobytes()), extra=chunk(b"PLTE", rng.integers(0, 256, 768, dtype=np.uint8).tobytes())))
    # ---- resize: 1 x 1, an upscale, the area path, an odd size, the identity
    for ww, hh in ((1, 1), (7, 5), (448, 448), (224, 224)):
        p = photo_raw(ww, hh, ww)
        rgb("resize_%dx%d" % (ww, hh), p, ww, hh)
    # ---- rejects: each also a host failure
    def rej(name, data, message):
        add(name, data, "reject", message)

    z = zwrap(zdeflate(raw), raw)
    rej("reject_truncated", png_of(w, h, 8, 2, z[:len(z) // 2] + z[-4:]), DEFLATE_MSG)
    rej("reject_adler", png_of(w, h, 8, 2, z[:-1] + bytes([z[-1] ^ 1])), ADLER_MSG)
    small = scanlines(9, 4, 8, 0, rng, filters=[0])
    sraw = small.tobytes()
    bw = Bits()
    write_block(bw, [("lit", sraw + b"\x07")], True)
    rej("reject_extra_byte", png_of(9, 4, 8, 0, zwrap(bw.done(), sraw)), DEFLATE_MSG)
    bw = Bits()
    write_block(bw, [("lit", sraw[:3]), ("match", 3, 10), ("lit", sraw[6:])], True)
    rej("reject_distance_before_start", png_of(9, 4, 8, 0, zwrap(bw.done(), sraw)), DEFLATE_MSG)
    ll = [0] * 257
    ll[0] = ll[1] = ll[256] = 1
    bw = Bits()
    write_block(bw, [("lit", b"\0\1")], True, ll, [1])
    rej("reject_oversubscribed", png_of(9, 4, 8, 0, zwrap(bw.done() + bytes(8), sraw)), DEFLATE_MSG)
    ll = [0] * 257
    ll[0] = ll[256] = 2
    bw = Bits()
    write_block(bw, [("lit", bytes(40))], True, ll, [1])
    rej("reject_incomplete_two_codes", png_of(9, 4, 8, 0, zwrap(bw.done() + bytes(8), bytes(40))), DEFLATE_MSG)
    ll = [0] * 257
    ll[0] = ll[1] = 1
    bw = Bits()
    write_block(bw, [("lit", bytes(40))], True, ll, [1])
    rej("reject_no_end_of_block", png_of(9, 4, 8, 0, zwrap(bw.done() + bytes(8), bytes(40))), DEFLATE_MSG)
    bw = Bits()
    write_block(bw, [("lit", sraw[:20]), ("raw", 286, 0, 0), ("lit", sraw[20:])], True)
    rej("reject_symbol_286", png_of(9, 4, 8, 0, zwrap(bw.done(), sraw)), DEFLATE_MSG)
    bw = Bits()
    write_block(bw, [("lit", sraw[:20]), ("raw", 257, 0, 0, 30, 0, 0), ("lit", sraw[23:])], True)
    rej("reject_distance_code_30", png_of(9, 4, 8, 0, zwrap(bw.done(), sraw)), DEFLATE_MSG)
    f5 = small.copy()
    f5[2, 0] = 5
    rej("reject_filter_5", png_of(9, 4, 8, 0, zwrap(zdeflate(f5.tobytes()), f5.tobytes())), FILTER_MSG)
    n = 512
    idx = np.zeros((n, n + 1), np.uint8)
    idx[:, 1:] = rng.integers(0, 16, (n, n))
    idx[unsampled(n), 1 + unsampled(n)] = 16
    rej("reject_palette_index", png_of(n, n, 8, 3, zwrap(zdeflate(idx.tobytes()), idx.tobytes()), extra=chunk(b"PLTE", bytes(range(48)))), PALETTE_MSG)
    # ---- files the GPU route does not take
    add("unqualified_adam7", adam7(13, 9), "unqualified")
    bad = bytearray(png_of(16, 16, 8, 2, zwrap(zdeflate(s.tobytes()), s.tobytes())))
    bad[-20] ^= 1  # inside the IDAT body: its CRC no longer matches
    add("unqualified_bad_crc", bytes(bad), "unqualified", "chunk CRC mismatch")
    assert len({c["name"] for c in out}) == len(out)
    return out


def adam7(w, h):
    """an interlaced RGB image (filter 0 everywhere)"""
    rng = np.random.default_rng(7)
    px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    raw = b""
    for xs, ys, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = px[ys::dy, xs::dx]
        if sub.size:
            raw += b"".join(b"\0" + sub[r].tobytes() for r in range(sub.shape[0]))
    return png_of(w, h, 8, 2, zwrap(zdeflate(raw), raw), interlace=1)


def write_all(directory):
    """cases() written to files: each case gains "path"."""
    cs = cases()
    for c in cs:
        p = directory / (c["name"] + ".png")
        p.write_bytes(c["data"])
        c["path"] = str(p)
    return cs


def idat_stream(data):
    """the concatenated IDAT bodies of a PNG"""
    z, pos = b"", 8
    while pos + 12 <= len(data):
        n = struct.unpack(">I", data[pos:pos + 4])[0]
        if data[pos + 4:pos + 8] == b"IDAT":
            z += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    return z
