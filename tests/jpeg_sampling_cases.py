"""JPEG files at the chroma layouts Pillow's encoder cannot write -- 4:4:0 (luma 1x2) and 4:1:1 (luma 4x1, or 1x4 after a lossless
rotation) -- for test_jpeg_sampling_cpu.py and test_jpeg_sampling_gpu.py.

A JPEG's entropy-coded stream does not encode the frame geometry: rewriting the luma sampling byte of the SOF segment (and width and
height) gives a valid file of another layout as long as the blocks per MCU and the number of MCUs stay what the stream holds.  A 2x1
file (4 blocks per MCU) becomes 1x2, a 2x2 file (6 blocks per MCU) becomes 4x1 or 1x4.  The picture comes out scrambled, which does
not matter: Pillow's (libjpeg-turbo's) decode of the same bytes is the reference.  Progressive files keep their size, a multiple of
32 both ways: their non-interleaved scans count blocks per component, and only then do those counts still match."""
import warnings

import numpy as np
from PIL import Image, ImageFile

from tests.jpeg_entropy_cases import _scan_extent, picture

ImageFile.MAXBLOCK = 1 << 26  # Pillow's progressive / optimising encoder needs the whole file in one buffer

SOURCE_OF = {(1, 2): (2, 1), (4, 1): (2, 2), (1, 4): (2, 2)}  # new luma sampling -> the sampling Pillow writes with as many blocks per MCU
PILLOW_SUB = {(2, 1): 1, (2, 2): 2}


def sof_offset(data):
    """Index of the frame header's FF Cx, found by walking the marker segments (an EXIF payload may contain FF C0)."""
    pos = 2
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF, "lost the marker chain at %d" % pos
        m = data[pos + 1]
        if m in (0xC0, 0xC1, 0xC2):
            return pos
        assert m != 0xDA, "scan before frame header"
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    raise AssertionError("no frame header")


def frame(data):
    """(W, H, [(h, v) per component]) of the frame header."""
    i = sof_offset(data)
    n = data[i + 9]
    return (data[i + 7] << 8) | data[i + 8], (data[i + 5] << 8) | data[i + 6], [(data[i + 11 + 3 * c] >> 4, data[i + 11 + 3 * c] & 15) for c in range(n)]


def mcus(w, h, hs, vs):
    return -(-w // (8 * hs)) * -(-h // (8 * vs))


def rewrite(data, luma=None, size=None, chroma=None):
    """data with the luma component's sampling byte (luma=(hs, vs)), the size (size=(W, H)) and / or the first chroma component's sampling
    byte (chroma=(h, v)) of the frame header replaced."""
    x = bytearray(data)
    i = sof_offset(x)
    assert x[i + 9] == 3
    if size is not None:
        w, h = size
        x[i + 5], x[i + 6], x[i + 7], x[i + 8] = h >> 8, h & 255, w >> 8, w & 255
    if luma is not None:
        x[i + 11] = (luma[0] << 4) | luma[1]
    if chroma is not None:
        x[i + 14] = (chroma[0] << 4) | chroma[1]
    return bytes(x)


def pillow_rgb(path, transposed=False):
    """Pillow's pixels of a file, every decoder warning an error (a stream that does not fill the new geometry warns); transposed=True
    applies the EXIF orientation as cv::imread does."""
    from PIL import ImageOps

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(path)
        im.load()
        if transposed:
            im = ImageOps.exif_transpose(im)
        return np.asarray(im.convert("RGB"))


def make(d, name, luma, src_size, size=None, seed=0, orient=0, **kw):
    """One file of luma sampling `luma` at `size` (default: the source's), rewritten from a Pillow file of src_size -> a case dict."""
    src = SOURCE_OF[luma]
    sw, sh = src_size
    w, h = size or src_size
    assert mcus(w, h, *luma) == mcus(sw, sh, *src), (name, "the MCU count must stay the stream's")
    if kw.get("progressive"):
        assert (w, h) == (sw, sh) and w % 32 == 0 and h % 32 == 0, name
    if orient:
        exif = Image.Exif()
        exif[0x0112] = orient
        kw["exif"] = exif.tobytes()
    kw.setdefault("quality", 85)
    p = d / name
    Image.fromarray(picture(sw, sh, seed)).save(str(p), "JPEG", subsampling=PILLOW_SUB[src], **kw)
    data = open(p, "rb").read()
    assert frame(data) == (sw, sh, [src, (1, 1), (1, 1)]), (name, frame(data))
    p.write_bytes(rewrite(data, luma, (w, h)))
    case = dict(path=str(p), luma=luma, size=(w, h), progressive=bool(kw.get("progressive")), orient=orient or 1)
    pillow_rgb(case["path"])  # the reference reads it without a warning
    return case


def corpus(d):
    """Every clean fixture -> list of case dicts (path, luma, size, progressive, orient)."""
    out = []
    seed = [400]

    def add(name, luma, src_size, size=None, **kw):
        seed[0] += 1
        out.append(make(d, name, luma, src_size, size, seed=seed[0], **kw))

    # one MCU: chroma planes 1, 2 and 3 samples wide or tall, where edge rules go wrong
    for w, h in ((1, 1), (2, 2), (3, 16), (8, 9)):
        add("v2_%dx%d.jpg" % (w, h), (1, 2), (16, 8), (w, h))
    for w, h in ((5, 8), (1, 1), (9, 3), (32, 8)):
        add("h4_%dx%d.jpg" % (w, h), (4, 1), (16, 16), (w, h))
    for w, h in ((8, 5), (3, 9), (1, 1)):
        add("v4_%dx%d.jpg" % (w, h), (1, 4), (16, 16), (w, h))
    # several MCUs, odd sizes; Huffman tables of the file's own; restart intervals in blocks and in rows; orientations that swap the axes
    variants = [("", {}), ("_opt", dict(optimize=True)), ("_rstb", dict(restart_marker_blocks=3)), ("_rstr", dict(restart_marker_rows=1))]
    variants += [("_o%d" % o, dict(orient=o)) for o in (5, 6, 8)]
    for tag, kw in variants:
        add("v2_41x50%s.jpg" % tag, (1, 2), (64, 48), (41, 50), **kw)
        add("h4_45x59%s.jpg" % tag, (4, 1), (64, 64), (45, 59), **kw)
    add("v4_59x45.jpg", (1, 4), (64, 64), (59, 45))
    add("v4_59x45_rstb.jpg", (1, 4), (64, 64), (59, 45), restart_marker_blocks=3)
    add("v4_59x45_o6.jpg", (1, 4), (64, 64), (59, 45), orient=6)
    # progressive: one scan per component for the AC bands, each with its own block extent
    add("h4_prog_96x64.jpg", (4, 1), (96, 64), progressive=True)
    add("v4_prog_96x64.jpg", (1, 4), (96, 64), progressive=True)
    add("v2_prog_64x96.jpg", (1, 2), (64, 96), progressive=True)
    # streams of a few hundred 1024-bit subsequences (more than one workgroup of the GPU entropy decoder), with and without restarts
    add("v2_317x473.jpg", (1, 2), (480, 320), (317, 473), quality=90)
    add("h4_470x315.jpg", (4, 1), (480, 320), (470, 315), quality=90)
    add("v4_315x470.jpg", (1, 4), (480, 320), (315, 470), quality=90)
    add("h4_470x315_rstr.jpg", (4, 1), (480, 320), (470, 315), quality=90, restart_marker_rows=2)
    return out


def blocks_of(case):
    """Blocks of the three components as the frame geometry implies them (padded to whole MCUs)."""
    (w, h), (hs, vs) = case["size"], case["luma"]
    m = mcus(w, h, hs, vs)
    return [m * hs * vs, m, m]


def damaged(d, cases):
    """Four damaged files from the 317x473 1x2 and the 470x315 4x1 file: each cut at half its scan, each with one byte flipped inside it."""
    rng = np.random.default_rng(20251018)
    out = []
    for key in ("v2_317x473.jpg", "h4_470x315.jpg"):
        src = open([c["path"] for c in cases if c["path"].endswith(key)][0], "rb").read()
        a, b = _scan_extent(src)
        p = d / ("trunc_" + key)
        p.write_bytes(src[: a + (b - a) // 2])
        out.append(str(p))
        x = bytearray(src)
        x[int(rng.integers(a, b))] ^= int(rng.integers(1, 256))
        p = d / ("flip_" + key)
        p.write_bytes(bytes(x))
        out.append(str(p))
    return out


def rejected(d):
    """Files whose sampling stays undecoded -> [(path, the sampling as the message names it)]: a 2x2 file with the luma byte rewritten to
    4x2, 2x4, 3x1 or 4x4, and one with the first chroma component at 2x1."""
    p = d / "src_2x2.jpg"
    Image.fromarray(picture(64, 64, 499)).save(str(p), "JPEG", quality=85, subsampling=2)
    data = open(p, "rb").read()
    out = []
    for hs, vs in ((4, 2), (2, 4), (3, 1), (4, 4)):
        q = d / ("luma_%dx%d.jpg" % (hs, vs))
        q.write_bytes(rewrite(data, (hs, vs)))
        out.append((str(q), "%dx%d,1x1,1x1" % (hs, vs)))
    q = d / "chroma_2x1.jpg"
    q.write_bytes(rewrite(data, chroma=(2, 1)))
    out.append((str(q), "2x2,2x1,1x1"))
    return out
