"""Files for the entropy-decoder tests (test_jpeg_entropy_cpu.py, test_ingest_entropy_gpu.py): the corpus of test_ingest_files_gpu.py
plus optimised Huffman tables, and a seeded set of damaged files."""
import numpy as np
from PIL import Image, ImageFile

ImageFile.MAXBLOCK = 1 << 26  # Pillow's progressive / optimising encoder needs the whole file in one buffer


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 100 * np.sin(x / (7 + 13 * c) + y / (11 + 5 * c) + c) for c in range(3)], -1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def save_jpeg(path, w, h, seed, **kw):
    im = Image.fromarray(picture(w, h, seed))
    if kw.pop("grey", False):
        im = im.convert("L")
    im.save(str(path), "JPEG", **kw)
    return str(path)


def is_progressive(path):
    return Image.open(path).info.get("progressive", 0) == 1


def corpus(d, big=True):
    """-> paths; the qualifying ones are exactly those that are not progressive."""
    paths = []
    seed = 0
    for w, h in [(1, 1), (8, 8), (17, 9), (37, 53), (224, 224), (448, 448), (481, 322), (1920, 1080)]:
        for sub in (0, 1, 2):  # 4:4:4, 4:2:2, 4:2:0
            seed += 1
            paths.append(save_jpeg(d / ("b%d_%dx%d_s%d.jpg" % (seed, w, h, sub)), w, h, seed, quality=80, subsampling=sub))
        seed += 1
        paths.append(save_jpeg(d / ("p%d_%dx%d.jpg" % (seed, w, h)), w, h, seed, quality=75, subsampling=2, progressive=True))
        seed += 1
        paths.append(save_jpeg(d / ("g%d_%dx%d.jpg" % (seed, w, h)), w, h, seed, quality=85, grey=True))
    if big:
        paths.append(save_jpeg(d / "big_4000x3000.jpg", 4000, 3000, 99, quality=75))
    paths.append(save_jpeg(d / "pg_481x322.jpg", 481, 322, 100, quality=70, progressive=True, grey=True))
    paths.append(save_jpeg(d / "rst_blocks.jpg", 481, 322, 101, quality=75, subsampling=2, restart_marker_blocks=3))
    paths.append(save_jpeg(d / "rst_rows.jpg", 37, 53, 102, quality=75, subsampling=1, restart_marker_rows=1))
    paths.append(save_jpeg(d / "rst_prog.jpg", 481, 322, 103, quality=75, subsampling=2, progressive=True, restart_marker_blocks=5))
    paths.append(save_jpeg(d / "q95_444.jpg", 1920, 1080, 104, quality=95, subsampling=0))
    try:  # RGB components without colour transform (Adobe transform 0), where this Pillow can write one
        paths.append(save_jpeg(d / "keep_rgb.jpg", 481, 322, 105, quality=90, keep_rgb=True))
    except (TypeError, ValueError, OSError):
        pass
        pass
    try:
        if big:  # components that share one table pair, far more than ICL_JE_LAUNCHES workgroups of stream
            paths.append(save_jpeg(d / "keep_rgb_1920x1080.jpg", 1920, 1080, 106, quality=90, keep_rgb=True))
    except (TypeError, ValueError, OSError):
        pass
    for orient in range(1, 9):
        for (w, h), sub in (((37, 53), 2), ((481, 322), 1), ((448, 448), 0)):
            exif = Image.Exif()
            exif[0x0112] = orient
            seed += 1
            paths.append(save_jpeg(d / ("o%d_%dx%d.jpg" % (orient, w, h)), w, h, seed, quality=85, subsampling=sub, exif=exif.tobytes()))
    # per-file Huffman tables (codes longer than the 9-bit lookahead), with and without restart intervals
    for k, ((w, h), sub, q) in enumerate((((481, 322), 2, 70), ((1920, 1080), 0, 95), ((448, 448), 1, 85), ((37, 53), 2, 90))):
        paths.append(save_jpeg(d / ("opt%d_%dx%d.jpg" % (k, w, h)), w, h, 200 + k, quality=q, subsampling=sub, optimize=True))
    paths.append(save_jpeg(d / "opt_grey.jpg", 481, 322, 210, quality=80, grey=True, optimize=True))
    paths.append(save_jpeg(d / "opt_rst.jpg", 481, 322, 211, quality=80, subsampling=2, optimize=True, restart_marker_rows=2))
    paths.append(save_jpeg(d / "rst_1080.jpg", 1920, 1080, 212, quality=75, subsampling=2, restart_marker_rows=4))
    return paths


def _scan_extent(data):
    """(first byte of the entropy-coded segment, position of the marker that ends it) of a single-scan file"""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + ((data[pos + 2] << 8) | data[pos + 3])
    a = pos + 2 + ((data[pos + 2] << 8) | data[pos + 3])
    b = a
    while not (data[b] == 0xFF and data[b + 1] != 0 and not 0xD0 <= data[b + 1] <= 0xD7):
        b += 1
    return a, b


def damaged(d, seed=20250917):
    """A seeded set of damaged baseline files -> paths."""
    rng = np.random.default_rng(seed)
    out = []

    def put(name, data):
        p = d / name
        p.write_bytes(bytes(data))
        out.append(str(p))

    plain = open(save_jpeg(d / "src_plain.jpg", 300, 200, 300, quality=85, subsampling=2), "rb").read()
    rst = open(save_jpeg(d / "src_rst.jpg", 300, 200, 301, quality=85, subsampling=1, restart_marker_blocks=4), "rb").read()
    opt = open(save_jpeg(d / "src_opt.jpg", 300, 200, 302, quality=85, subsampling=0, optimize=True), "rb").read()
    for name, src in (("plain", plain), ("rst", rst), ("opt", opt)):
        a, b = _scan_extent(src)
        for k in range(6):  # byte flips inside the entropy-coded segment
            x = bytearray(src)
            at = int(rng.integers(a, b))
            x[at] ^= int(rng.integers(1, 256))
            put("flip_%s_%d.jpg" % (name, k), x)
        for k, frac in enumerate((0.1, 0.5, 0.9, 0.999)):  # truncation
            put("trunc_%s_%d.jpg" % (name, k), src[: a + int((b - a) * frac)])
        x = bytearray(src)  # an inserted FF FF
        at = int(rng.integers(a, b))
        x[at:at] = b"\xff\xff"
        put("ffff_%s.jpg" % name, x)
    a, b = _scan_extent(rst)
    marks = [i for i in range(a, b - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7]
    m = marks[len(marks) // 2]
    put("rst_removed.jpg", rst[:m] + rst[m + 2:])
    put("rst_duplicated.jpg", rst[:m] + rst[m:m + 2] + rst[m:])
    put("rst_fill_byte.jpg", rst[:m] + b"\xff" + rst[m:])
    # a DHT with unused codes: one more symbol appended to the longest code length of the first table (the stream never uses it)
    x = bytearray(plain)
    pos = 2
    while x[pos + 1] != 0xC4:
        pos += 2 + ((x[pos + 2] << 8) | x[pos + 3])
    seg = (x[pos + 2] << 8) | x[pos + 3]
    bits = x[pos + 5:pos + 21]
    nvals = sum(bits)
    longest = max(i for i in range(16) if bits[i])
    if seg == 2 + 17 + nvals:  # one table per DHT segment (what Pillow writes)
        x[pos + 5 + longest] += 1
        x[pos + 21 + nvals:pos + 21 + nvals] = bytes([0x0B if x[pos + 4] < 16 else 0xFA])
        seg += 1
        x[pos + 2], x[pos + 3] = seg >> 8, seg & 255
        put("dht_unused.jpg", x)
    return out


if __name__ == "__main__":  # python -m tests.jpeg_entropy_cases DIR: the damaged set for scratch/asan_jpeg/run.sh DIR
    import pathlib
    import sys

    out_dir = pathlib.Path(sys.argv[1])
    out_dir.mkdir(parents=True, exist_ok=True)
    print("%d files in %s" % (len(damaged(out_dir)), out_dir))
