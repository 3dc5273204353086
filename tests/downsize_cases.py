"""Inputs of the JPEG encoder and downsizer tests (test_jpeg_encode_*.py, test_downsize_*.py): the image contents the encoder is pinned
on, Pillow as its reference, and the source files of the downsizer with what resizeImageIfNeeded must make of them."""
import io
import warnings

import numpy as np
from PIL import Image, ImageFile, ImageOps

from tests.jpeg_entropy_cases import picture

ImageFile.MAXBLOCK = 1 << 26  # Pillow's progressive encoder needs the whole file in one buffer

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (37, 53), (64, 48), (250, 131)]  # (w, h)
QUALITIES = [95, 75, 50, 30, 100, 1]
CONTENTS = ["noise", "flat", "gradient", "checker", "sparse_hf", "primaries"]


def content(kind, w, h, seed=0):
    """h x w x 3 u8 RGB."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":  # long codes, and 0xFF bytes in the stream
        return np.random.default_rng(1000 + seed + 7 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":  # EOB only
        return np.full((h, w, 3), (200, 30, 90), np.uint8)
    if kind == "gradient":
        return np.stack([x * 255 // max(1, w - 1), y * 255 // max(1, h - 1), (x + y) * 255 // max(1, w + h - 2)], -1).astype(np.uint8)
    if kind == "checker":  # 0 / 255 per pixel and per 8 x 8 block: the largest DC differences and amplitudes
        return np.repeat(((((x + y) & 1) ^ (((x >> 3) + (y >> 3)) & 1)) * 255).astype(np.uint8)[..., None], 3, -1)
    if kind == "sparse_hf":  # grey blocks of the highest-frequency basis function alone: DC, 62 zeros, one coefficient -> ZRL runs
        c = np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
        return np.repeat(np.clip(128 + 110 * c, 0, 255).astype(np.uint8)[..., None], 3, -1)
    if kind == "primaries":  # the Cb / Cr extremes
        cols = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 255, 255), (255, 0, 255), (255, 255, 0), (0, 0, 0), (255, 255, 255)], np.uint8)
        return cols[((x // 3) + (y // 5)) % 8]
    raise ValueError(kind)


def pillow_jpeg(rgb, quality):
    """The reference: Pillow (libjpeg-turbo) with nothing but the quality set."""
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality)
    return b.getvalue()


def pillow_pixels(data, transposed=True):
    """Pillow's RGB pixels of an encoded image, every decoder warning an error; the EXIF orientation applied as cv::imread does."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
        if transposed:
            im = ImageOps.exif_transpose(im)
        return np.ascontiguousarray(np.asarray(im.convert("RGB")))


def scan_of(jpeg):
    """The entropy-coded segment of a single-scan file (between the SOS header and EOI)."""
    i = jpeg.index(b"\xff\xda")
    return jpeg[i + 2 + ((jpeg[i + 2] << 8) | jpeg[i + 3]):-2]


def new_size(R, C, max_dim):
    """resizeImageIfNeeded's size rule in Python floats (= Go's float64): rows R, columns C -> (newW, newH)."""
    ratio = float(C) / float(R)
    if R > C:
        return max_dim, int(max_dim * ratio)
    return int(max_dim / ratio), max_dim


def expected_downsize(L, data, max_bytes, max_dim):
    """What resizeImageIfNeeded returns for `data`, from Pillow's decoder and encoder and the pinned resize -> (bytes, attempts)."""
    if len(data) <= max_bytes:
        return data, 0
    px = pillow_pixels(data)
    nw, nh = new_size(px.shape[0], px.shape[1], max_dim)
    out = pillow_jpeg(L.resize_u8(px, nw, nh), 95)
    if len(out) > max_bytes and nw // 2 >= 1 and nh // 2 >= 1:
        return pillow_jpeg(L.resize_u8(px, nw // 2, nh // 2), 95), 2
    return out, 1


def _save(rgb, fmt, **kw):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, fmt, **kw)
    return b.getvalue()


def ppm_bytes(rgb):
    return b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]) + rgb.tobytes()


def sources():
    """name -> encoded bytes, every one above 20 000 bytes: the formats and layouts the downsizer must take."""
    pic = picture(400, 300, 31)
    tall = picture(300, 400, 32)
    exif = Image.Exif()
    exif[0x0112] = 6
    rgba = np.dstack([picture(200, 150, 33), np.random.default_rng(5).integers(0, 256, (150, 200), dtype=np.uint8)])
    b = io.BytesIO()
    Image.fromarray(rgba, "RGBA").save(b, "PNG")
    return {
        "jpeg_420": _save(pic, "JPEG", quality=92, subsampling=2),
        "jpeg_444": _save(tall, "JPEG", quality=92, subsampling=0),
        "jpeg_422": _save(pic, "JPEG", quality=92, subsampling=1),
        "jpeg_gray": _save(np.ascontiguousarray(picture(500, 380, 34)[..., 0]), "JPEG", quality=95),
        "jpeg_progressive": _save(tall, "JPEG", quality=92, progressive=True),
        "jpeg_orient6": _save(pic, "JPEG", quality=92, exif=exif.tobytes()),
        "png_alpha": b.getvalue(),
        "ppm": ppm_bytes(picture(160, 120, 35)),
    }


def noise_ppm(w, h, seed=0):
    return ppm_bytes(content("noise", w, h, seed))


def truncated_jpeg():
    """A JPEG the decoders reject that is still above 20 000 bytes: a 30 000-byte ICC segment in front, cut where the scan would begin."""
    data = _save(picture(120, 90, 36), "JPEG", quality=90, icc_profile=bytes(30000))
    return data[: data.index(b"\xff\xda")]
