"""A memory source is never read past its last byte: tests/ingest_mem_main.cpp, a stand-alone program (its own main) linked with the host
decoders -- image_io.hip, jpeg_decode.hip and png_decode.hip compiled for the host alone -- built with -fsanitize=address,undefined and
run as a child process.  Every prefix length 0 .. len of a baseline 4:2:0 JPEG, a progressive JPEG, a 4:1:1 JPEG and a PNG, each in a
heap allocation of exactly that size, and 200 single-byte mutations of each, go through icl_decode_image_mem.  No GPU, no Python in the
sanitised process."""
import os
import shutil
import subprocess

import pytest
from PIL import Image

from tests import jpeg_sampling_cases
from tests.jpeg_entropy_cases import picture, save_jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "imageclust_amd", "csrc")
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
UNITS = ["image_io.hip", "jpeg_decode.hip", "png_decode.hip"]
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
LIMIT_S = 600


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: the host decoders are .hip units"
    d = tmp_path_factory.mktemp("mem_asan")
    objs = []
    for u in UNITS:
        o = str(d / (u[:-4] + ".o"))
        r = subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include")] + SAN +
                           ["-c", os.path.join(CSRC, u), "-o", o], capture_output=True, text=True, timeout=LIMIT_S)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(o)
    exe = str(d / "ingest_mem")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17"] + SAN + ["-static-libsan", "-x", "c++", os.path.join(HERE, "ingest_mem_main.cpp"),
                        "-x", "none"] + objs + ["-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = tmp_path_factory.mktemp("mem_asan_img")
    out = [save_jpeg(d / "base420.jpg", 64, 48, 1, quality=80, subsampling=2),
           save_jpeg(d / "prog.jpg", 64, 48, 2, quality=80, subsampling=2, progressive=True),
           jpeg_sampling_cases.make(d, "h4_45x59.jpg", (4, 1), (64, 64), (45, 59), seed=3)["path"]]
    Image.fromarray(picture(64, 48, 4)).save(str(d / "rgb.png"))
    out.append(str(d / "rgb.png"))
    assert jpeg_sampling_cases.frame(open(out[0], "rb").read())[2][0] == (2, 2) and jpeg_sampling_cases.frame(open(out[2], "rb").read())[2][0] == (4, 1)
    assert all(os.path.getsize(p) < 16384 for p in out), "keep the prefix sweep short"
    return out


def test_prefixes_and_mutations_stay_inside_the_buffer(program, images):
    r = subprocess.run([program] + images, capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(images) + 1, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_ppm_reader_from_memory(program, tmp_path):
    """The one decoder that read its file as it went: from memory its tokens, comment and pixel data stay inside the buffer too."""
    p = tmp_path / "tiny.ppm"
    p.write_bytes(b"P6\n# c\n5 3\n255\n" + picture(5, 3, 5).tobytes())
    r = subprocess.run([program, str(p)], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
