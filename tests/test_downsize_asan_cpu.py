"""The host JPEG encoder and downsizer under AddressSanitizer + UBSan: tests/downsize_asan_main.cpp, a stand-alone program (its own main)
linked with jpeg_encode.hip and the host decoders compiled for the host alone, built with -fsanitize=address,undefined and run as a child
process over the sizes of test_jpeg_encode_cpu.py and the sources of test_downsize_cpu.py.  Its outputs must also be the library's own.
No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

from tests.downsize_cases import QUALITIES, SIZES, noise_ppm, sources, truncated_jpeg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "imageclust_amd", "csrc")
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
UNITS = ["jpeg_encode.hip", "image_io.hip", "jpeg_decode.hip", "png_decode.hip"]
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
LIMIT_S = 600


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: the host encoder and decoders are .hip units"
    d = tmp_path_factory.mktemp("downsize_asan")
    objs = []
    for u in UNITS:
        o = str(d / (u[:-4] + ".o"))
        r = subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include")] + SAN +
                           ["-c", os.path.join(CSRC, u), "-o", o], capture_output=True, text=True, timeout=LIMIT_S)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(o)
    exe = str(d / "downsize_asan")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17"] + SAN + ["-static-libsan", "-x", "c++", os.path.join(HERE, "downsize_asan_main.cpp"),
                        "-x", "none"] + objs + ["-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def clean(r):
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]


def test_encoder_over_every_size_and_quality(program):
    for w, h in SIZES:
        for q in QUALITIES:
            for seed in (1, 2):  # odd: noise, even: a gradient
                r = subprocess.run([program, "encode", str(w), str(h), str(q), str(seed)], capture_output=True, text=True, timeout=LIMIT_S)
                clean(r)
                assert r.stdout.startswith("encode %dx%d q%d: " % (w, h, q)), r.stdout


def test_downsizer_over_the_sources(program, tmp_path):
    from imageclust_amd import _lib as L

    files = dict(sources(), trunc=truncated_jpeg(), noise=noise_ppm(200, 200), thin=noise_ppm(4000, 1), text=b"not an image " * 40)
    paths = []
    for name, data in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    paths.append(str(tmp_path / "missing.jpg"))
    for max_bytes, max_dim in ((20000, 96), (5000, 64), (2000, 96), (100, 2**31 - 1)):  # (the last: the size rule at the edge of int)
        r = subprocess.run([program, "downsize", str(max_bytes), str(max_dim)] + paths, capture_output=True, text=True, timeout=LIMIT_S)
        clean(r)
        lines = r.stdout.strip().split("\n")
        assert lines[-1] == "ok" and len(lines) == len(paths) + 1, r.stdout
        for line, (name, data) in zip(lines, files.items()):  # the sanitised build computes what the library computes
            try:
                want = "rc 0, %d bytes" % len(L.downsize_image_mem(data, max_bytes, max_dim))
            except L.ICLError as e:
                want = "rc %d, 0 bytes" % e.code
            assert want in line, (name, line, want)
        assert "rc %d" % L.ICL_ERR_IO in lines[len(files)]
