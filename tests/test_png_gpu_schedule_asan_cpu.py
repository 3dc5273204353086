"""The GPU PNG route's schedule never leaves its buffers: tests/png_inflate_main.cpp, a stand-alone program (its own main) linked with the
host decoders -- image_io.hip, jpeg_decode.hip and png_decode.hip compiled for the host alone -- built with -fsanitize=address,undefined
and run as a child process.  The whole corpus of tests/png_gpu_cases.py goes through the host loop at every stage, each file in a heap
allocation of exactly its size; three small files are swept: every prefix of the file and of its zlib stream, and 200 single-byte
mutations with the CRCs recomputed, so that hostile streams reach the inflate loop.  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

from tests import png_gpu_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "imageclust_amd", "csrc")
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
UNITS = ["image_io.hip", "jpeg_decode.hip", "png_decode.hip"]
SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
SWEPT = ["codes_single_distance", "codes_repeat_across_tables", "filters_row0_ft4"]  # dynamic codes by hand, a match, zlib's own output
LIMIT_S = 900


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: the host decoders are .hip units"
    d = tmp_path_factory.mktemp("png_asan")
    objs = []
    for u in UNITS:
        o = str(d / (u[:-4] + ".o"))
        r = subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include")] + SAN +
                           ["-c", os.path.join(CSRC, u), "-o", o], capture_output=True, text=True, timeout=LIMIT_S)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(o)
    exe = str(d / "png_inflate")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17"] + SAN + ["-static-libsan", "-x", "c++", os.path.join(HERE, "png_inflate_main.cpp"),
                        "-x", "none"] + objs + ["-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_corpus_prefixes_and_mutations_stay_inside_the_buffers(program, tmp_path):
    cs = png_gpu_cases.write_all(tmp_path)
    by = {c["name"]: c for c in cs}
    swept = [by[n]["path"] for n in SWEPT]
    assert all(os.path.getsize(p) < 1024 for p in swept), "keep the sweeps short"
    rest = [c["path"] for c in cs if c["name"] not in SWEPT]
    r = subprocess.run([program, str(len(swept))] + swept + rest, capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(cs) + 2, r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    states = {os.path.basename(l.split(":")[0])[:-4]: int(l.rsplit(" ", 1)[1]) for l in lines if ": state " in l}
    for c in cs:
        if c["name"] not in SWEPT:
            assert states[c["name"]] == {"clean": 1, "reject": 0, "unqualified": -1}[c["kind"]], c["name"]
