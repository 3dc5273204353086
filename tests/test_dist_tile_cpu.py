"""The distance kernels' tile decode and tile count: tests/dist_tile_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/dist_tile.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child
process.  It checks that the band decode maps a launch's ids one to one onto its tiles -- tile rows starting at 0, 1, 7, 8, 9, 13 and
100, 1 to 41 rows each, then (0, 782), (0, 1954) and (500, 782) --, that the last ids of the largest launch a grid can hold decode into
range, that the host count is the number of tiles and refuses what no grid holds, and that the order of (0, 10) and (3, 12) is the
recorded one.  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["small launches", "large launches", "grid limit", "tile order"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("dist_tile") / "dist_tile")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "dist_tile_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_band_decode_is_a_bijection_in_the_recorded_order(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
