"""The band walk's column-split decision: tests/band_plan_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/band_plan.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child
process.  It checks band_splits, the pure function behind icl_nearest's and icl_cluster_fit's split count, for 1 to 600 bands, 0 to
2000 column tiles and devices of 1 and 256 CUs: a forced count f gives min(f, max(1, min(tiles, 1024))), the automatic one is 1 from
2 x CUs bands on and max(1, min(2 x CUs / bands, cap)) below, and every result lies in [1, max(1, tiles)].  No GPU, no Python in the
sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["forced", "auto", "range"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("band_plan") / "band_plan")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "band_plan_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_split_count_forced_automatic_and_in_range(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
