"""Which pixels the pruned fused stage-1 bottleneck stores: tests/bneck56_needed_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/prune_map.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child process.
It walks runs of 1 to 4 images in the kernel's 4-row steps with the cursor and the rules bneck56_kernel<false, 2> itself calls (bn56_row,
bn56_step_rows, bn56_quarter_row, bn56_col_needed), for H in 1..9 and 56 and W in {1, 13, 14, 15, 29, 56}, and checks against the triple
loop that exactly the pixels (2 oy, 2 ox) of the run's images are stored, each once.  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
GROUPS = ["walk", "rules"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("bneck56_needed") / "bneck56_needed")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "bneck56_needed_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_the_walk_stores_exactly_the_even_pixels(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(GROUPS) + 1, r.stdout
    assert all(ln.startswith(g) for ln, g in zip(lines, GROUPS)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
