"""The bump layout of the grow-only workspaces: tests/ws_layout_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/icl_ws_layout.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child
process.  It checks for the alignments 16 and 256 that take() returns aligned offsets, each advancing by the size rounded up, that a
piece of 0 bytes takes no room, and that the offsets and totals of three small shapes -- icl_pairs_within with n = 129, icl_nearest
with nq = 130, n = 257, k = 64 and two splits, icl_cluster_requests with 3 rows, head = 1000 and 5 labels -- are the ones the units'
earlier hand-written expressions gave (literals in the program).  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["steps", "shapes"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("ws_layout") / "ws_layout")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "ws_layout_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_layout_offsets_and_totals(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
