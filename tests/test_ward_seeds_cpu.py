"""The host rules every clustering call shares (imageclust_amd/csrc/ward_seeds.h): tests/ward_seeds_main.cpp, a stand-alone program
(its own main) that includes the header alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a
child process.  It checks that the final-list walk with null sizes (rows of one item: icl_cluster, icl_cluster_many) equals the walk
with an explicit array of ones and the member lists written out, on random valid logs for m = 0, 1, 2, 3, 17, 64 and min_size = 1, 3;
that a log with an id below 0, an id that does not exist yet, a dead id or one id twice, and a size of 0, are refused with their step
and pair and nothing written; and ward_seed_admit against the rule written out (2^30 items, the first unfrozen seed above max_size,
k_target, CalculateOptimalClusters, the constraint text, the clamp of max_size, the effective sizes, m = 0).  No GPU, no Python in the
sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["null sizes are ones", "bad logs", "admission"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("ward_seeds") / "ward_seeds")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "ward_seeds_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_one_walk_and_one_admission_rule(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
