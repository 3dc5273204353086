"""The forward pass's output-pixel map and prune rule: tests/prune_map_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/prune_map.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child
process.  prune_map_pixel -- the function conv_wr_kernel's mapped form calls for its residual loads and stores -- is checked against the
triple loop over (b, oy, ox) for strides 1 to 3, even and odd heights, non-square tensors and pixel counts that are no multiple of the
kernel's 64-pixel tile, and must hit exactly the pixels whose coordinates are multiples of the stride, each once; prune_stride is checked
on ResNet50-v1's records (the last block of stages 1, 2 and 3 and nothing else) and on records that break one of its conditions each.
No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
GROUPS = ["map", "rule", "refused"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("prune_map") / "prune_map")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "prune_map_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_map_equals_the_triple_loop_and_the_rule_reads_the_records(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(GROUPS) + 1, r.stdout
    assert all(ln.startswith(g) for ln, g in zip(lines, GROUPS)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
