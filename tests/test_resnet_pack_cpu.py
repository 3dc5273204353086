"""The weight packer, layout by layout: tests/resnet_pack_main.cpp, a stand-alone program (its own main) that includes
imageclust_amd/csrc/resnet_pack.h alone, built with a plain host C++17 compile under -fsanitize=address,undefined and run as a child
process.  It checks every layout rule the model loader and the per-layer entry points share -- the OHWI re-pack, the stem's padded
rows, the stem2 layout with the scale folded in, the BatchNorm fold, row scale and row concatenation, the three storage formats --
element by element against index formulas written out in the program.  No GPU, no Python in the sanitised process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]
RULES = ["ohwi", "ohwi", "stem rows", "stem2", "fold", "row scale + concat", "storage"]
LIMIT_S = 300


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler of the sanitised build"
    exe = str(tmp_path_factory.mktemp("resnet_pack") / "resnet_pack")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + SAN +
                       [os.path.join(HERE, "resnet_pack_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_every_layout_matches_its_index_formula(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=LIMIT_S)  # (the sanitizer runtime is linked in statically)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "ok" and len(lines) == len(RULES) + 1, r.stdout
    assert all(ln.startswith(rule) for ln, rule in zip(lines, RULES)), r.stdout
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
