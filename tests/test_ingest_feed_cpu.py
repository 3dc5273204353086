"""ingest_feed.h (the ordered, bounded feed between the file workers and the slab builder of jpeg_gpu.hip) without a GPU:
tests/ingest_feed_main.cpp, a stand-alone program over the header alone, built with the host C++ compiler and run as a child process
under AddressSanitizer + UBSan and under ThreadSanitizer.  Order, admission window, the item larger than the byte budget, a consumer
that leaves early, a worker without memory, n = 1 and n = 0, each on 1, 4 and 16 threads."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "imageclust_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
LIMIT_S = 60  # a deadlock is a failure, not a stall
# the runtimes are linked statically: as shared libraries they refuse to start wherever the environment preloads another library
IS_CLANG = CXX is not None and "clang" in subprocess.run([CXX, "--version"], capture_output=True, text=True).stdout
STATIC = {"address,undefined": ["-static-libasan", "-static-libubsan"], "thread": ["-static-libtsan"]}


def build(out, src, sanitize):
    assert CXX is not None, "no host C++ compiler"
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all",
           "-I", CSRC, str(src), "-o", str(out)] + (["-static-libsan"] if IS_CLANG else STATIC[sanitize])
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


def run_program(tmp_path, sanitize):
    exe = tmp_path / ("feed_" + sanitize.split(",")[0])
    b = build(exe, os.path.join(HERE, "ingest_feed_main.cpp"), sanitize)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, "exit %d\n%s\n%s" % (r.returncode, r.stdout, r.stderr)
    assert r.stdout.split("\n")[:3] == ["threads %d: ok" % t for t in (1, 4, 16)], r.stdout


def test_header_is_host_only():
    text = open(os.path.join(CSRC, "ingest_feed.h")).read()
    includes = [ln.split()[1] for ln in text.split("\n") if ln.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_feed_under_asan_ubsan(tmp_path):
    run_program(tmp_path, "address,undefined")


def test_feed_under_tsan(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    b = build(tmp_path / "probe", probe, "thread")
    started = b.returncode == 0 and subprocess.run([str(tmp_path / "probe")], capture_output=True, timeout=LIMIT_S).returncode == 0
    if not started:
        pytest.skip("a one-line program built with -fsanitize=thread does not start here (old TSan runtimes refuse some kernels' "
                    "address-space layouts): " + (b.stderr.strip() or "it exits non-zero")[-300:])
    run_program(tmp_path, "thread")
