"""Host JPEG stage A alone, two builds of the library against each other (no GPU):
    python scratch/stage_a_time.py PARENT.so NEW.so [--rounds 7] [--calls 12] [--out profiles/NAME.txt]

Times icl_jpeg_coefs_file_host(path, 0, NULL, 0, ...) -- stage A plus a page-cached read of the file -- on four files of
tests.jpeg_entropy_cases.corpus (same sizes, seeds and encoder settings) and a 1920x1080 progressive 4:2:0 file made the same way.
The two libraries alternate, round by round; a round's figure for a file is the minimum of its calls.  The margin is the parent's own
spread across its rounds, (max - min) / median per file: the new build's median must not exceed the parent's by more than that.
Exit status 1 when a file misses."""
import argparse
import ctypes as C
import os
import pathlib
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.jpeg_entropy_cases import save_jpeg  # noqa: E402


def files(d):
    return [save_jpeg(d / "q95_444.jpg", 1920, 1080, 104, quality=95, subsampling=0),
            save_jpeg(d / "rst_1080.jpg", 1920, 1080, 212, quality=75, subsampling=2, restart_marker_rows=4),
            save_jpeg(d / "big_4000x3000.jpg", 4000, 3000, 99, quality=75),
            save_jpeg(d / "rst_prog.jpg", 481, 322, 103, quality=75, subsampling=2, progressive=True, restart_marker_blocks=5),
            save_jpeg(d / "prog_1920x1080.jpg", 1920, 1080, 213, quality=75, subsampling=2, progressive=True)]


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.icl_jpeg_coefs_file_host.restype = C.c_int
    lib.icl_jpeg_coefs_file_host.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]
    return lib


def best_ms(lib, path, calls):
    need, info, best = C.c_int64(), (C.c_int32 * 8)(), float("inf")
    for _ in range(calls):
        t0 = time.perf_counter()
        rc = lib.icl_jpeg_coefs_file_host(os.fsencode(path), 0, None, 0, C.byref(need), info)
        best = min(best, time.perf_counter() - t0)
        assert rc == 0 and info[0] == 1 and need.value > 0, (path, rc)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.rounds >= 5 and a.calls >= 10
    libs = {"parent": load(a.parent), "new": load(a.new)}
    with tempfile.TemporaryDirectory() as tmp:
        paths = files(pathlib.Path(tmp))
        ms = {k: {p: [] for p in paths} for k in libs}
        for _ in range(a.rounds):
            for k, lib in libs.items():
                for p in paths:
                    ms[k][p].append(best_ms(lib, p, a.calls))
    lines = ["host stage A, icl_jpeg_coefs_file_host(path, 0, NULL, ...): %d alternating rounds, each the minimum of %d calls; ms" % (a.rounds, a.calls),
             "%-20s %14s %14s %12s %8s  %s" % ("file", "parent median", "parent spread", "new median", "ratio", "")]
    missed = 0
    for p in paths:
        pm, nm = statistics.median(ms["parent"][p]), statistics.median(ms["new"][p])
        spread = (max(ms["parent"][p]) - min(ms["parent"][p])) / pm
        ok = nm <= pm * (1 + spread)
        missed += not ok
        lines.append("%-20s %14.3f %13.1f%% %12.3f %8.3f  %s" % (os.path.basename(p), pm, 100 * spread, nm, nm / pm, "ok" if ok else "MISSES"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
