"""Every convolution launch of ONE forward pass (the second batch of a rocprofv3 --kernel-trace csv, as scratch/layer_report.py picks it),
in launch order with its layer's name: layer_launches.py trace.csv [trace2.csv ...].  layer_report.py sums the launches of one shape; this
lists them one by one, which is what a change to single blocks (the pruned last block of a stage) needs.  With several traces the
durations stand side by side (the launch sequence must be the same)."""
import csv
import re
import sys


def batch_of(path):
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Grid_Size_X", r.get("Grid_Size", ""))) for r in csv.DictReader(open(path)))
    idx = [i for i, e in enumerate(ev) if "stem" in e[2][:40]]
    return ev[idx[1]:idx[2]]


def names():
    out = ["stem"]
    for s, nb in enumerate([3, 4, 6, 3]):
        for b in range(nb):
            out += ["s%d.b%d" % (s + 1, b)] if s == 0 else ["s%d.b%d.%s" % (s + 1, b, c) for c in ("c1", "c2", "c3")]
    return out


def short(n):
    m = re.match(r"(?:void )?(\w+)(<[^>]*>)?", n)
    return (m.group(1) + (m.group(2) or "")) if m else n[:40]


def main():
    batches = [batch_of(p) for p in sys.argv[1:]]
    convs = [[e for e in b if re.search(r"stem|bneck56|conv_igemm|conv3x3_halo|conv_p8|conv_wr", e[2])] for b in batches]
    assert len({len(c) for c in convs}) == 1, [len(c) for c in convs]
    for i, name in enumerate(names()[:len(convs[0])]):
        us = ["%8.1f" % ((c[i][1] - c[i][0]) / 1e3) for c in convs]
        print("%-9s %s us  grid %-8s %s" % (name, " ".join(us), convs[-1][i][3], short(convs[-1][i][2])))
    for p, b in zip(sys.argv[1:], batches):
        print("batch span %.1f us  (%s)" % ((b[-1][1] - b[0][0]) / 1e3, p))


if __name__ == "__main__":
    main()
