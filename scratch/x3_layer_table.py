"""Per-layer table of one forward pass of each precision from a rocprofv3 kernel trace (csv) of
    ICL_EMBED_STREAMS=1 rocprofv3 --kernel-trace --stats --output-format csv -- python scratch/embed_prec_rate.py --n 512 --reps 1
(one stream: launch durations do not overlap).  The last pass of each precision is the one after its stem launch
(fp32: stem_pool_kernel<F32, false>, bf16x3: stem_pool_kernel<F32, true>, bf16: stem2_pool_kernel); batch 256.
TF/s is fp32-equivalent work (2 M Cout K per conv): bf16x3 issues three bf16 MFMAs per product."""
import csv
import sys

STEMS = {"fp32": "stem_pool_kernel<F32, false>", "bf16x3": "stem_pool_kernel<F32, true>", "bf16": "stem2_pool_kernel"}


def layers():
    out = [("stem+pool", 256 * 112 * 112, 64, 147)]
    h, cin = 56, 64
    for s, nb in enumerate([3, 4, 6, 3]):
        cout = 256 << s
        mid = cout // 4
        for b in range(nb):
            ho = h // (2 if (b == 0 and s > 0) else 1)
            M = 256 * ho * ho
            out += [("s%d.b%d.c1" % (s + 1, b), M, mid, cin), ("s%d.b%d.c2" % (s + 1, b), M, mid, 9 * mid),
                    ("s%d.b%d.c3%s" % (s + 1, b, "+ds" if b == 0 else ""), M, cout, mid + (cin if b == 0 else 0))]
            cin, h = cout, ho
    return out + [("avgpool", 0, 0, 0)]


def passes(path):
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(path)))
    res = {}
    for prec, stem in STEMS.items():
        idx = [i for i, e in enumerate(ev) if e[2].startswith("void " + stem) or e[2].startswith(stem)]
        if not idx:
            continue
        i0 = idx[-1]
        j = next(j for j in range(i0, len(ev)) if "avgpool" in ev[j][2])
        res[prec] = ev[i0:j + 1]
    return res


def main():
    P = passes(sys.argv[1])
    L = layers()
    for prec in ("fp32", "bf16x3"):
        if prec in P:
            assert len(P[prec]) == len(L), (prec, len(P[prec]))
    print("%-12s %8s %5s %6s | %-44s %9s %7s | %-44s %9s %7s" % ("layer", "M", "Cout", "K", "bf16x3 kernel", "us", "TF/s", "fp32 kernel", "us", "TF/s"))
    tot = {"fp32": 0.0, "bf16x3": 0.0}
    for i, (name, M, co, K) in enumerate(L):
        row = "%-12s %8d %5d %6d" % (name, M, co, K)
        for prec in ("bf16x3", "fp32"):
            s, e, k = P[prec][i]
            us = (e - s) / 1e3
            tot[prec] += us
            tf = 2.0 * M * co * K / us / 1e6 if M else 0.0
            row += " | %-44s %9.1f %7.1f" % (k.replace("void ", "").split("(")[0][:44], us, tf)
        print(row)
    print("sum of launches per batch of 256 (one stream): bf16x3 %.0f us, fp32 %.0f us, ratio %.2f" % (tot["bf16x3"], tot["fp32"], tot["fp32"] / tot["bf16x3"]))
    if "bf16" in P:
        print("bf16 (stage 1 fused, for comparison): %.0f us" % sum((e - s) / 1e3 for s, e, _ in P["bf16"]))


if __name__ == "__main__":
    main()
