#!/usr/bin/env python3
"""Weight packing of two builds of the library compared on what it feeds: pack_parity.py PARENT_SO [BRANCH_SO]

Each build runs in a child process of its own (ICL_SO_PATH; BRANCH_SO defaults to the tree's library).  The child times
load_synthetic(1) three times (wall clock: blob generation, packing, upload), embeds 4 icl_synth_images images with the seed-1
synthetic model in each precision and head, and with the variant blob of tests/resnet_blocks.py (a bias everywhere, gammas of both
signs, bn_eps 1e-3) in bf16, and prints a SHA-256 of every output array.  The parent prints both columns; exit status 1 when a digest
differs or the branch's median load time exceeds the parent's slowest repeat.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child():
    from imageclust_amd import _lib as L
    from tests import resnet_blocks as RB

    out = {"so": L.SO_PATH, "load_s": [], "sha": {}}
    ctx = L.Context(0)
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.load_synthetic(1)
        out["load_s"].append(time.perf_counter() - t0)
    imgs = L.synth_images(20250217, 0, 4, L.SYNTH_STRUCTURED)
    precs = (("fp32", L.PREC_FP32), ("bf16", L.PREC_BF16), ("bf16x3", L.PREC_BF16X3))
    for pn, p in precs:
        for hn, h in (("pooled", L.HEAD_POOLED), ("dense0", L.HEAD_DENSE0)):
            out["sha"]["synthetic %s %s" % (pn, hn)] = hashlib.sha256(ctx.embed_u8(imgs, h, p).tobytes()).hexdigest()
    ctx.load_blob(RB.variant_blob(L.synthetic_blob(1)))
    out["sha"]["variant bf16 pooled"] = hashlib.sha256(ctx.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16).tobytes()).hexdigest()
    ctx.close()
    print(json.dumps(out))


def main():
    if sys.argv[1:] == ["--child"]:
        return child()
    sos = {"parent": os.path.abspath(sys.argv[1]), "branch": os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ""}
    res = {}
    for name, so in sos.items():
        env = dict(os.environ)
        env.pop("ICL_SO_PATH", None)
        if so:
            env["ICL_SO_PATH"] = so
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print("%s: exit %d\n%s" % (name, r.returncode, r.stderr[-3000:]))
            return 1
        res[name] = json.loads(r.stdout.strip().split("\n")[-1])
        print("%s: %s" % (name, os.path.relpath(res[name]["so"], ROOT)))
    bad = 0
    print("%-26s %-64s %-64s" % ("output", "parent sha256", "branch sha256"))
    for k, a in res["parent"]["sha"].items():
        b = res["branch"]["sha"][k]
        bad += a != b
        print("%-26s %s %s %s" % (k, a, b, "same" if a == b else "DIFFERS"))
    lp, lb = res["parent"]["load_s"], res["branch"]["load_s"]
    print("load_synthetic wall s, parent: %s" % " ".join("%.3f" % v for v in lp))
    print("load_synthetic wall s, branch: %s" % " ".join("%.3f" % v for v in lb))
    slow = sorted(lb)[1] > max(lp)
    print("branch median %.3f s, parent slowest %.3f s: %s" % (sorted(lb)[1], max(lp), "SLOWER" if slow else "ok"))
    print("ALL DIGESTS MATCH" if not bad else "%d DIGESTS DIFFER" % bad)
    return 1 if bad or slow else 0


if __name__ == "__main__":
    sys.exit(main())
