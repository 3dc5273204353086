#!/usr/bin/env python3
"""Two builds of the library, bit for bit, on every merge loop that runs ward.hip's finish steps and lazy selection:
  finish_ab_bits.py PARENT.so BRANCH.so [OUT.txt]

Alternating child processes (ICL_SO_PATH), one per (library, ICL_WARD_BATCH) -- the batch switch is read once per process.  Inputs: the
generators of tests/ward_cases.py, mog at n = 300, 5 000, 24 000 with d = 64 and n = 300 with d = 6 (scalar centroid paths), min / max size
5 / 50.  Loops of a batched process: auto (bound rows with complete rows from n = 4096), ICL_DIST_LWBOUND with complete rows and with
ICL_WARD_WIDE=0, ICL_DIST_BOUND, ICL_DIST_EXACT, UPDATE_FAST; of an ICL_WARD_BATCH=0 process: auto, ICL_DIST_BOUND, ICL_DIST_EXACT,
UPDATE_FAST.  Compared: cluster ids, member ranks, the merge log, every merge value's bits, last_ward_stats (merges, steps, single-pick
steps, sum of live clusters), the row mode and the layout.  Exit status 1 on any difference or failed child.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(300, 64, 1), (5000, 64, 2), (24000, 64, 3), (300, 6, 4)]
BATCHED = [("auto", 0, None, 0), ("lwbound_complete_rows", 4, "1", 0), ("lwbound_wide0", 4, "0", 0), ("bound", 2, None, 0), ("exact", 1, None, 0),
           ("fast", 0, None, 1)]
SINGLE = [("auto", 0, None, 0), ("bound", 2, None, 0), ("exact", 1, None, 0), ("fast", 0, None, 1)]


def child(out, batched):
    from imageclust_amd import _lib
    from tests import ward_cases as WC

    ctx = _lib.Context(0)
    res = {}
    for n, d, seed in CASES:
        E = WC.mog(n, d, seed)
        for name, mode, wide, lw in (BATCHED if batched else SINGLE):
            if wide is None:
                os.environ.pop("ICL_WARD_WIDE", None)
            else:
                os.environ["ICL_WARD_WIDE"] = wide
            ctx.set_ward_options(mode)
            cid, rank, nc = ctx.cluster(E, 5, 50, _lib.UPDATE_LW if lw else _lib.UPDATE_EXACT)
            st = ctx.last_ward_stats()
            key = "n%d_d%d_%s" % (n, d, name)
            res[key + "/cid"] = cid.copy()
            res[key + "/rank"] = rank.copy()
            res[key + "/merges"] = ctx.last_merges().copy()
            res[key + "/value_bits"] = ctx.last_merge_values().view(np.uint32).copy()
            res[key + "/stats"] = np.array([nc, st["merges"], st["steps"], st["single_pick_steps"], st["sum_live"], ctx.last_ward_mode()[0],
                                            int(ctx.last_ward_mode()[1]), int(ctx.last_ward_layout()[0]), ctx.last_ward_bound_violations()], np.int64)
    ctx.close()
    np.savez(out, **res)


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3] == "1")
    parent, branch = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    lines, bad = [], 0
    tmp = tempfile.mkdtemp(prefix="finish_ab_bits_")
    for batched in ("1", "0"):
        got = {}
        for tag, so in (("parent", parent), ("branch", branch)):
            out = os.path.join(tmp, "%s_batch%s.npz" % (tag, batched))
            env = dict(os.environ, ICL_SO_PATH=so, ICL_WARD_BATCH=batched)
            env.pop("ICL_WARD_WIDE", None)
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, batched], env=env, timeout=280).returncode
            if rc != 0:
                print("child %s ICL_WARD_BATCH=%s ended with status %d: nothing more is started" % (tag, batched, rc))
                return 1
            got[tag] = np.load(out)
        P, B = got["parent"], got["branch"]
        assert sorted(P.files) == sorted(B.files)
        for k in sorted(P.files, key=lambda s: (s.split("/")[0], s)):
            same = P[k].shape == B[k].shape and np.array_equal(P[k], B[k])
            bad += not same
            if k.endswith("/stats"):
                s = P[k]
                lines.append("ICL_WARD_BATCH=%s %-34s parent: clusters %d merges %d steps %d single-pick %d sum_live %d rows %d bounds %d complete %d viol %d | branch %s"
                             % (batched, k.split("/")[0], *s.tolist(), "identical" if same else "DIFFERS %s" % B[k].tolist()))
            elif not same:
                lines.append("ICL_WARD_BATCH=%s %s DIFFERS" % (batched, k))
    lines.append("cluster ids, member ranks, merge logs, merge value bits and statistics: %s" % ("ALL IDENTICAL" if not bad else "%d ARRAYS DIFFER" % bad))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
