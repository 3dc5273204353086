#!/usr/bin/env python3
"""Which finishes of the batched merge loops do the suite's small inputs reach?  finish_path_coverage.py [OUT.txt]

Needs a library built with -DICL_WARD_TIMERS (scratch/build_timers.sh; select it with ICL_SO_PATH): with ICL_WARD_STATS set such a build
reports every batched loop's counters on stderr.  Runs every input of tests/ward_cases.py small_cases() -- the adversarial batch inputs of
tests/test_ward_gpu.py are among them -- plus that file's wide and odd-dimension inputs, in the forced modes of the suite: auto (exact fill
below n = 4096), ICL_DIST_BOUND, ICL_DIST_LWBOUND with complete rows and with ICL_WARD_WIDE=0, and UPDATE_FAST.  Each call's report is
read from a redirected stderr and booked under the rows the loop used (last_ward_mode): bound rows = ward_finish_lb_kernel, exact rows and
FAST rows = ward_finish_batch_kernel.  Per kind of rows: steps, and how many ended express (steps - non-express), truncated,
with a stale preselection, with a new row first, and single-pick steps.  Exit status 1 when one of them is 0.
"""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    os.environ["ICL_WARD_STATS"] = "1"
    from imageclust_amd import _lib
    from tests import ward_cases as WC

    cases = list(WC.small_cases()) + [("mog_%d_%d" % (n, d), WC.mog(n, d, n + d), mn, mx)
                                      for n, d, mn, mx in [(100, 4096, 2, 10), (90, 2052, 1, 7), (700, 6, 1, 9), (600, 5, 2, 40), (600, 8, 2, 40)]]
    modes = [("auto", 0, None, 0), ("bound", 2, None, 0), ("lwbound_complete_rows", 4, "1", 0), ("lwbound_wide0", 4, "0", 0), ("fast", 0, None, 1)]
    names = {_lib.ROWS_LW_BOUND: "bound rows (ward_finish_lb_kernel)", _lib.ROWS_EXACT_BATCH: "exact rows (ward_finish_batch_kernel)",
             _lib.ROWS_LW_FAST: "FAST rows (ward_finish_batch_kernel, lw)"}
    keys = ["calls", "steps", "express", "truncated", "stale_preselection", "new_row_first", "single_pick", "general_path"]
    tot = {v: dict.fromkeys(keys, 0) for v in names.values()}
    ctx = _lib.Context(0)
    for mname, mode, wide, lw in modes:
        if wide is None:
            os.environ.pop("ICL_WARD_WIDE", None)
        else:
            os.environ["ICL_WARD_WIDE"] = wide
        ctx.set_ward_options(mode)
        for cname, E, mn, mx in cases:
            if E.shape[0] < 2:
                continue
            sys.stderr.flush()
            saved, tf = os.dup(2), tempfile.TemporaryFile()
            os.dup2(tf.fileno(), 2)
            try:
                ctx.cluster(E, mn, mx, _lib.UPDATE_LW if lw else _lib.UPDATE_EXACT)
            except _lib.ICLError:
                pass
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tf.seek(0)
            text = tf.read().decode(errors="replace")
            a = re.search(r"batched ward: merges (\d+) steps (\d+) commits (\d+) single-pick steps (\d+) general-path steps (\d+)", text)
            b = re.search(r"non-express finishes: truncated (\d+), preselection stale/empty (\d+), new-row-first/forwarding (\d+)", text)
            if not a or not b:
                continue
            t = tot[names[ctx.last_ward_mode()[0]]]
            steps, slow, general = int(a.group(2)), int(a.group(4)), int(a.group(5))
            why = [int(b.group(i)) for i in (1, 2, 3)]
            for k, v in zip(keys, [1, steps, steps - sum(why), why[0], why[1], why[2], slow, general]):
                t[k] += v
    ctx.close()
    lines, bad = [], 0
    for name, t in tot.items():
        lines.append("%-42s %s" % (name, " ".join("%s %d" % (k, t[k]) for k in keys)))
        bad += any(t[k] == 0 for k in keys[2:7])
    lines.append("every finish (express, truncated, stale preselection, new row first, single pick) occurred for every kind of rows" if not bad
                 else "%d kinds of rows miss a finish" % bad)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
