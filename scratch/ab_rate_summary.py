#!/usr/bin/env python3
"""Two builds of the library under the rate scripts: ab_rate_summary.py DIR OUT.json

DIR holds what the scripts wrote with --out, one process per file, the builds alternating (ICL_SO_PATH): SCRIPT_parentK.json and
SCRIPT_branchK.json.  For every figure a script reports as {"median": ..} (a rate or a time over its repetitions): the parent runs'
medians and their range, the pooled range of all parent repetitions (the runs' min and max), the branch runs' medians, the median of
those, and whether it lies inside the range of the parent's medians / inside the pooled range.  No figure is dropped.
"""
import glob
import json
import os
import re
import sys

import numpy as np


def figures(node, path=""):
    if isinstance(node, dict):
        if "median" in node and "min" in node and "max" in node:
            yield path, node
            return
        for k, v in node.items():
            yield from figures(v, path + "/" + k if path else k)


def main():
    src, out = sys.argv[1], sys.argv[2]
    runs = {}  # script -> build -> [figures of run 1, run 2, ...]
    for f in sorted(glob.glob(os.path.join(src, "*.json"))):
        m = re.match(r"(.+)_(parent|branch)(\d+)\.json$", os.path.basename(f))
        if m:
            runs.setdefault(m.group(1), {}).setdefault(m.group(2), []).append(dict(figures(json.load(open(f)))))
    res, outside = {}, []
    for script, builds in runs.items():
        res[script] = dict(parent_runs=len(builds["parent"]), branch_runs=len(builds["branch"]), figures={})
        for name in builds["parent"][0]:
            P, B = [r[name] for r in builds["parent"]], [r[name] for r in builds["branch"]]
            pm, bm = [r["median"] for r in P], [r["median"] for r in B]
            lo, hi, b = min(r["min"] for r in P), max(r["max"] for r in P), float(np.median(bm))
            fig = dict(parent_medians=pm, parent_median_range=[min(pm), max(pm)], parent_pooled_range=[lo, hi], branch_medians=bm, branch_median=b,
                       inside_parent_median_range=bool(min(pm) <= b <= max(pm)), inside_parent_pooled_range=bool(lo <= b <= hi))
            res[script]["figures"][name] = fig
            if not fig["inside_parent_median_range"]:
                outside.append("%s %s: %.6g, parent medians %.6g .. %.6g (pooled %.6g .. %.6g)" % (script, name, b, min(pm), max(pm), lo, hi))
    res["branch_median_outside_parent_median_range"] = outside
    with open(out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print("\n".join(outside) if outside else "every branch median lies inside the range of the parent's medians")


if __name__ == "__main__":
    main()
