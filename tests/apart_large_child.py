"""Child process of test_cluster_apart_large_gpu.py::test_constrained_and_unconstrained_steps_do_not_share_a_graph: under the ICL_WARD_*
switches the parent put into the environment (read once per process), ONE context runs the problems of an npz in the order given -- kind
"apart": Context.cluster_apart, kind "seeded": Context.cluster_seeded on the same seeds -- and writes every call's results and row mode."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from imageclust_amd import _lib  # noqa: E402

if __name__ == "__main__":
    jobs, order = np.load(sys.argv[1]), sys.argv[3].split(",")
    C, ss, mn, mx, kt, cls, pairs = (jobs[k] for k in ("C", "ss", "mn", "mx", "kt", "cls", "pairs"))
    ctx = _lib.Context(0)
    out = {}
    for i, kind in enumerate(order):
        if kind == "apart":
            r = ctx.cluster_apart(C, ss, int(mn), int(mx), int(kt), cls, pairs)
        else:
            r = ctx.cluster_seeded(C, ss, int(mn), int(mx), int(kt))
        for k, v in zip(("cid", "rank", "nc", "st", "log", "co"), r):
            out["%s%d" % (k, i)] = np.asarray(v)
        out["mode%d" % i] = np.array([int(x) for x in ctx.last_ward_mode()], np.int32)
        out["vals%d" % i] = ctx.last_merge_values()
    ctx.close()
    np.savez(sys.argv[2], **out)
