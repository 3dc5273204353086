"""Child process of test_seeded_fast_gpu.py::test_one_merge_per_step_loop_equals_restatement: runs the seeded problems of an npz through
Context.cluster_seeded(update=UPDATE_LW) under whatever ICL_WARD_* switches the parent put into the environment (they are read once per
process), and leaves each call's results, merge heights and row mode."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from imageclust_amd import _lib  # noqa: E402

if __name__ == "__main__":
    jobs, count = np.load(sys.argv[1]), int(sys.argv[3])
    ctx = _lib.Context(0)
    out = {}
    for i in range(count):
        C, ss, mn, mx, kt = (jobs["%s%d" % (k, i)] for k in "CSNXK")
        r = ctx.cluster_seeded(C, ss, int(mn), int(mx), int(kt), update=_lib.UPDATE_LW)
        for k, v in zip(("cid", "rank", "nc", "st", "log", "co"), r):
            out["%s%d" % (k, i)] = np.asarray(v)
        out["val%d" % i] = ctx.last_merge_values() if r[3] == _lib.ICL_OK else np.zeros(0, np.float32)
        out["mode%d" % i] = np.array([int(x) for x in ctx.last_ward_mode()], np.int32)
    ctx.close()
    np.savez(sys.argv[2], **out)
