"""Child process of tests/test_stem_exact_gpu.py (no test in here): ICL_FUSE is read once per process, so the stem kernels the default mask
does not select run in a fresh process that the test starts with the mask in its environment.

    python stem_exact_child.py BLOB.npy OUT.npz BLOBNAME ROUTE

ROUTE "pool": icl_stem_pool in bf16 (under ICL_FUSE=7: stem_pool_kernel<BF16>).  ROUTE "taps": tap 0 of icl_embed_taps in every precision
(under ICL_FUSE=0: stem_conv_kernel + maxpool_kernel in fp32 and bf16, the forward plan's stem_pool_kernel<F32, SPLIT> in bf16x3).
Every walk of stem_exact.WALKS, and the uncapped run of each capped walk's input, goes to OUT under "<kind>.<prec>.<images>.<cap>"."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from imageclust_amd import _lib as L  # noqa: E402
from tests import stem_exact as SE  # noqa: E402


def main(blob_path, out_path, blob, route):
    assert route in ("pool", "taps")
    ctx = L.Context(0)
    out = {}
    try:
        ctx.load_blob(np.load(blob_path))
        for kind in SE.KINDS_OF[blob]:
            for prec in SE.PRECS_OF[kind] if route == "taps" else ("bf16",):
                p = getattr(L, "PREC_" + prec.upper())
                for B, cap in sorted(set(SE.WALKS) | {(B, 0) for B, _ in SE.WALKS}):
                    imgs = SE.images_of(kind)[:B]
                    ctx.set_stem_max_blocks(cap)
                    out["%s.%s.%d.%d" % (kind, prec, B, cap)] = ctx.stem_pool(imgs, p) if route == "pool" else ctx.embed_taps(imgs, 0, p)
        ctx.set_stem_max_blocks(0)
    finally:
        ctx.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(*sys.argv[1:5])
