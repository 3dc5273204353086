"""Bit-exact GPU tests of the four stem kernels -- stem2_pool_kernel, stem_pool_kernel (fp32, the split bf16x3 output, bf16) and
stem_conv_kernel + maxpool_kernel -- including their persistent unit walk, on models and images for which every pooled output has one
correct bit pattern (tests/stem_exact.py: integer or one-hot conv0 weights, a BatchNorm that folds to gamma and beta exactly, binary /
bf16-grid / all-byte images).  The comparison is np.array_equal against float64 im2col -> ReLU -> one rounding -> maxpool; a failure lists
the differing positions as (image, pooled row mod 4, pooled column mod 7, channel mod 16).  tests/test_stem_exact_cpu.py shows on the same
inputs that ten planted mistakes are each reported and that the max-norm bounds of the other stem tests let the rounding ones through.

The walk.  On 256 compute units no workgroup of stem2_pool_kernel walks a second (image, strip) unit below 161 images, so the cases run
under icl_set_stem_max_blocks (tests only; the kernels are the production ones): 3 images on 8 workgroups (each walks one strip of three
successive images: the carried conv row's columns coincide), 2 images on 5 (workgroup 0 walks units 0, 5, 10, 15: the strip changes and
the walk crosses the image boundary), 1 image on 1 (all 8 strips), and the production grid.  The transition t = 13 -> 0, the carry buffer
that still holds the previous unit's conv row 111 and the prefetch across the image boundary are then compared with the reference, and
each capped run is bit-equal to the uncapped run of the same input.  The images are bright in their last rows and dark in their first.

Which kernel runs: icl_stem_pool and tap 0 of icl_embed_taps in this process take stem2_pool_kernel (bf16) and stem_pool_kernel<F32> /
<F32, SPLIT> (fp32 / bf16x3) -- the default ICL_FUSE mask; tests/test_conv_select_cpu.py holds the plan's choice per mask.  The mask is read
once per process, so stem_pool_kernel<BF16> (ICL_FUSE=7) and stem_conv_kernel + maxpool_kernel (ICL_FUSE=0, tap 0) run in fresh child
processes (tests/stem_exact_child.py), one at a time, each under its own timeout."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import resnet_blocks as RB
from tests import stem_exact as SE

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_LIMIT_S = 120
IN_PROCESS = {"bf16": "stem2_pool_kernel", "fp32": "stem_pool_kernel<F32>", "bf16x3": "stem_pool_kernel<F32, SPLIT>"}
# route -> (ICL_FUSE, the precisions it runs, the kernel by precision)
CHILD = {"pool": ("7", ("bf16",), {"bf16": "stem_pool_kernel<BF16>"}),
         "taps": ("0", ("fp32", "bf16x3", "bf16"), {"fp32": "stem_conv_kernel<F32> + maxpool_kernel", "bf16": "stem_conv_kernel<BF16> + maxpool_kernel",
                                                    "bf16x3": "stem_pool_kernel<F32, SPLIT> (plan)"})}


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def base_model(L):
    return RB.read_blob(L.synthetic_blob(1))


class Net:
    def __init__(self, L, name, blob):
        self.name, self.blob, self.ctx = name, blob, L.Context(0)
        self.ctx.load_blob(blob)

    def run(self, cap, call):
        """One call under a cap on the stem's grid, restored afterwards."""
        try:
            self.ctx.set_stem_max_blocks(cap)
            return call()
        finally:
            self.ctx.set_stem_max_blocks(0)


@pytest.fixture(scope="module", params=SE.BLOBS)
def net(request, L, base_model):
    """One context per blob for the whole module (loading the model dominates a test)."""
    n = Net(L, request.param, SE.blob_of(request.param, base_model))
    yield n
    n.ctx.close()


def check(kernel, blob, kind, prec, B, cap, got):
    r = SE.exact_ref(blob, kind, prec)
    want, v32 = r["want"][:B], r["v32"][:B]
    print(SE.report_line(kernel, blob, kind, prec, B, cap, v32, got, want))
    SE.assert_exact(got, want, v32, "%s %s %s %s, %d images, grid cap %d" % (kernel, blob, kind, prec, B, cap))


@pytest.mark.parametrize("walk", SE.WALKS, ids=SE.walk_id)
def test_fused_stems_are_exact_along_the_walk(net, L, walk):
    """stem2_pool_kernel, stem_pool_kernel<F32> and <F32, SPLIT> through icl_stem_pool, and the same launch as the forward plan makes it
    (tap 0 of icl_embed_taps): both places that size the stem's grid take the cap."""
    B, cap = walk
    for kind in SE.KINDS_OF[net.name]:
        imgs = SE.images_of(kind)[:B]
        for prec in SE.PRECS_OF[kind]:
            p = getattr(L, "PREC_" + prec.upper())
            got = net.run(cap, lambda: net.ctx.stem_pool(imgs, p))
            check(IN_PROCESS[prec], net.name, kind, prec, B, cap, got)
            tap = net.run(cap, lambda: net.ctx.embed_taps(imgs, 0, p))
            assert np.array_equal(tap, got), "%s %s: tap 0 of the forward pass differs from icl_stem_pool under cap %d" % (kind, prec, cap)
            if cap:
                assert np.array_equal(net.ctx.stem_pool(imgs, p), got), "%s %s: the capped run differs from the uncapped one" % (kind, prec)


@pytest.mark.parametrize("route", list(CHILD))
def test_other_stems_are_exact_along_the_walk(net, route, tmp_path):
    """stem_pool_kernel<BF16> (ICL_FUSE=7) and stem_conv_kernel + maxpool_kernel (ICL_FUSE=0; bf16x3 there: the plan's split stem), each in a
    fresh child process: every walk equals the reference, and each capped run the uncapped run of the same input."""
    fuse, precs, kernels = CHILD[route]
    blob_path, out_path = str(tmp_path / "blob.npy"), str(tmp_path / "out.npz")
    np.save(blob_path, net.blob)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stem_exact_child.py"), blob_path, out_path, net.name, route], env=dict(os.environ, ICL_FUSE=fuse),
                       capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    assert r.returncode == 0, "child exit %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = np.load(out_path)
    n = 0
    for kind in SE.KINDS_OF[net.name]:
        for prec in (q for q in SE.PRECS_OF[kind] if q in precs):
            for B, cap in SE.WALKS:
                got = out["%s.%s.%d.%d" % (kind, prec, B, cap)]
                check(kernels[prec], net.name, kind, prec, B, cap, got)
                assert np.array_equal(got, out["%s.%s.%d.0" % (kind, prec, B)]), "%s %s: the capped run differs from the uncapped one" % (kind, prec)
                n += 1
    assert n == len(SE.WALKS) * sum(1 for kind in SE.KINDS_OF[net.name] for q in SE.PRECS_OF[kind] if q in precs)
