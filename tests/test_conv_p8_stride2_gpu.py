"""The identity under a pruned bottleneck's c2 (conv_select.h plan_pruned_block): on conv_p8_kernel, the 3x3 / stride 2 / pad 1 convolution
equals the 3x3 / stride 1 / pad 1 convolution sampled at the pixels (2 oy, 2 ox), BIT FOR BIT -- same taps, same zero padding, same k
order (iy0 = 2 oy - 1).  Inputs are Gaussian, rounded to bf16, so that another summation order would show.  Both layouts of the kernel
(Cout = 128: 4 x 2 waves, Cout = 256: 2 x 4 waves), an even and an odd height each, several images, so that the strided launch's tile rows
span images; ICL_CONV_P8_ALL, and the launch counters show that both launches ran on conv_p8_kernel.

tests/test_conv_p8_edges_gpu.py and the exact-convolution cases (tests/conv_exact.py) run stride 2 on conv_p8_kernel for 1x1 layers only
(b1_h16_c256-512_k1_s2, b2_h14_c512-256_k1_s2, b6_h14_c2048-512_k1_s2); a strided 3x3 layer is what this file adds."""
import numpy as np
import pytest

from tests import resnet_blocks as RB

pytestmark = pytest.mark.gpu
CASES = [(3, 8, 128, 128), (3, 7, 128, 128), (2, 14, 128, 256), (3, 9, 128, 256)]  # (B, H, Cin, Cout)


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.set_conv_options(L.CONV_P8_ALL)
    yield c
    c.close()


@pytest.mark.parametrize("B,H,cin,cout", CASES)
def test_stride2_equals_stride1_subsampled(ctx, L, B, H, cin, cout):
    rng = np.random.default_rng([B, H, cin, cout])
    x = RB.bf16_round(rng.standard_normal((B, H, H, cin), np.float32))
    w = RB.bf16_round((rng.standard_normal((cout, cin, 3, 3), np.float32) / np.sqrt(9 * cin)).astype(np.float32))
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (0.25 * rng.standard_normal(cout)).astype(np.float32)
    out = []
    for stride in (1, 2):
        before = ctx.conv_stats()
        out.append(ctx.conv2d_fused(x, w, scale, shift, stride, 1, None, True, L.PREC_BF16))
        assert tuple(a - b for a, b in zip(ctx.conv_stats(), before)) == (1, 0)
    full, strided = out
    Ho = (H - 1) // 2 + 1
    assert full.shape == (B, H, H, cout) and strided.shape == (B, Ho, Ho, cout) and (strided > 0).mean() > 0.2
    want = full[:, ::2, ::2]
    bad = np.nonzero(strided.view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
    assert not len(bad[0]), "%d of %d values differ, first at (b, oy, ox, c) = %s" % (len(bad[0]), want.size, tuple(int(v[0]) for v in bad))
