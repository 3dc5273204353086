"""GPU parity tests of the dual-operand convolution launch (launch_conv_fused_ds of imageclust_amd/csrc/resnet.hip: block 0 of
stages 2-4 as one convolution over K = [Cin of t2 | Cin2 of the strided block input]) through icl_conv2d_dual, in each of its three
kernels: conv_igemm_kernel<T, 128, DUAL>, conv_p8_kernel<2, 4, .., DUAL> and conv_p8_kernel<4, 2, .., DUAL> (Cout = 128 * odd, which no
ResNet layer selects).  The reference is resnet_blocks.dual_ref in float64, on bf16-rounded operands for bf16.

Tolerances, the project's for one layer: fp32 and bf16x3 1e-4 * max(1, max|ref|); bf16 maximum 1.2e-2 * max(1, max|ref|) and median
2e-3 * max(1, max|ref|).  tests/test_forward_blocks_cpu.py shows what these bounds see."""
import numpy as np
import pytest

from tests import resnet_blocks as RB

pytestmark = pytest.mark.gpu
IDS = lambda s: "b%d_ho%d_h%d_s%d_c%d_%d_%d" % s


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def run(ctx, L, c, prec, mode, counter):
    """One launch under a conv option; asserts which kernel family ran (conv_stats: [0] conv_p8_kernel, [1] the others)."""
    try:
        ctx.set_conv_options(mode)
        before = ctx.conv_stats()
        y = ctx.conv2d_dual(c["x"], c["w1"], c["x2"], c["w2"], c["stride2"], c["scale"], c["shift"], True, prec)
        after = ctx.conv_stats()
    finally:
        ctx.set_conv_options(L.CONV_P8_AUTO)
    if counter is not None:
        assert after[counter] == before[counter] + 1 and after[1 - counter] == before[1 - counter], (before, after)
    return y


@pytest.mark.parametrize("shape", RB.DUAL_SHAPES, ids=IDS)
def test_dual_bf16_both_kernel_families(ctx, L, shape):
    c = RB.dual_case(shape)
    ref = RB.dual_ref(*(RB.bf16_round(c[k]) for k in ("x", "w1", "x2", "w2")), c["stride2"], c["scale"], c["shift"])
    y8 = run(ctx, L, c, L.PREC_BF16, L.CONV_P8_ALL, 0)
    yi = run(ctx, L, c, L.PREC_BF16, L.CONV_P8_OFF, 1)
    RB.check_close(y8, ref, "bf16", "dual %s conv_p8" % (shape,))
    RB.check_close(yi, ref, "bf16", "dual %s conv_igemm" % (shape,))
    d = np.abs(y8.astype(np.float64) - yi).max()
    assert d <= RB.bounds("bf16", ref)[0], "the two kernel families differ by %.4e" % d
    # a lone image reproduces its rows bit for bit: a tile's result does not depend on the images beside it
    B = shape[0]
    lone = dict(c, x=c["x"][B - 1:], x2=c["x2"][B - 1:])
    assert np.array_equal(run(ctx, L, lone, L.PREC_BF16, L.CONV_P8_ALL, 0)[0], y8[B - 1])
    assert np.array_equal(run(ctx, L, lone, L.PREC_BF16, L.CONV_P8_OFF, 1)[0], yi[B - 1])


@pytest.mark.parametrize("shape", RB.DUAL_SHAPES, ids=IDS)
def test_dual_fp32(ctx, L, shape):
    c = RB.dual_case(shape)
    ref = RB.dual_ref(c["x"], c["w1"], c["x2"], c["w2"], c["stride2"], c["scale"], c["shift"])
    RB.check_close(run(ctx, L, c, L.PREC_FP32, L.CONV_P8_AUTO, 1), ref, "fp32", "dual %s" % (shape,))


@pytest.mark.parametrize("shape", RB.DUAL_SHAPES, ids=IDS)
def test_dual_bf16x3_both_kernel_families(ctx, L, shape):
    c = RB.dual_case(shape)
    ref = RB.dual_ref(c["x"], c["w1"], c["x2"], c["w2"], c["stride2"], c["scale"], c["shift"])
    RB.check_close(run(ctx, L, c, L.PREC_BF16X3, L.CONV_P8_ALL, 0), ref, "bf16x3", "dual %s conv_p8" % (shape,))
    RB.check_close(run(ctx, L, c, L.PREC_BF16X3, L.CONV_P8_OFF, 1), ref, "bf16x3", "dual %s conv_igemm" % (shape,))


def test_dual_rejects_bad_arguments(ctx, L):
    z = lambda *s: np.zeros(s, np.float32)
    with pytest.raises(L.ICLError) as ei:  # output row 6 would read row 12 of a 12-row second operand
        ctx.conv2d_dual(z(1, 7, 7, 64), z(128, 64), z(1, 12, 12, 64), z(128, 64), 2, z(128), z(128))
    assert ei.value.code == L.ICL_ERR_ARG
    with pytest.raises(L.ICLError) as ei:
        ctx.conv2d_dual(z(1, 7, 7, 64), z(128, 64), z(1, 14, 14, 32), z(128, 32), 2, z(128), z(128))
    assert ei.value.code == L.ICL_ERR_UNSUPPORTED
    with pytest.raises(L.ICLError) as ei:
        ctx.conv2d_dual(z(1, 7, 7, 64), z(64, 64), z(1, 14, 14, 64), z(64, 64), 2, z(64), z(64))
    assert ei.value.code == L.ICL_ERR_UNSUPPORTED
