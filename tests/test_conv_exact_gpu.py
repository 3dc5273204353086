"""Bit-exact GPU tests of every convolution kernel: conv_igemm_kernel, conv3x3_halo_kernel, conv_p8_kernel (both layouts, the
dual-operand and the split form), conv_wr_kernel, and bneck56_kernel (both forms), on inputs whose accumulator and epilogue are exact
in fp32 under any summation order (tests/conv_exact.py).  Each output element has one correct value -- the number itself in fp32 and
bf16x3, its round-to-nearest-even in bf16 -- and the comparison is np.array_equal: truncation, round-half-up, a second rounding,
bf16 partial sums, one lost product or a lost lo part fail it, which the max-norm tolerances of the parity tests let through
(tests/test_conv_exact_cpu.py shows both).  A failure lists the differing positions modulo the kernels' tile sizes.

Kernels are selected through icl_set_conv_options only, and every launch is checked against the launch counters; conv_exact.route
names the kernel (the counters tell conv_wr_kernel / conv_p8_kernel from the 128 x 128 kernels, not the kernels of one counter apart).
fp32 always runs on the 128 x 128 kernels, and conv_wr_kernel and the split form are bf16 only (bf16x3 runs on the 128 x 128 kernels
and on conv_p8_kernel: those two get the split-operand cases).

The stem reads the loaded model, so it has a module of its own, tests/test_stem_exact_gpu.py, which loads models whose conv0 folds
exactly (tests/stem_exact.py) and also walks the stem kernels' persistent grid.  Left out: conv_wr_kernel's ICL_WR_PT256=32 instantiation
(the variable is read once per process)."""
import time

import numpy as np
import pytest

from tests import conv_exact as CE

pytestmark = pytest.mark.gpu
PRECS = ("fp32", "bf16", "bf16x3")
OFF, AUTO, ALL = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    assert (_lib.CONV_P8_OFF, _lib.CONV_P8_AUTO, _lib.CONV_P8_ALL) == (OFF, AUTO, ALL)
    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def launch(ctx, L, mode, split, kernel, call):
    """One launch under a conv option, restored afterwards; the counters must show the launch that `kernel` (conv_exact.route) implies."""
    try:
        ctx.set_conv_options(mode | (L.CONV_SPLIT if split else 0))
        before = ctx.conv_stats() + (ctx.conv_split_launches(),)
        t0 = time.perf_counter()
        y = call()
        ms = 1e3 * (time.perf_counter() - t0)
        after = ctx.conv_stats() + (ctx.conv_split_launches(),)
    finally:
        ctx.set_conv_options(L.CONV_P8_AUTO)
    assert tuple(a - b for a, b in zip(after, before)) == CE.counters_of(kernel), (kernel, before, after)
    return y, ms


def report(what, kernel, prec, d, v32, ms):
    r, t, up = CE.rounding_shares(v32)
    print("conv_exact: %-46s %-6s %-32s M %5d K %4d N %4d  rounded %4.1f %% ties %4.1f %% (up %4.1f %%)  %6.1f ms" %
          (what, prec, kernel, d["M"], d["K"], d["N"], 100 * r, 100 * t, 100 * up, ms))


def run_conv(ctx, L, c, prec, mode, split=False, family=None):
    """Convolution case c in `prec` under `mode`: bit-equal to the one correct output.  family: what the kernel's name must start with."""
    d = CE.case_of(c)
    want, v32 = CE.exact_ref(c, prec)
    kernel = CE.route(c, prec, mode, split)
    assert family is None or kernel.startswith(family), (kernel, family)
    y, ms = launch(ctx, L, mode, split, kernel, lambda: ctx.conv2d_fused(d["x"], d["w"], d["scale"], d["shift"], c.stride, d["pad"], d["res"] if c.res else None,
                                                                       c.relu, getattr(L, "PREC_" + prec.upper())))
    report(CE.conv_id(c), kernel, prec, d, v32, ms)
    CE.assert_exact(y, want, v32, "%s %s on %s" % (CE.conv_id(c), prec, kernel))
    return y


@pytest.mark.parametrize("c", CE.IGEMM_CASES, ids=CE.conv_id)
def test_conv_igemm_kernel(ctx, L, c):
    """M = 147 (a ragged 128-row tile shared by three images), three 64-channel tiles, stride 2, residual without ReLU."""
    for prec in PRECS:  # (bf16x3 sees twice the channels: its 3x3 case goes to the halo kernel)
        run_conv(ctx, L, c, prec, OFF, family=None if prec == "bf16x3" else "conv_igemm")


@pytest.mark.parametrize("c", CE.HALO_CASES, ids=CE.conv_id)
def test_conv3x3_halo_kernel(ctx, L, c):
    for prec in PRECS:
        run_conv(ctx, L, c, prec, OFF, family="conv3x3_halo")


@pytest.mark.parametrize("c", CE.P8_CASES, ids=CE.conv_id)
def test_conv_p8_kernel(ctx, L, c):
    """Both layouts under ICL_CONV_P8_ALL: ragged last tiles, nine taps of several K-tiles, three channel tiles, residual, stride 2."""
    run_conv(ctx, L, c, "fp32", ALL)
    run_conv(ctx, L, c, "bf16", ALL, family="conv_wr" if (c.cin, c.cout, c.k) == (256, 128, 1) else "conv_p8")
    run_conv(ctx, L, c, "bf16x3", ALL, family="conv_p8")


@pytest.mark.parametrize("c", CE.SPLIT_CASES, ids=CE.conv_id)
def test_conv_p8_split_form(ctx, L, c):
    """Two workgroups per tile, the partner's half sums added in fp32: bit-equal to the reference, and so to the one-workgroup form."""
    y2 = run_conv(ctx, L, c, "bf16", ALL, split=True, family="conv_p8_kernel<256x256, split>")
    y1 = run_conv(ctx, L, c, "bf16", ALL, family="conv_p8_kernel<256x256>")
    assert np.array_equal(y1, y2)
    run_conv(ctx, L, c, "fp32", ALL, split=True)
    run_conv(ctx, L, c, "bf16x3", ALL, split=True, family="conv_p8_kernel<256x256>")  # (the split form is bf16 only)


@pytest.mark.parametrize("c", CE.WR_CASES, ids=CE.conv_id)
def test_conv_wr_kernel(ctx, L, c):
    """K = 128 / 256 / 512 with and without residual and ReLU: M = 243, 245, 1 089 (ragged last tiles) and 196."""
    run_conv(ctx, L, c, "bf16", AUTO, family="conv_wr")


@pytest.mark.parametrize("K", [128, 256, 512])
def test_conv_wr_kernel_multi_tile_walk(ctx, L, K):
    """Every worker walks at least three tiles and the last tile is ragged (sized from conv_select's rule and the device's CU count):
    the double buffer is reused, the prefetched residual is used and a tile past the end is requested."""
    run_conv(ctx, L, CE.wr_walk_case(K, ctx.device_info()[1]), "bf16", AUTO, family="conv_wr")


@pytest.mark.parametrize("c", CE.X3_SPLIT_CASES, ids=CE.conv_id)
def test_bf16x3_split_operands(ctx, L, c):
    """x (or w) with non-zero lo parts: wh.xl (or wl.xh) must arrive, on the 128 x 128 kernels and on conv_p8_kernel."""
    run_conv(ctx, L, c, "bf16x3", OFF, family="conv_igemm" if c.k == 1 else "conv3x3_halo")
    run_conv(ctx, L, c, "bf16x3", ALL, family="conv_p8")


@pytest.mark.parametrize("shape,relu", CE.DUAL_CASES, ids=lambda v: "b%d_ho%d_h%d_s%d_c%d_%d_%d" % v if isinstance(v, tuple) else ("relu" if v else "norelu"))
def test_conv2d_dual_in_each_kernel(ctx, L, shape, relu):
    """Two products, one epilogue: conv_igemm_kernel<.., DUAL> and conv_p8_kernel<.., DUAL> in both layouts, selected as
    tests/test_conv_dual_gpu.py selects them."""
    d = CE.dual_case(shape)
    layout = "256x256" if shape[6] % 256 == 0 else "512x128"
    for prec, mode in (("bf16", ALL), ("bf16", OFF), ("fp32", AUTO), ("bf16x3", ALL), ("bf16x3", OFF)):
        kernel = "conv_p8_kernel<%s, dual>" % layout if mode == ALL else "conv_igemm_kernel<128, dual>"
        want, v32 = CE.dual_ref(shape, relu, prec)
        y, ms = launch(ctx, L, mode, False, kernel, lambda: ctx.conv2d_dual(d["x"], d["w1"], d["x2"], d["w2"], d["stride2"], d["scale"], d["shift"], relu,
                                                                           getattr(L, "PREC_" + prec.upper())))
        report("dual b%d_ho%d_h%d_s%d_c%d_%d_%d" % shape, kernel, prec, d, v32, ms)
        CE.assert_exact(y, want, v32, "dual %s %s on %s" % (shape, prec, kernel))


@pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape", CE.BNECK_CASES, ids=lambda s: "b%d_h%d_w%d" % s)
def test_bottleneck56(ctx, L, shape, ds):
    """Three convolutions in one launch: t1 and t2 must be the round-to-nearest-even of their exact values, or the output differs."""
    d = CE.bneck_case(shape, ds)
    p = d["p"]
    t0 = time.perf_counter()
    y = ctx.bottleneck56(d["x"], p["w1"], p["bn1"], p["w2"], p["bn2"], p["w3"], p["bn3"], p.get("wds"), p.get("bnds"))
    what = "bottleneck56 b%d_h%d_w%d %s" % (shape + ("downsample" if ds else "identity",))
    report(what, "bneck56_kernel", "bf16", dict(M=d["M"], K=64, N=256), d["v32"], 1e3 * (time.perf_counter() - t0))
    CE.assert_exact(y, d["want"], d["v32"], what)
