"""conv_p8_kernel at the edges of its prologue and epilogue, bit for bit (tests/conv_exact.py): tiles far smaller than one tile, tiles
whose rows span images, a full tile beside a ragged one (the epilogue's two paths), every one of the nine taps invalid somewhere (the tap
mask), three column tiles, K of two and of four K-tiles (prologue and peeled K-tiles only; one steady-state iteration), a strided 1x1
layer and the dual-operand launch.

Every case runs on conv_p8_kernel: the context is created with ICL_CONV_WR=0 (read once per context, icl_create), so that the 1x1
layers of K = 128 and 256 do not go to conv_wr_kernel, and under ICL_CONV_P8_ALL; conv_stats() must show one launch of the first counter
(conv_wr_kernel / conv_p8_kernel) and none of the second.  bf16 is the flagship's precision; bf16x3 runs the X3 instantiations (twice
the K-tiles) on the same inputs.

The CPU tests of this file (not marked gpu) assert exact_ref's own conditions on each case, as tests/test_conv_exact_cpu.py does for its
lists, and that each case covers what it is listed for."""
import os

import numpy as np
import pytest

from tests import conv_exact as CE
from tests import resnet_blocks as RB

ALL = 2
PRECS = ("bf16", "bf16x3")
# (case, full tiles along M, rows of the ragged last tile): M against the layout's tile height (256 for Cout % 256 == 0, else 512)
CASES = [
    (CE.conv(1, 7, 128, 256, 3), 0, 49),                   # far less than one tile; every one of the 9 taps is invalid somewhere
    (CE.conv(5, 7, 128, 128, 3), 0, 245),                  # 4 x 2 layout; the images span the wave rows
    (CE.conv(2, 15, 128, 256, 3), 1, 194),                 # odd width; a full tile and a ragged one
    (CE.conv(3, 14, 128, 128, 3), 1, 76),                  # 4 x 2 layout: a full 512 tile and a ragged one
    (CE.conv(3, 13, 128, 384, 3, relu=False), 0, 507),     # three column tiles
    (CE.conv(2, 9, 128, 256, 1), 0, 162),                  # K = 128: two K-tiles, prologue and peeled tiles only
    (CE.conv(2, 9, 256, 256, 1, res=True), 0, 162),        # four K-tiles: one steady-state iteration
    (CE.conv(1, 16, 256, 512, 1, 2), 0, 64),               # strided 1x1 layer
]
IDS = [CE.conv_id(c) for c, _, _ in CASES]


def dual_eligible(shape):
    """conv_p8_eligible (conv_p8.h) for a dual-operand launch: whole K-tiles of both operands, an even number of them, Cout % 128 == 0."""
    B, Ho, H2, s2, cin, cin2, cout = shape
    return cin % 64 == 0 and cin2 % 64 == 0 and (cin + cin2) % 128 == 0 and cout % 128 == 0


def smallest_dual_shape():
    """The eligible shape of resnet_blocks.DUAL_SHAPES with the fewest multiply-adds."""
    return min((s for s in RB.DUAL_SHAPES if dual_eligible(s)), key=lambda s: s[0] * s[1] * s[1] * (s[4] + s[5]) * s[6])


# ---- CPU: the cases meet the conditions of the exact comparison and cover what they are listed for ----------------------------------
@pytest.mark.parametrize("c,full,ragged", CASES, ids=IDS)
def test_case_meets_the_conditions(c, full, ragged):
    Ho = (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1
    for prec in ("fp32",) + PRECS:
        want, v32 = CE.exact_ref(c, prec)
        assert want.dtype == np.float32 and want.shape == (c.B, Ho, Ho, c.cout)
    bm = 256 if c.cout % 256 == 0 else 512
    M = c.B * Ho * Ho
    assert (M // bm, M % bm) == (full, ragged)
    for prec in PRECS:  # conv_p8_eligible under ICL_CONV_P8_ALL: whole K-tiles, an even number of them
        K = c.k * c.k * c.cin * (2 if prec == "bf16x3" else 1)
        assert c.cout % 128 == 0 and c.cin % 64 == 0 and K % 128 == 0
        assert CE.route(c, "bf16x3", ALL).startswith("conv_p8")


def test_every_tap_is_invalid_somewhere_and_images_span_wave_rows():
    c = CASES[0][0]  # 7 x 7, pad 1: tap (kh, kw) is invalid in row 0 / 6 for kh = 0 / 2, in column 0 / 6 for kw = 0 / 2; the centre tap only beyond M
    assert c.k == 3 and c.H == 7 and c.B * 49 < 256
    c = CASES[1][0]  # wave rows are 128 pixels: 49 does not divide 128
    assert c.cout % 256 != 0 and 128 % (c.H * c.H) != 0 and c.B * c.H * c.H > 128


def test_dual_case_meets_the_conditions():
    shape = smallest_dual_shape()
    assert shape in RB.DUAL_SHAPES and dual_eligible(shape)
    for prec in ("fp32",) + PRECS:
        CE.dual_ref(shape, False, prec)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    old = os.environ.get("ICL_CONV_WR")
    os.environ["ICL_CONV_WR"] = "0"  # read by icl_create: this context's 1x1 layers of K <= 512 do not go to conv_wr_kernel
    try:
        c = L.Context(0)
    finally:
        if old is None:
            del os.environ["ICL_CONV_WR"]
        else:
            os.environ["ICL_CONV_WR"] = old
    c.set_conv_options(ALL)
    yield c
    c.close()


def on_conv_p8(ctx, call):
    before = ctx.conv_stats()
    y = call()
    after = ctx.conv_stats()
    assert tuple(a - b for a, b in zip(after, before)) == (1, 0), (before, after)
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("c,full,ragged", CASES, ids=IDS)
def test_conv_p8_edges(ctx, L, c, full, ragged):
    d = CE.case_of(c)
    for prec in PRECS:
        want, v32 = CE.exact_ref(c, prec)
        y = on_conv_p8(ctx, lambda: ctx.conv2d_fused(d["x"], d["w"], d["scale"], d["shift"], c.stride, d["pad"], d["res"] if c.res else None, c.relu,
                                                     getattr(L, "PREC_" + prec.upper())))
        CE.assert_exact(y, want, v32, "%s %s on conv_p8_kernel" % (CE.conv_id(c), prec))


@pytest.mark.gpu
def test_conv_p8_dual_edge(ctx, L):
    shape = smallest_dual_shape()
    d = CE.dual_case(shape)
    for prec in PRECS:
        want, v32 = CE.dual_ref(shape, False, prec)
        y = on_conv_p8(ctx, lambda: ctx.conv2d_dual(d["x"], d["w1"], d["x2"], d["w2"], d["stride2"], d["scale"], d["shift"], False, getattr(L, "PREC_" + prec.upper())))
        CE.assert_exact(y, want, v32, "dual %s %s on conv_p8_kernel" % (shape, prec))
