"""The FAST-mode distance matrix, dist_split_kernel + dist_mfma_kernel (distance_mfma.hip), through icl_distance_mfma_dev with the test owning
the pitch and seeing the whole buffer: every cell is prefilled with a sentinel NaN, entries j <= i must have the wanted bits and EVERY other
cell -- above the diagonal, pad columns, behind the last row -- must still hold the sentinel.
  a  bit equality on inputs with one correct bit pattern per entry (tests/dist_exact.py; conditions and teeth: tests/test_dist_exact_cpu.py);
  b  every pitch class: ld = n .. n + 5, the 16-byte stores (ld % 4 == 0) and the scalar ones;
  c  invariances on ordinary floats that need no reference and no tolerance: a row pair's entry does not depend on which lanes, tiles or
     k padding it meets, nor on a NaN / Inf row elsewhere;
  d  an entry-wise bound against float64 on adversarial floats (dist_exact.error_bound), no entry with its sign bit set;
  e  the packed form FAST clustering uses (dist_mfma_kernel<0>): singleton merges have the expected entries as heights, bit for bit.
The checker of the bound tests, icl_distance_bounds_check_dev, is held to the oracle-pinned exact matrix by its sum of values
(tests/test_dist_i8_epilogue_gpu.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import dist_exact as DE
from tests import lw_numpy as LW

pytestmark = pytest.mark.gpu
TAIL = 64  # sentinel words kept behind the last row


@pytest.fixture(scope="module")
def ctx():
    from imageclust_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def run(ctx, E, ld=None):
    """icl_distance_mfma_dev on rows E with pitch ld -> the whole buffer (n * ld + TAIL uint32), prefilled with the sentinel."""
    from imageclust_amd import _lib

    E = np.ascontiguousarray(E, np.float32)
    n, d = E.shape
    ld = n if ld is None else ld
    buf = np.full(n * ld + TAIL, DE.SENTINEL, np.uint32)
    dE, dD = ctx.malloc(max(E.nbytes, 16)), ctx.malloc(buf.nbytes)
    try:
        assert dD % 16 == 0
        if E.size:
            ctx.h2d(dE, E)
        ctx.h2d(dD, buf)
        _lib.check(ctx.h, _lib.load().icl_distance_mfma_dev(ctx.h, C.c_void_p(dE), n, d, C.c_void_p(dD), ld))
        ctx.d2h(buf, dD)
    finally:
        ctx.free(dE)
        ctx.free(dD)
    return buf


def matrix(ctx, E, ld=None):
    """The dense lower triangle [n][n] fp32 (+0 above the diagonal), after checking that nothing else in the buffer was written."""
    n = len(E)
    ld = n if ld is None else ld
    buf = run(ctx, E, ld)
    rows = buf[:n * ld].reshape(n, ld)
    low = np.tri(n, n, 0, dtype=bool)
    D = np.where(low, rows[:, :n], 0).astype(np.uint32).view(np.float32)
    msg = DE.buffer_report(buf, n, ld, D, "n %d d %d ld %d" % (n, E.shape[1], ld))
    assert msg is None, msg
    return D


def check_exact(ctx, case, ld=None):
    n, d, kind = case
    E = DE.exact_rows(n, d, 0, kind)
    want, shares = DE.expected(E)
    what = DE.case_id(case) + ("" if ld is None else "_ld%d" % ld)
    print("%s: %s" % (what, shares))
    msg = DE.buffer_report(run(ctx, E, ld), n, n if ld is None else ld, want, what)
    assert msg is None, msg


# ---- a. one correct bit pattern per entry --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DE.DS)
@pytest.mark.parametrize("n", DE.NS)
def test_exact_inputs_bit_for_bit(ctx, n, d):
    cases = [c for c in DE.EXACT_CASES if c[:2] == (n, d)]
    assert len(cases) == (len(DE.KINDS) if d == 100 else 1)
    for case in cases:
        check_exact(ctx, case)


def test_exact_inputs_bit_for_bit_over_96_k_steps(ctx):
    check_exact(ctx, DE.LONG_CASE)


@pytest.mark.parametrize("n", [1, 129])
def test_d0_is_all_plus_zero(ctx, n):
    """d = 0 is accepted (dp = 0, K' = 192 of zeros): every entry of the triangle is +0."""
    msg = DE.buffer_report(run(ctx, np.zeros((n, 0), np.float32)), n, n, np.zeros((n, n), np.float32), "n %d d 0" % n)
    assert msg is None, msg


# ---- b. pitch and untouched cells ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", DE.PITCHES)
def test_every_pitch_class_bit_for_bit(ctx, ld):
    assert DE.PITCH_CASE[0] == DE.PITCHES[0] and [p % 4 == 0 for p in DE.PITCHES] == [False, True, False, False, True]
    check_exact(ctx, DE.PITCH_CASE, ld)


# ---- c. invariances on ordinary floats -------------------------------------------------------------------------------------------------
INV_KINDS = ("normal", "offset", "huge_coordinate")
_full = {}


def full(ctx, kind, n=300, d=100):
    if (kind, n, d) not in _full:
        _full[kind, n, d] = matrix(ctx, DE.float_rows(n, d, kind))
    return _full[kind, n, d]


@pytest.mark.parametrize("kind", INV_KINDS)
def test_prefix_invariance(ctx, kind):
    E, D = DE.float_rows(300, 100, kind), full(ctx, kind)
    for m in (127, 128, 129, 256, 257):
        DE.assert_same_bits(matrix(ctx, E[:m]), D[:m, :m], "%s: D(E[:%d]) against D(E)[:%d, :%d]" % (kind, m, m, m))


@pytest.mark.parametrize("kind", INV_KINDS)
def test_subselection_invariance(ctx, kind):
    """The same pair of rows on other lanes and tiles, diagonal and interior."""
    E, D = DE.float_rows(300, 100, kind), full(ctx, kind)
    for name, S in (("every second row", np.arange(0, 300, 2)), ("all rows but the first", np.arange(1, 300))):
        DE.assert_same_bits(matrix(ctx, E[S]), D[np.ix_(S, S)], "%s, %s" % (kind, name))


@pytest.mark.parametrize("kind", INV_KINDS)
def test_zero_padding_invariance(ctx, kind):
    for d, to in ((100, 128), (1, 64)):
        E = DE.float_rows(300, d, kind)
        P = np.zeros((300, to), np.float32)
        P[:, :d] = E
        DE.assert_same_bits(matrix(ctx, P), full(ctx, kind, 300, d), "%s: d = %d zero-padded to %d" % (kind, d, to))


@pytest.mark.parametrize("kind", INV_KINDS)
def test_nan_and_inf_rows_stay_in_their_rows_and_columns(ctx, kind):
    n, bad = 260, (70, 200)
    Z = DE.float_rows(n, 100, kind).copy()
    Z[list(bad)] = 0.0
    E = Z.copy()
    E[70] = DE.float_rows(n, 100, kind)[70]
    E[70, 37] = np.nan
    E[200] = np.inf
    D, D0 = matrix(ctx, E), matrix(ctx, Z)
    hit = np.zeros((n, n), bool)
    hit[list(bad), :] = hit[:, list(bad)] = True
    hit &= np.tri(n, n, -1, dtype=bool)
    assert hit.sum() == 70 + 200 + (n - 71) + (n - 201) - 1
    assert (np.isnan(D[hit]) | (np.isposinf(D[hit]))).all(), "%s: a finite entry in the row or column of a NaN / Inf row" % kind
    assert D[70, 70] == 0 and D[200, 200] == 0
    DE.assert_same_bits(np.where(hit, 0, D), np.where(hit, 0, D0), "%s: entries away from the NaN and Inf rows" % kind)


# ---- d. entry-wise bound against float64 ---------------------------------------------------------------------------------------------
FIGURES = {}


@pytest.mark.parametrize("kind", DE.FLOAT_KINDS)
@pytest.mark.parametrize("shape", DE.BOUND_SHAPES, ids=lambda s: "n%d_d%d" % s)
def test_entrywise_error_bound_against_fp64(ctx, shape, kind):
    """|D - ref| <= B_ij (dist_exact.error_bound) for every entry, and no sign bit.  The figures (max err / B, and the scale-relative figure of
    test_mfma_distance_tile_error_bound) are printed; with ICL_DIST_EXACT_RECORD=<file> they are also written there as JSON."""
    n, d = shape
    E = DE.float_rows(n, d, kind)
    D = matrix(ctx, E)
    ref, scale, _ = DE.reference(E)
    B = DE.error_bound(E)
    low = np.tri(n, n, -1, dtype=bool)
    err = np.abs(D.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(B[low] > 0, err[low] / B[low], np.where(err[low] > 0, np.inf, 0.0)).max())
        old = float(np.where(scale[low] > 0, err[low] / scale[low], 0.0).max())
        # the accumulation and norm part alone: against the float64 sum of the same bf16 products (entries the clamp changed left out)
        _, three, absdot = DE.three_products(E)
        t64 = scale - three
        part = (B - DE.SPLIT_COEFF * absdot)[low]
        keep = D[low] > 0
        acc = float(np.where(keep & (part > 0), np.abs(D.astype(np.float64) - t64)[low] / part, 0.0).max())
    FIGURES["n%d_d%d_%s" % (n, d, kind)] = {"max_err_over_B": ratio, "max_err_over_scale": old, "max_err_less_split_over_rest_of_B": acc}
    print("n %d d %d %-16s max err / B = %.3f   max err / scale = %.3g (old tolerance 2e-5)   accumulation and norms alone / their part of B = %.3f" % (n, d, kind, ratio, old, acc))
    path = os.environ.get("ICL_DIST_EXACT_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)
    assert np.isfinite(D[low]).all()
    assert not np.signbit(D).any(), "%d entries have their sign bit set" % int(np.signbit(D).sum())
    worst = np.unravel_index(np.where(low, err - B, -np.inf).argmax(), err.shape)
    assert (err[low] <= B[low]).all(), "%d entries exceed B, worst at %s: |err| %.3g, B %.3g" % (int((err[low] > B[low]).sum()), worst, err[worst], B[worst])


# ---- e. the packed form ------------------------------------------------------------------------------------------------------------
def test_packed_form_singleton_merges_have_the_expected_heights(ctx):
    """icl_cluster with ICL_UPDATE_LW, max_size 2: every merge joins two singletons, at the height of their entry in dist_mfma_kernel<0>'s packed matrix."""
    from imageclust_amd import _lib

    n, d, kind = DE.PACKED_CASE
    E = DE.exact_rows(n, d, 0, kind)
    want, _ = DE.expected(E)
    ctx.cluster(E, 1, 2, _lib.UPDATE_LW)
    m, v = ctx.last_merges(), ctx.last_merge_values()
    # not vacuous, and nothing but singleton merges: the merge log is the restatement's on the EXPECTED matrix
    wm, wv = LW.cluster_lw(want, 1, 2)[3:5]
    assert len(wm) >= 50 and np.array_equal(m, wm) and ((m[:, 0] < n) & (m[:, 1] < n)).all()
    entry = want[np.maximum(m[:, 0], m[:, 1]), np.minimum(m[:, 0], m[:, 1])]
    bad = np.flatnonzero(v.view(np.uint32) != entry.view(np.uint32))
    assert not len(bad), "%d of %d merges, first merge %d of (%d, %d): height 0x%08x (%r), expected entry 0x%08x (%r)" % (
        len(bad), len(m), bad[0], m[bad[0], 0], m[bad[0], 1], int(v.view(np.uint32)[bad[0]]), float(v[bad[0]]), int(entry.view(np.uint32)[bad[0]]), float(entry[bad[0]]))
