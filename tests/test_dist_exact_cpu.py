"""The bit-exact check of the FAST-mode distance matrix (tests/dist_exact.py) on the CPU: every case of tests/test_dist_exact_gpu.py meets
expected's own conditions (e = hi + lo, span, norms, fp32-exact values) and the floors on what it exercises with no GPU, the numpy model
of the kernel reproduces the expected matrix bit for bit, and the comparison has teeth: each of eleven planted mistakes is reported by
bit equality on at least one case, while the criterion of test_mfma_distance_tile_error_bound (2e-5 of 0.5 (|a|^2 + |b|^2) on a mixture
of Gaussians) lets several of them through.  The split bound the GPU file's entry-wise bound starts from is checked here in float64."""
import numpy as np
import pytest

from tests import dist_exact as DE

# floors on what a case exercises (shares of expected()); a case below them does not test what it is for
SPLIT_LO_SHARE = 0.02      # split: coordinates with lo != 0
SPLIT_LOLO_PAIRS = 0.10    # split, sparse: pairs with la.lb != 0
SPARSE_LO_SHARE = 0.0015   # sparse (d = 2048): four split columns per row, three of 2048 guaranteed
CLAMP_ENTRIES = 8          # clamp: entries whose exact value is negative (every pair of rows 2p, 2p + 1: n // 2 of them where n < 16)

# the cases the planted mistakes are tried on: the ragged three-tile-row shape in every family, and the 96 k-step case
TEETH = [(300, 100, kind) for kind in DE.KINDS] + [(129, 65, "split"), DE.LONG_CASE]
# the shapes and seeds of test_mfma_distance_tile_error_bound that fit a CPU test
OLD_SHAPES = [(130, 64), (257, 100), (129, 1000)]
SLIPS_THROUGH = ("lolo_included", "no_clamp", "negative_zero_kept")


def test_teeth_cases_are_gpu_cases():
    assert all(c in DE.EXACT_CASES for c in TEETH)
    assert DE.PITCH_CASE[2] == "split" and DE.PACKED_CASE in DE.EXACT_CASES
    assert len(set(DE.EXACT_CASES)) == len(DE.EXACT_CASES) == len(DE.NS) * (len(DE.DS) - 1 + len(DE.KINDS)) + 1


@pytest.mark.parametrize("case", DE.EXACT_CASES + [DE.PITCH_CASE], ids=DE.case_id)
def test_every_gpu_case_meets_the_conditions_and_the_floors(case):
    n, d, kind = case
    E = DE.exact_rows(n, d, 0, kind)
    assert E.shape == (n, d) and E.dtype == np.float32
    m = E.astype(np.float64) * 16
    assert np.array_equal(m, np.rint(m))
    want, s = DE.expected(E)  # raises where equality would not be legitimate
    assert want.shape == (n, n) and want.dtype == np.float32 and not np.signbit(want).any() and not np.triu(want).any()
    pairs = n * (n - 1) // 2
    if kind == "small":
        assert s["lo_nonzero"] == 0 and s["not_plain"] == 0 and (np.abs(m) <= 3).all()
    if kind == "split":
        assert s["lo_nonzero"] >= SPLIT_LO_SHARE, s
    if kind == "sparse":
        assert s["lo_nonzero"] >= SPARSE_LO_SHARE, s
    if kind in ("split", "sparse") and pairs:
        assert s["lolo_pairs"] >= SPLIT_LOLO_PAIRS and s["not_plain"] >= SPLIT_LOLO_PAIRS * pairs, s
    if kind == "duplicates" and n >= 4:
        dup = np.tri(n, n, -1, dtype=bool) & (E[:, None, :] == E[None, :, :]).all(2)
        assert dup.sum() >= n // 4 and (want[dup] > 0).all(), "a pair of copies must come out as sum lo^2 > 0"
    if kind == "clamp":
        assert s["clamped"] >= min(CLAMP_ENTRIES, n // 2), s
    if kind == "zero_rows":
        zero = ~E.any(axis=1)
        assert zero[0] and (n < 16 or zero.sum() >= 2)
        assert not want[np.ix_(zero, zero)].any()
    # the model of the kernel computes exactly this
    DE.assert_same_bits(DE.kernel_model(E), want, DE.case_id(case))


def test_d0_is_all_zero():
    want, s = DE.expected(np.zeros((129, 0), np.float32))
    assert not want.view(np.uint32).any() and s["clamped"] == 0
    DE.assert_same_bits(DE.kernel_model(np.zeros((129, 0), np.float32)), want)


def test_every_planted_mistake_is_reported_by_bit_equality():
    print()
    table = {}
    for mistake in DE.MISTAKES:
        hits = []
        for case in TEETH:
            E = DE.exact_rows(case[0], case[1], 0, case[2])
            want, _ = DE.expected(E)
            msg = DE.same_bits(DE.kernel_model(E, mistake), want, DE.case_id(case))
            if msg is not None:
                ndiff = int(msg.split(": ")[1].split(" ")[0])
                assert msg.startswith("%s: %d of %d entries differ, first at (i, j) = (" % (DE.case_id(case), ndiff, want.size)) and "tile (" in msg
                hits.append((DE.case_id(case), ndiff))
        table[mistake] = hits
        print("%-20s caught on %d of %d cases: %s" % (mistake, len(hits), len(TEETH), ", ".join("%s (%d entries)" % h for h in hits)))
    missed = [m for m, hits in table.items() if not hits]
    assert not missed, "the exact comparison does not see %s" % missed
    # what each family is for
    caught_on = lambda m, kind: any(cid.endswith(kind) for cid, _ in table[m])
    assert caught_on("no_clamp", "clamp") and caught_on("negative_zero_kept", "clamp") and caught_on("diagonal_not_zero", "duplicates")
    assert caught_on("lolo_included", "split") and caught_on("dropped_last_kstep", "sparse") and caught_on("neighbour_row", "zero_rows")
    assert not any(table[m] and caught_on(m, "small") for m in ("lo_ignored", "dropped_segment", "lolo_included", "truncating_split", "norms_from_hi"))


def old_criterion(D, E):
    """test_mfma_distance_tile_error_bound's figure and verdict (the diagonal is zero, max error below 2e-5 of the scale)."""
    ref, scale, _ = DE.reference(E)
    err = np.abs(np.tril(D, -1).astype(np.float64) - np.tril(ref, -1)) / np.maximum(scale, 1e-30)
    return float(err.max()), bool(np.all(np.diag(D) == 0) and err.max() < 2e-5)


def test_the_old_criterion_lets_mistakes_through():
    """The proof that the gap was real: the same wrong matrices, on the inputs of the old test, pass its 2e-5."""
    print()
    passes = {}
    for mistake in (None,) + DE.MISTAKES:
        res = [old_criterion(DE.kernel_model(E, mistake), E) for E in (DE.mog(n, d, n + d) for n, d in OLD_SHAPES)]
        passes[mistake] = all(ok for _, ok in res)
        print("%-20s max err / scale %s -> the old criterion %s" % (mistake or "(the kernel)", " ".join("%.2e" % e for e, _ in res), "PASSES" if passes[mistake] else "fails"))
    assert passes[None]
    slipped = [m for m in DE.MISTAKES if passes[m]]
    print("let through by the old criterion: %s" % ", ".join(slipped))
    assert len(slipped) >= 3 and set(SLIPS_THROUGH) <= set(slipped)


def test_same_bits_names_position_tile_and_edge():
    want, _ = DE.expected(DE.exact_rows(300, 100, 0, "split"))
    got = want.copy()
    got[255, 128] = np.nextafter(got[255, 128], np.float32(np.inf))
    got[260, 3] += 1
    msg = DE.same_bits(got, want, "two entries")
    assert msg.startswith("two entries: 2 of 90000 entries differ, first at (i, j) = (255, 128)") and "0x%08x" % int(want.view(np.uint32)[255, 128]) in msg
    assert msg.endswith("tile (1, 1), last row of the tile, first column of the tile")
    z = np.zeros((2, 2), np.float32)
    assert DE.same_bits(z, z) is None and "0x80000000" in DE.same_bits(-z, z)  # -0 is not +0
    nan = np.full((1, 1), np.nan, np.float32)
    assert DE.same_bits(nan, nan) is None


def test_buffer_report_sees_every_kind_of_stray_write():
    n, ld = 131, 136
    want, _ = DE.expected(DE.exact_rows(*DE.PITCH_CASE[:2], 0, DE.PITCH_CASE[2]))
    buf = np.full(n * ld + 64, DE.SENTINEL, np.uint32)
    rows = buf[:n * ld].reshape(n, ld)
    low = np.tri(n, ld, 0, dtype=bool)
    rows[low] = np.where(np.tri(n, n, 0, dtype=bool), want.view(np.uint32), 0)[np.tri(n, n, 0, dtype=bool)]
    assert DE.buffer_report(buf, n, ld, want) is None
    for (i, j), text in (((5, 6), "outside the lower triangle"), ((7, 133), "a pad column"), ((130, 135), "a pad column")):
        b = buf.copy()
        b[i * ld + j] = 0
        assert text in DE.buffer_report(b, n, ld, want)
    b = buf.copy()
    b[n * ld + 3] = 0
    assert "3 words past the end" in DE.buffer_report(b, n, ld, want)
    b = buf.copy()
    b[9 * ld + 9] = 0x80000000  # -0 on the diagonal
    assert "first at (i, j) = (9, 9)" in DE.buffer_report(b, n, ld, want)


@pytest.mark.parametrize("shape", DE.BOUND_SHAPES, ids=lambda s: "n%d_d%d" % s)
def test_split_bound_holds_on_every_float_family(shape):
    """|a.b - (ha.hb + ha.lb + la.hb)| <= 3.01 * 2^-16 sum |a_k b_k|, in float64 (whose own error, d * 2^-53 of sum |a_k b_k|, is six orders below
    the 0.01 * 2^-16 of slack); the bound is not slack by orders: one dominant coordinate comes within a factor of three of it."""
    print()
    worst = {}
    for kind in DE.FLOAT_KINDS:
        dot, three, absdot = DE.three_products(DE.float_rows(shape[0], shape[1], kind))
        ratio = np.abs(dot - three) / np.maximum(absdot, 1e-300)
        worst[kind] = float(ratio.max())
        print("n %d d %d %-16s max |a.b - three products| / sum |a_k b_k| = %.3f * 2^-16" % (shape + (kind, worst[kind] * 2 ** 16)))
        assert (np.abs(dot - three) <= DE.SPLIT_COEFF * absdot).all(), kind
    assert max(worst.values()) > 2.0 ** -16
