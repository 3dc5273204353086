"""The bit-exact stem check (tests/stem_exact.py) on the CPU: the builders' exactness conditions hold for every case of
tests/test_stem_exact_gpu.py (the loader's fold gives scale == gamma, the pixel claims, the budget below 2^24 quanta, one tap per channel
and all 147 taps over the three hot blobs, every byte value pinned), the numpy model of the kernels and of their persistent unit walk
reproduces the reference bit for bit, and the comparison has teeth: each of ten planted mistakes is reported on the inputs the GPU tests use,
while the tolerances that held the stem so far (resnet_blocks.bounds: 1e-4 max|ref| in fp32, 1.2e-2 max|ref| in bf16) let the rounding
mistakes and px / 255.0f through.

What no input can catch, and why: px / 255.0f in bf16 -- bf16(px / 255.0f) == bf16(px * (float)(1.0 / 255.0)) for all 256 byte values, so
there it is no mistake (asserted below; fp32 and bf16x3 see it on 126 byte values); the shift added after the bf16 rounding on the
one-hot models and on the binary images -- the product (there: the integer sum times the scale, whose large values come from the channels of
scale 2) is a bf16 number already, so the first rounding changes nothing; the many-valued "grid" images see it; and the walk mistakes on a grid with one workgroup per unit, which is why the GPU tests cap the grid."""
import numpy as np
import pytest

from tests import conv_exact as CE
from tests import resnet_blocks as RB
from tests import stem_exact as SE

CASES = [(blob, kind, prec) for blob in SE.BLOBS for kind in SE.KINDS_OF[blob] for prec in SE.PRECS_OF[kind]]
case_id = lambda c: "_".join(str(v) for v in c) if isinstance(c, tuple) else str(c)
INT_BIN, INT_GRID, INT_F32, INT_X3 = ("int", "binary", "bf16"), ("int", "grid", "bf16"), ("int", "binary", "fp32"), ("int", "binary", "bf16x3")
HOT_F32, HOT_BF16, HOT_X3 = ("hot0", "onehot", "fp32"), ("hot1", "onehot", "bf16"), ("hot2", "onehot", "bf16x3")
ANY = [INT_BIN, INT_GRID, INT_F32, HOT_F32, HOT_BF16, HOT_X3]
# mistake -> the cases (of the GPU tests) that must report it, and the walks (images, grid) it is planted in
APPLIES = {"carry_leak": (ANY, [(3, 8), (2, 5), (1, 1)]), "prefetch_same_image": (ANY, [(3, 8), (2, 5)]),
           "px_truncated": ([INT_GRID, HOT_BF16], [(3, 8)]), "px_divided": ([HOT_F32, HOT_X3], [(3, 8)]),
           "truncation": ([INT_BIN, INT_GRID, HOT_BF16], [(3, 8)]), "round_half_up": ([INT_BIN, INT_GRID, HOT_BF16], [(3, 8)]),
           "shift_after_rounding": ([INT_GRID], [(3, 8)]), "dropped_tap": (ANY + [INT_X3], [(3, 8)]),
           "col16_pooled": (ANY, [(3, 8)]), "pad_neighbour": (ANY, [(3, 8)])}
TEETH = [(m, c, w) for m, (cases, walks) in APPLIES.items() for c in cases for w in walks]
SLIPS_THROUGH = [("truncation", INT_BIN), ("round_half_up", INT_BIN), ("truncation", INT_GRID),
                 ("round_half_up", INT_GRID), ("shift_after_rounding", INT_GRID), ("px_truncated", INT_GRID), ("px_divided", HOT_F32)]


def test_builders_hold_their_conditions():
    assert set(APPLIES) == set(SE.MISTAKES) and all(c in CASES for cs, _ in APPLIES.values() for c in cs)
    SE.check_pixels()
    assert len(SE.taps_covered()) == 147
    for blob in SE.BLOBS:
        c0 = SE.conv0_of(blob)  # (asserts scale == gamma, shift == beta, bf16-exact W and W * scale)
        assert set(np.abs(c0["scale"]).tolist()) <= {0.5, 1.0, 2.0} and (c0["scale"] < 0).any() and (c0["scale"] > 0).any()
        assert np.array_equal(c0["shift"] * 8, np.rint(c0["shift"] * 8)) and not c0["mean"].any()
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(SE.pixels(b, "bf16"), SE.pixels(b, "bf16", "px_divided"))  # no mistake in bf16
    assert (SE.pixels(b, "fp32") != SE.pixels(b, "fp32", "px_divided")).sum() == 126
    for kind in ("binary", "grid", "onehot"):  # bright last rows in front of a boundary, dark first rows behind it
        im = SE.images_of(kind).astype(np.float64)
        assert im.shape == (SE.NIMG, 224, 224, 3) and im[:, 208:].mean() > 8 * im[:, :8].mean()


def test_the_blob_carries_conv0_through_the_loaders_fold():
    """write_blob -> read_blob (the loader's arithmetic): conv0's folded scale and shift are gamma and beta, every other layer is unchanged."""
    from imageclust_amd import _lib as L

    base = L.synthetic_blob(1)
    model = RB.read_blob(base)
    m = RB.read_blob(SE.blob_of("hot1", model))
    c0 = SE.conv0_of("hot1")
    assert m.eps == SE.BN_EPS and np.array_equal(m.layers[0].W, c0["W"])
    assert np.array_equal(m.layers[0].scale, c0["gamma"]) and np.array_equal(m.layers[0].shift, c0["beta"])
    assert all(np.array_equal(a.W, b.W) for a, b in zip(m.layers[1:], model.layers[1:])) and np.array_equal(m.fcw, model.fcw)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_gpu_case_meets_the_conditions_and_the_model_equals_the_reference(case):
    blob, kind, prec = case
    r = SE.exact_ref(*case)
    assert r["want"].shape == (SE.NIMG, 56, 56, 64) and r["want"].dtype == np.float32 and (r["want"] >= 0).all()
    assert (r["span"] is None) == (kind == "onehot" and prec != "bf16")
    rounded, ties, up = CE.rounding_shares(r["v32"])
    print(SE.report_line("(reference)", blob, kind, prec, SE.NIMG, 0, r["v32"], r["want"], r["want"]), "budget", r["span"])
    if prec == "bf16":  # a case cannot pass because nothing in it had to be rounded
        n = r["v32"].size
        assert rounded >= 0.1 and ties * n >= 200 and up * n >= 100, (rounded, ties, up)  # (absolute numbers, as conv_exact.finish's "chain")
    for B, G in ((3, 8), (2, 5)):
        for folded in ((False, True) if prec == "bf16" else (False,)):
            SE.assert_exact(SE.kernel_model(blob, kind, prec, B, G, folded), r["want"][:B], r["v32"][:B], "model %s B %d grid %d" % (case_id(case), B, G))
    if blob == "hot0" and prec == "fp32":
        SE.onehot_pins_every_byte(blob)


@pytest.mark.parametrize("mistake,case,walk", TEETH, ids=case_id)
def test_every_planted_mistake_is_reported(mistake, case, walk):
    blob, kind, prec = case
    B, G = walk
    r = SE.exact_ref(*case)
    want, v32 = r["want"][:B], r["v32"][:B]
    for folded in ((False, True) if prec == "bf16" else (False,)):
        got = SE.kernel_model(blob, kind, prec, B, G, folded, mistake)
        what = "%s %s%s" % (mistake, case_id(case), " folded" if folded else "")
        msg = SE.stem_report(got, want, v32, what)
        assert msg is not None, "the exact comparison does not see %s" % what
        bad = np.argwhere(got != want)
        print(msg.split("\n")[0])
        assert msg.startswith("%s: %d of %d elements differ" % (what, len(bad), want.size))
        assert "(image, pooled row mod 4, pooled column mod 7, channel mod 16): count" in msg and "tile (pooled row // 4):" in msg and "strip (pooled column // 7):" in msg
        if mistake == "carry_leak":  # pooled row 0 of the units a workgroup does not start with, and nothing else
            assert (bad[:, 1] == 0).all() and "tile (pooled row // 4): 0:%d\n" % len(bad) in msg
            assert all((int(b) * 8 + int(x) // 7) >= G for b, x in zip(bad[:, 0], bad[:, 2]))
        if mistake == "prefetch_same_image":  # tile 0 and the row it hands on, of the images behind a boundary
            assert (bad[:, 1] <= 4).all() and (bad[:, 0] >= 1).all()
        if mistake == "col16_pooled":
            assert (bad[:, 2] % 7 == 6).all() and (bad[:, 2] < 49).all()
        if mistake == "pad_neighbour":
            assert np.isin(bad[:, 2], (0, 1, 55)).all()  # conv columns 0, 1 and 111 read padding
        if mistake == "dropped_tap":
            assert (bad[:, 3] == SE.dropped_tap_of(blob)[0]).all()
        if mistake in ("truncation", "round_half_up"):  # exactly the outputs the rule is about (rounding is monotonic: the pooled exact value decides)
            u = np.ascontiguousarray(v32).view(np.uint32)
            low, odd = u & 0xFFFF, ((u >> 16) & 1) == 1
            hit = (low > 0x8000) | ((low == 0x8000) & odd) if mistake == "truncation" else (low == 0x8000) & ~odd
            assert np.array_equal(got != want, hit)


@pytest.mark.parametrize("mistake,case", SLIPS_THROUGH, ids=case_id)
def test_the_tolerance_of_the_other_stem_tests_lets_it_through(mistake, case):
    """The same wrong result passes test_stem_pool_fused_matches_oracle's and test_tap0_is_the_stem's max-norm (and median) bounds."""
    blob, kind, prec = case
    r = SE.exact_ref(*case)
    got = SE.kernel_model(blob, kind, prec, SE.NIMG, 8, False, mistake)
    assert not np.array_equal(got, r["want"])
    _, emax, emed = RB.errors(got, r["want"])
    bmax, bmed = RB.bounds(prec, r["want"])
    print("%s %s: %d elements differ, max error %.3g of the bound" % (mistake, case_id(case), int((got != r["want"]).sum()), emax / bmax))
    assert emax <= bmax and (bmed is None or emed <= bmed)
    RB.check_close(got, r["want"], prec, "%s %s" % (mistake, case_id(case)))
    assert emax <= (1.2e-2 if prec == "bf16" else 1e-4) * np.abs(r["want"]).max()  # the bounds as the stem tests state them


def test_stem_report_names_the_pixel():
    r = SE.exact_ref("int", "binary", "bf16")
    got = r["want"].copy()
    got[2, 9, 34, 37] += 1.0
    got[2, 13, 41, 21] += 1.0
    msg = SE.stem_report(got, r["want"], r["v32"], "two pixels")
    assert "2 of %d elements differ" % got.size in msg and "first at (image, y, x, channel) = (2, 9, 34, 37)" in msg
    assert "  (2, 1, 6, 5): 2" in msg and "tile (pooled row // 4): 2:1 3:1" in msg and "strip (pooled column // 7): 4:1 5:1" in msg
    assert SE.stem_report(r["want"].copy(), r["want"], r["v32"], "equal") is None
