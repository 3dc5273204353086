"""The bit-exact convolution check (tests/conv_exact.py) on the CPU: every case of tests/test_conv_exact_gpu.py meets exact_ref's own
conditions (span, fp32-exact epilogue, shares of rounded outputs and ties) with no GPU, the numpy model of a kernel reproduces the
reference bit for bit, and the comparison has teeth: each of nine planted mistakes is reported, while the tolerance the other
convolution tests use (resnet_blocks.bounds) lets truncation, round-half-up, the double rounding and a single dropped product through."""
import numpy as np
import pytest

from tests import conv_exact as CE
from tests import resnet_blocks as RB

# one conv_wr_kernel case, one conv_p8_kernel 3x3 case and one split-operand case of the GPU module
TEETH = {"conv_wr": (CE.conv(3, 9, 128, 512, 1, res=True), "bf16"), "conv_p8_3x3": (CE.conv(11, 7, 128, 256, 3, res=True), "bf16"),
         "x_split": (CE.conv(2, 9, 128, 256, 1, res=True, kind="x_split"), "bf16x3")}
# the mistakes that change a result in that precision at all: the small cases have no lo parts, and the hi + lo store of bf16x3 has
# no single rounding to get wrong
APPLIES = {"bf16": [m for m in CE.MISTAKES if m != "lo_ignored"],
           "bf16x3": ["scale_shift_bf16", "bf16_partial_sums", "dropped_product", "neighbour_shift", "lo_ignored", "relu_before_residual"]}
SLIPS_THROUGH = ("truncation", "round_half_up", "residual_after_rounding", "dropped_product")


def test_teeth_cases_are_gpu_cases():
    assert TEETH["conv_wr"][0] in CE.WR_CASES and TEETH["conv_p8_3x3"][0] in CE.P8_CASES and TEETH["x_split"][0] in CE.X3_SPLIT_CASES
    assert set(m for ms in APPLIES.values() for m in ms) == set(CE.MISTAKES)


@pytest.mark.parametrize("name", list(TEETH))
def test_kernel_model_equals_the_reference(name):
    c, prec = TEETH[name]
    want, v32 = CE.exact_ref(c, prec)
    CE.assert_exact(CE.kernel_model(c, prec), want, v32, name)
    if prec == "bf16":  # the same inputs in the other two precisions: the number itself
        for p in ("fp32", "bf16x3"):
            w, _ = CE.exact_ref(c, p)
            assert np.array_equal(w, v32)
            CE.assert_exact(CE.kernel_model(c, p), w, v32, name + " " + p)


@pytest.mark.parametrize("name,mistake", [(n, m) for n in TEETH for m in APPLIES[TEETH[n][1]]])
def test_every_planted_mistake_is_reported(name, mistake):
    c, prec = TEETH[name]
    want, v32 = CE.exact_ref(c, prec)
    got = CE.kernel_model(c, prec, mistake)
    msg = CE.mismatch_report(got, want, v32, "%s %s" % (name, mistake))
    assert msg is not None, "the exact comparison does not see %s" % mistake
    ndiff = int((got != want).sum())
    print(msg.split("\n")[0])
    assert msg.startswith("%s %s: %d of %d elements differ" % (name, mistake, ndiff, want.size)) and "first at (image, y, x, channel)" in msg
    assert all("%s mod %d:" % (a, m) in msg for a, ms in (("pixel", (16, 32, 64, 256)), ("channel", (8, 16, 32, 128))) for m in ms)
    if mistake == "dropped_product":
        assert ndiff == 1
    if mistake in ("truncation", "round_half_up") and prec == "bf16":  # exactly the outputs the rule is about
        u = v32.view(np.uint32)
        low = u & 0xFFFF
        hit = (low > 0x8000) if mistake == "truncation" else (low == 0x8000) & (((u >> 16) & 1) == 0)
        if mistake == "truncation":
            hit = hit | ((low == 0x8000) & (((u >> 16) & 1) == 1))
        assert np.array_equal(got != want, hit)


@pytest.mark.parametrize("name", ["conv_wr", "conv_p8_3x3"])
@pytest.mark.parametrize("mistake", SLIPS_THROUGH)
def test_the_tolerance_of_the_other_tests_lets_it_through(name, mistake):
    """The proof that the exact comparison sees more: the same wrong result passes the max-norm and median bounds."""
    c, prec = TEETH[name]
    want, v32 = CE.exact_ref(c, prec)
    got = CE.kernel_model(c, prec, mistake)
    assert not np.array_equal(got, want)
    _, emax, emed = RB.errors(got, want)
    bmax, bmed = RB.bounds(prec, want)
    print("%s %s: %d elements differ, max error %.3g of the bound, median %.3g of the bound" % (name, mistake, int((got != want).sum()), emax / bmax, emed / bmed))
    assert emax <= bmax and emed <= bmed
    RB.check_close(got, want, prec, "%s %s" % (name, mistake))


def test_mismatch_report_names_position_bits_and_tie():
    c, prec = TEETH["conv_wr"]
    want, v32 = CE.exact_ref(c, prec)
    tie = np.argwhere((v32.view(np.uint32) & 0xFFFF) == 0x8000)[0]
    got = want.copy()
    got[tuple(tie)] = np.nextafter(got[tuple(tie)], np.float32(np.inf))
    msg = CE.mismatch_report(got, want, v32, "one bit")
    assert "1 of %d elements differ" % want.size in msg and str(tuple(int(v) for v in tie)) in msg and ", a tie" in msg
    assert "0x%08x" % int(want[tuple(tie)].view(np.uint32)) in msg and "channel mod 128: %d:1" % (tie[3] % 128) in msg
    z = np.zeros((1, 1, 1, 8), np.float32)
    assert CE.mismatch_report(-z, z, z, "signed zero") is None  # -0 equals +0


GPU_CONVS = CE.IGEMM_CASES + CE.HALO_CASES + CE.P8_CASES + CE.SPLIT_CASES + CE.WR_CASES + CE.X3_SPLIT_CASES


@pytest.mark.parametrize("c", GPU_CONVS, ids=CE.conv_id)
def test_every_gpu_convolution_case_meets_the_conditions(c):
    Ho = (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1
    for prec in (("bf16x3",) if c.kind != "small" else ("fp32", "bf16", "bf16x3")):
        want, v32 = CE.exact_ref(c, prec)
        assert want.dtype == np.float32 and want.shape == (c.B, Ho, Ho, c.cout)
    if c.kind != "small":
        assert not np.array_equal(CE.kernel_model(c, "bf16x3", "lo_ignored"), want)


@pytest.mark.parametrize("K", [128, 256, 512])
def test_conv_wr_walk_case_meets_the_conditions(K):
    """The multi-tile walk as it is sized on 256 compute units (the GPU test takes the count from device_info), and the rule on others."""
    for ncu in (256, 304, 64, 8):
        c = CE.wr_walk_case(K, ncu)
        pt, nworkers = CE.wr_rule(K, 2048, ncu, c.B * 81)
        ntiles = -(-c.B * 81 // pt)
        assert ntiles > 3 * nworkers and (c.B * 81) % pt != 0 and nworkers % 8 == 0
    assert CE.wr_rule(128, 2048, 256, 1 << 20)[1] == 64
    CE.exact_ref(CE.wr_walk_case(K, 256), "bf16")


@pytest.mark.parametrize("shape,relu", CE.DUAL_CASES, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_gpu_dual_case_meets_the_conditions(shape, relu):
    for prec in ("fp32", "bf16", "bf16x3"):
        want, v32 = CE.dual_ref(shape, relu, prec)
    d = CE.dual_case(shape)
    # the exact arithmetic against the float64 reference of the parity tests on the same inputs
    ref = RB.dual_ref(d["x"], d["w1"], d["x2"], d["w2"], d["stride2"], d["scale"], d["shift"], relu)
    assert np.array_equal(ref, v32.astype(np.float64))


@pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
@pytest.mark.parametrize("shape", CE.BNECK_CASES, ids=lambda s: "b%d_h%d_w%d" % s)
def test_every_gpu_bottleneck_case_meets_the_conditions(shape, ds):
    d = CE.bneck_case(shape, ds)
    assert d["want"].shape == shape + (256,) and np.array_equal(d["want"], RB.bf16_round(d["v32"]))
