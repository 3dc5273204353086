"""The references of the per-block GPU tests (tests/resnet_blocks.py) checked on the CPU: the blob reader and block_ref are right, and
the bounds of tests/test_conv_dual_gpu.py and tests/test_forward_blocks_gpu.py have teeth."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import resnet_blocks as RB


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def chains(L):
    """Per blob ("synthetic", "variant"): the model, its ICLW bytes and the fp32 block_ref chain (taps 0..16) on the tap images."""
    imgs = RB.tap_images(L)
    out = {}
    blob = L.synthetic_blob(1)
    for name, bl in (("synthetic", blob), ("variant", RB.variant_blob(blob))):
        model = RB.read_blob(bl)
        taps = {0: RB.stem_ref(model, imgs)}
        taps.update(RB.chain_ref(model, taps[0]))
        out[name] = (model, bl, taps, imgs)
    return out


@pytest.mark.parametrize("name", ["synthetic", "variant"])
def test_blob_reader_and_block_ref_against_whole_oracle(chains, name):
    """The fp32 block_ref chained over all 16 bottlenecks from the oracle's stem + maxpool, average-pooled, against
    icl_ref_resnet50_forward on the noise image: the two differ only in where BatchNorm is applied (folded scale / shift against
    gamma * (x - mean) / sqrt(var + eps) + beta), so they agree within the fp32 bound 1e-4 * max(1, max|ref|).  The variant blob
    puts a bias on every convolution, negative gammas and another epsilon through the reader's folding."""
    model, blob, taps, imgs = chains[name]
    assert len(model.layers) == 53 and [len(b) for b in RB.blocks_of(model)] == [4, 3, 3, 4, 3, 3, 3, 4, 3, 3, 3, 3, 3, 4, 3, 3]
    if name == "variant":
        assert model.has_bias[:53].all() and abs(model.eps - 1e-3) < 1e-9 and (model.layers[7].scale < 0).any()
    ref, _ = O.resnet50_forward(blob, imgs[0])
    pooled = taps[16][0].astype(np.float64).mean(axis=(0, 1))
    err = np.abs(pooled - ref).max()
    print("%s: pooled max err %.3e, bound %.3e" % (name, err, 1e-4 * max(1.0, np.abs(ref).max())))
    assert err <= 1e-4 * max(1.0, np.abs(ref).max())


def _moved(mut, ref, prec):
    """How far a mistake moves the reference, in units of the bound(s) the GPU test applies: (maximum, median or None)."""
    _, emax, emed = RB.errors(mut, ref)
    bmax, bmed = RB.bounds(prec, ref)
    return emax / bmax, (None if bmed is None else emed / bmed)


def _seen(mv):
    return mv[0] >= 3.0 or (mv[1] is not None and mv[1] >= 3.0)


@pytest.mark.parametrize("shape", RB.DUAL_SHAPES, ids=lambda s: "b%d_ho%d_h%d_s%d_c%d_%d_%d" % s)
def test_dual_bounds_have_teeth(shape):
    """Each known mistake of a dual-operand kernel moves dual_ref, on the inputs of tests/test_conv_dual_gpu.py, by at least 3 x
    the bound that test applies (bf16: operands rounded to bf16, bound 1.2e-2 on the maximum; fp32 / bf16x3: 1e-4).

    Measured, bf16, movement of the maximum in units of its bound, the smallest over the shapes: gather_row_plus1 58 x, odd_h2 (the
    four shapes with an odd H2) 56 x, drop_last64 17 x (K = 1536, of which 64 channels are 4 %), zero_ragged_rows (M is no multiple
    of 256 in any of the shapes) 57 x.  The median moves by at least 7 x its bound for the two gather mistakes, by 0.9 x for
    drop_last64 and not at all for zero_ragged_rows (few rows change): there the maximum is what sees it.  fp32 / bf16x3: 120 times
    the figures of the maximum."""
    c = RB.dual_case(shape)
    B, Ho, H2, s2 = shape[:4]
    M = B * Ho * Ho
    mistakes = ["gather_row_plus1", "drop_last64"] + (["odd_h2"] if H2 % 2 else []) + (["zero_ragged_rows"] if M % 256 else [])
    for prec in ("bf16", "fp32"):
        a = {k: (RB.bf16_round(v) if prec == "bf16" and k in ("x", "w1", "x2", "w2") else v) for k, v in c.items()}
        ref = RB.dual_ref(**a)
        for mk in mistakes:
            mv = _moved(RB.dual_ref(mistake=mk, **a), ref, prec)
            print("dual %s %s %s: max x%.1f median %s" % (shape, prec, mk, mv[0], "-" if mv[1] is None else "x%.1f" % mv[1]))
            assert _seen(mv), (shape, prec, mk, mv)


BLOCK0_TAPS = (1, 4, 8, 14)


@pytest.mark.parametrize("tap", BLOCK0_TAPS)
def test_block_bounds_have_teeth(chains, tap):
    """Each known mistake of block 0 of a stage moves block_ref by at least 3 x the bound tests/test_forward_blocks_gpu.py applies,
    on that test's inputs: the tap images through the synthetic and the variant blob, the block's input being the previous tap (here
    from the fp32 chain, rounded to bf16 for bf16; on the GPU the engine's own).  Movement of the bf16 reference in units of the bounds
    (maximum 1.2e-2, median 2e-3, both times max(1, max|ref|)), measured, as maximum / median:

        mistake         blob        stage 1        stage 2        stage 3        stage 4
        ds_scale_s3     synthetic   51 / 0.35      35 / 0.70      40 / 0.33      50 / 0.42
        ds_scale_s3     variant     83 / 20        78 / 11        83 / 17        69 / 15
        no_shiftds      synthetic   4.7 / 0.32     0.91 / 0.06    0.15 / 0       0.01 / 0       <- unseen beyond stage 1
        no_shiftds      variant     8.8 / 1.1      6.1 / 0.16     8.6 / 1.3      7.0 / 0.53
        wrap_column     synthetic   37 / 0         24 / 0         20 / 0         21 / 0
        wrap_column     variant     14 / 0         13 / 0         17 / 0         14 / 0
        t2_unrounded    synthetic   0.19 / 0       0.15 / 0       0.18 / 0       0.14 / 0       <- the bounds cannot see it
        t2_unrounded    variant     0.12 / 0       0.08 / 0       0.08 / 0       0.08 / 0       <- the bounds cannot see it

    "shift3 without shiftds" is invisible in the synthetic blob beyond stage 1 whatever the image: its activations double per
    bottleneck (max|ref| 45 after stage 2's first block, 6 800 after stage 4's), and a shift of at most 0.65 is then far below 1.2e-2 *
    max|ref|.  That is why the variant blob keeps its activations of order 1 (resnet_blocks.variant_blob) and why the GPU test runs all
    four stages on it: the assertion on no_shiftds is made there.  A t2 left unrounded (one bf16 ulp of an intermediate, 2^-9
    relative) stays within a sixth of the bound everywhere: the per-block bounds do not tell whether the engine rounds t2, and this
    test asserts that they do not, so that nobody believes otherwise.  In fp32 / bf16x3 (bound 1e-4) ds_scale_s3 moves the maximum by
    more than 4 000 x the bound in both blobs; no_shiftds by 560, 110, 18 and 0.95 x (stages 1 to 4) in the synthetic blob -- unseen
    in stage 4 even in fp32 -- and by more than 700 x in the variant blob."""
    for name in ("synthetic", "variant"):
        model, _, taps, _ = chains[name]
        layers = RB.blocks_of(model)[tap - 1]
        for prec in ("bf16", "fp32"):
            x = RB.bf16_round(taps[tap - 1]) if prec == "bf16" else taps[tap - 1]
            ref = RB.block_ref(layers, x, prec)
            for mk in ("ds_scale_s3", "no_shiftds", "wrap_column", "t2_unrounded"):
                if prec == "fp32" and mk in ("t2_unrounded", "wrap_column"):
                    continue  # (fp32 has no rounding of t2; the 3x3 layer's border is covered in bf16, at a bound 120 times wider)
                mv = _moved(RB.block_ref(layers, x, prec, mk), ref, prec)
                print("block %d %s %s %s: max x%.2f median %s" % (tap, name, prec, mk, mv[0], "-" if mv[1] is None else "x%.2f" % mv[1]))
                if mk == "t2_unrounded":
                    assert mv[0] <= 1.0 / 3 and mv[1] <= 1.0 / 3, (tap, name, mk, mv)
                elif mk == "no_shiftds" and name == "synthetic" and tap > 1:
                    assert prec == "fp32" or not _seen(mv), (tap, name, mk, mv)  # documented above: the variant blob is what sees it
                else:
                    assert _seen(mv), (tap, name, prec, mk, mv)
