"""GPU tests of the pruned fused stage-1 bottleneck, bneck56_kernel<false, 2> (imageclust_amd/csrc/resnet_fused.h, prune_map.h): stage 2's
block 0 reads stage 1's output at the pixels (2 oy, 2 ox) only, so the last identity block of stage 1 computes its 3x3 and its last 1x1
convolution for those pixels alone and stores nothing else.  Everything here is equality of bits.

1. The kernel alone (icl_bottleneck56_sub: the launch on caller tensors, the output preset to a 16-bit pattern): at every (even row, even
   column) the pruned launch gives the unpruned launch's bits; every other pixel still holds the pattern -- two patterns, one of them a NaN.
   Shapes: 56 x 56; heights where H + 1 is even and odd and the last row is needed and not; widths with a masked strip, an even and an odd
   last column, two and three strips; the ring test's 1400-column shapes, whose runs hold several images, so that the parity of a virtual row
   flips inside a run; run lengths in every residue class of the 4-row step; one image alone against the same image in a batch of 5.
2. The side operand alone: with W3 = 0 the even pixels are bf16(max(x, 0)).
3. Through the model (synthetic weights, bf16): embeddings and taps with the part on and off, the counter of pruned fused launches, a tapped
   tensor whole, no stale pixel after a pruned pass, the other precisions untouched, conv_stats unmoved."""
import numpy as np
import pytest

from tests.test_fused_gpu import L, ctx, _bneck_weights, bf16_round  # noqa: F401  (L, ctx: fixtures)

pytestmark = pytest.mark.gpu

STEP = 4  # BN56_ROWS
WIDE = 1400
FILLS = (0x7FC1, 0x3C5A)  # a quiet NaN with a payload bit, and 0.0133...: neither is a value the ReLU output could be mistaken for by chance
_ids = lambda s: "b%d_h%d_w%d" % s


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _run(ctx, x, p, sub, fill):
    return ctx.bottleneck56_sub(x, p["w1"][:, :, 0, 0], p["bn1"], p["w2"], p["bn2"], p["w3"][:, :, 0, 0], p["bn3"], sub, fill)


def _check_pruned(y2, y1, fill, what):
    """y2 (pruned, preset to fill) against y1 (whole): equal bits at (even, even), the fill pattern everywhere else."""
    b2, b1 = _bits(y2), _bits(y1)
    even = np.zeros(y1.shape[:3], bool)
    even[:, ::2, ::2] = True
    bad = (b2 != b1) & even[..., None]
    assert not bad.any(), "%s: %d words of the needed pixels differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[:4])
    rest = b2[~even]
    assert (rest == np.uint32(fill << 16)).all(), "%s: %d words outside the needed pixels were written" % (what, int((rest != np.uint32(fill << 16)).sum()))


BIG = [(3, 56, 56)]
HEIGHTS = [(2, h, 14) for h in (1, 2, 3, 5, 6, 7)]
WIDTHS = [(2, 6, w) for w in (1, 13, 15, 29)]
# one image per run (few strips: every image has a workgroup of its own): the run is H + 1 rows -- 4, 5, 2, 3
RESIDUES = [(1, 3, 20), (1, 4, 20), (1, 1, 20), (1, 2, 20)]
# 100 strips: at most 4 runs on any device below 500 CUs, so runs of several images; H + 1 = 2 .. 5 rows per image
RUNS = [(5, 1, WIDE), (5, 2, WIDE), (5, 3, WIDE), (5, 4, WIDE)]


def test_residue_shapes_cover_every_class():
    assert {(H + 1) % STEP for _, H, _ in RESIDUES} == set(range(STEP))
    assert {(H + 1) % 2 for _, H, _ in HEIGHTS} == {0, 1} and {(H - 1) % 2 for _, H, _ in HEIGHTS} == {0, 1}


@pytest.mark.parametrize("shape", BIG + HEIGHTS + WIDTHS + RESIDUES + RUNS, ids=_ids)
def test_needed_pixels_equal_the_unpruned_kernel(ctx, shape):
    B, H, Wd = shape
    rng = np.random.default_rng(B * 100000 + H * 10000 + Wd)
    p = _bneck_weights(rng, 256, False)
    x = bf16_round(rng.standard_normal((B, H, Wd, 256)).astype(np.float32))
    y1 = _run(ctx, x, p, 1, FILLS[0])
    assert not (_bits(y1) == np.uint32(FILLS[0] << 16)).all(axis=-1).any(), "the unpruned launch left a pixel unwritten"
    for fill in FILLS:
        _check_pruned(_run(ctx, x, p, 2, fill), y1, fill, "%s fill %04x" % (shape, fill))


def test_sub_1_is_the_forward_pass_launch(ctx):
    rng = np.random.default_rng(5)
    p = _bneck_weights(rng, 256, False)
    x = bf16_round(rng.standard_normal((2, 5, 29, 256)).astype(np.float32))
    y = ctx.bottleneck56(x, p["w1"][:, :, 0, 0], p["bn1"], p["w2"], p["bn2"], p["w3"][:, :, 0, 0], p["bn3"])
    assert np.array_equal(_bits(_run(ctx, x, p, 1, FILLS[1])), _bits(y))


@pytest.mark.parametrize("shape", [(5, 6, 29), (5, 3, WIDE), (5, 2, WIDE)], ids=_ids)
def test_image_alone_equals_the_image_in_a_batch(ctx, shape):
    B, H, Wd = shape
    rng = np.random.default_rng(4242 + H * 10 + Wd)
    p = _bneck_weights(rng, 256, False)
    x = bf16_round(rng.standard_normal((B, H, Wd, 256)).astype(np.float32))
    y = _run(ctx, x, p, 2, FILLS[0])
    for b in range(B):
        alone = _run(ctx, x[b:b + 1], p, 2, FILLS[0])
        assert np.array_equal(_bits(alone[0]), _bits(y[b])), "image %d of %d" % (b, B)


@pytest.mark.parametrize("shape", [(2, 56, 56), (3, 5, 29), (1, 1, 1), (4, 3, 15), (5, 2, WIDE)], ids=_ids)
def test_side_operand_is_exact(ctx, shape):
    """conv1 / conv2 random (they must not leak into the output), conv3 = 0 with shift 0: the residual alone, pixel, column and channel slice."""
    B, H, Wd = shape
    rng = np.random.default_rng(77 + B * 1000 + H * 10 + Wd)
    p = _bneck_weights(rng, 256, False)
    p["w3"] = np.zeros_like(p["w3"])
    p["bn3"] = (np.ones(256, np.float32), np.zeros(256, np.float32))
    x = rng.standard_normal((B, H, Wd, 256)).astype(np.float32)
    want = np.maximum(bf16_round(x), 0) + np.float32(0.0)  # (+ 0.0: the kernel's ReLU turns -0 into +0)
    _check_pruned(_run(ctx, x, p, 2, FILLS[0]), want, FILLS[0], "side operand %s" % (shape,))


# ---- through the model

@pytest.fixture(scope="module")
def imgs(L):
    return np.concatenate([L.synth_images(7, 11, 20, L.SYNTH_NOISE), L.synth_images(20250217, 3, 18, L.SYNTH_STRUCTURED)])


def both(ctx, call, other=None):
    """call() with the fused part off, then on -> (off, on, conv_stats moves, fused counter moves, block counter moves).  `other` (images) is
    embedded with the part off in between, so that the pixels the pruned launch leaves alone hold values of OTHER images."""
    out = []
    try:
        for on in (False, True):
            ctx.set_forward_prune_fused(False)
            if on and other is not None:
                ctx.embed_u8(other, 2048, 1)
            ctx.set_forward_prune_fused(on)
            s0, f0, p0 = ctx.conv_stats(), ctx.forward_prune_fused_stats(), ctx.forward_prune_stats()
            y = call()
            s1, f1, p1 = ctx.conv_stats(), ctx.forward_prune_fused_stats(), ctx.forward_prune_stats()
            out.append((y, tuple(a - b for a, b in zip(s1, s0)), f1 - f0, p1 - p0))
    finally:
        ctx.set_forward_prune_fused(True)
    (y0, s0, f0, p0), (y1, s1, f1, p1) = out
    return y0, y1, (s0, s1), (f0, f1), (p0, p1)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n", [1, 5, 33])
def test_embeddings_are_bit_identical(ctx, L, imgs, n):
    try:
        ctx.set_batch(16)
        nbatches = -(-n // 16)
        off, on, s, f, p = both(ctx, lambda: ctx.embed_u8(imgs[:n], L.HEAD_POOLED, L.PREC_BF16), imgs[::-1][:16])
        assert same_bits(off, on), "%d values differ" % int((off != on).sum())
        assert np.isfinite(on).all() and on.std() > 0
        assert s[0] == s[1] and sum(s[0]) > 0, s      # conv_stats does not move between the part on and off
        assert f == (0, nbatches)                    # one pruned fused launch per batch
        assert p == (2 * nbatches, 2 * nbatches)     # the blocks of stages 2 and 3: counted apart, with the part on and off
    finally:
        ctx.set_batch(256)


def test_tap_behind_the_pruned_launch(ctx, L, imgs):
    off, on, s, f, p = both(ctx, lambda: ctx.embed_taps(imgs[:3], 4, L.PREC_BF16), imgs[::-1][:8])
    assert same_bits(off, on), "tap 4: %d values differ" % int((off != on).sum())
    assert s[0] == s[1] and f == (0, 1) and p == (0, 0)


def test_the_tapped_tensor_is_whole(ctx, L, imgs):
    off, on, s, f, p = both(ctx, lambda: ctx.embed_taps(imgs[:3], 3, L.PREC_BF16), imgs[::-1][:8])
    assert same_bits(off, on), "tap 3: %d values differ" % int((off != on).sum())
    assert (off[:, 1::2, 1::2] != 0).any()
    assert s[0] == s[1] and f == (0, 0) and p == (0, 0)


def test_a_pruned_pass_before_a_tap_leaves_no_stale_pixels(ctx, L, imgs):
    """The pruned launch leaves the odd pixels of its buffer unwritten; a tap-3 pass of other images must overwrite all of its tensor."""
    try:
        ctx.set_forward_prune_fused(False)
        want = ctx.embed_taps(imgs[:2], 3, L.PREC_BF16)
        ctx.set_forward_prune_fused(True)
        f0 = ctx.forward_prune_fused_stats()
        ctx.embed_u8(imgs[2:6], L.HEAD_POOLED, L.PREC_BF16)
        assert ctx.forward_prune_fused_stats() - f0 == 1
        assert same_bits(ctx.embed_taps(imgs[:2], 3, L.PREC_BF16), want)
    finally:
        ctx.set_forward_prune_fused(True)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_other_precisions_are_not_pruned(ctx, L, imgs, prec):
    q = {"fp32": L.PREC_FP32, "bf16x3": L.PREC_BF16X3}[prec]
    off, on, s, f, p = both(ctx, lambda: ctx.embed_u8(imgs[:2], L.HEAD_POOLED, q))
    assert same_bits(off, on) and s[0] == s[1] and f == (0, 0) and p == (0, 0)


def test_forward_prune_off_turns_both_parts_off(ctx, L, imgs):
    try:
        ctx.set_forward_prune(False)
        ctx.set_forward_prune_fused(True)
        f0, p0 = ctx.forward_prune_fused_stats(), ctx.forward_prune_stats()
        off = ctx.embed_u8(imgs[:3], L.HEAD_POOLED, L.PREC_BF16)
        assert (ctx.forward_prune_fused_stats() - f0, ctx.forward_prune_stats() - p0) == (0, 0)
    finally:
        ctx.set_forward_prune(True)
    assert same_bits(ctx.embed_u8(imgs[:3], L.HEAD_POOLED, L.PREC_BF16), off)
