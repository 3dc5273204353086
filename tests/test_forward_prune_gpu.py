"""The bf16 forward pass with and without its dead pixels (icl_set_forward_prune; resnet.hip forward_batch, prune_map.h): block 0 of
stages 2, 3 and 4 reads the tensor in front of it at the pixels (2 oy, 2 ox) only, so the bottleneck in front of it may run its 3x3
convolution at stride 2 and its last 1x1 convolution over a quarter of the pixels.  Every value that is still computed comes from the same
kernel in the same k order: everything below is equality of bits, on the synthetic blob.

  * both heads of embed_u8, option on against off: 1 image, 3 images, and 7 images at a batch of 3 (two passes in flight, a ragged last batch);
  * one image alone against its row of a batch;
  * icl_embed_taps at taps 4, 8, 14 (the tensor behind a pruned block's reader) and 16;
  * taps 3, 7 and 13 -- the very tensors a longer pass prunes -- come back WHOLE with the option on: a tap never prunes what it returns;
  * the launch counters: the option moves no launch between the kernel families (every pruned launch is still counted under
    conv_p8_kernel / conv_wr_kernel), and icl_forward_prune_stats counts the blocks the records say (stages 2 and 3 of this model; stage 1
    runs as fused bottlenecks), none in fp32 / bf16x3, none where the unpruned layers would take other kernels (ICL_CONV_P8_OFF), and not
    stage 3's under ICL_CONV_SPLIT (its quartered 3x3 layer would take the split form, another summation order);
  * 9 images at a batch of 4 (batches of 4, 4 and 1 on two lanes: the plan of the full batch and the plan of the remainder) in every
    precision and both heads: each row equals that image's embedding in a call of its own, and the launch counters move by what
    conv_exact.route says of the model's records."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.load_blob(L.synthetic_blob(1))
    yield c
    c.close()


@pytest.fixture(scope="module")
def imgs(L):
    return np.concatenate([L.synth_images(7, 11, 4, L.SYNTH_NOISE), L.synth_images(20250217, 3, 3, L.SYNTH_STRUCTURED)])


def both(ctx, call, other=None):
    """call() with the option off, then on -> (off, on, launch counters off, launch counters on, pruned blocks off, pruned blocks on).
    The pixels a pruned pass does not write keep what the pass before it left there; `other` (images) is embedded unpruned in between, so
    that those are values of OTHER images: a reader of a dead pixel would not find the right value there by accident."""
    out = []
    try:
        for on in (False, True):
            if on and other is not None:
                ctx.set_forward_prune(False)
                ctx.embed_u8(other, 2048, 1)
            ctx.set_forward_prune(on)
            s0, p0 = ctx.conv_stats(), ctx.forward_prune_stats()
            y = call()
            s1, p1 = ctx.conv_stats(), ctx.forward_prune_stats()
            out.append((y, tuple(a - b for a, b in zip(s1, s0)), p1 - p0))
    finally:
        ctx.set_forward_prune(True)
    (y0, s0, p0), (y1, s1, p1) = out
    return y0, y1, s0, s1, p0, p1


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("n,batch", [(1, 256), (3, 256), (7, 3)])
def test_embeddings_are_bit_identical(ctx, L, imgs, n, batch):
    try:
        ctx.set_batch(batch)
        nbatches = -(-n // batch)
        for head in (L.HEAD_POOLED, L.HEAD_DENSE0):
            off, on, s0, s1, p0, p1 = both(ctx, lambda: ctx.embed_u8(imgs[:n], head, L.PREC_BF16), imgs[::-1])
            assert same_bits(off, on), "head %d: %d values differ" % (head, int((off != on).sum()))
            assert np.isfinite(on).all() and on.std() > 0
            assert s0 == s1 and s0[0] > 0, (s0, s1)  # no launch changed its kernel family
            assert (p0, p1) == (0, 2 * nbatches)     # stages 2 and 3, once per batch
    finally:
        ctx.set_batch(256)


def test_one_image_alone_equals_its_row_of_a_batch(ctx, L, imgs):
    ctx.set_forward_prune(True)
    e = ctx.embed_u8(imgs[:5], L.HEAD_POOLED, L.PREC_BF16)
    for i in (0, 4):
        assert same_bits(ctx.embed_u8(imgs[i:i + 1], L.HEAD_POOLED, L.PREC_BF16)[0], e[i])


@pytest.mark.parametrize("tap,pruned", [(4, 0), (8, 1), (14, 2), (16, 2)])
def test_taps_behind_a_pruned_block(ctx, L, imgs, tap, pruned):
    off, on, s0, s1, p0, p1 = both(ctx, lambda: ctx.embed_taps(imgs[:3], tap, L.PREC_BF16), imgs[::-1])
    assert same_bits(off, on), "tap %d: %d values differ" % (tap, int((off != on).sum()))
    assert s0 == s1 and (p0, p1) == (0, pruned)


@pytest.mark.parametrize("tap,pruned", [(3, 0), (7, 0), (13, 1)])
def test_a_tapped_tensor_is_whole(ctx, L, imgs, tap, pruned):
    """The pass that ends at the block a longer pass would prune: every pixel of its tensor, odd ones included."""
    off, on, s0, s1, p0, p1 = both(ctx, lambda: ctx.embed_taps(imgs[:3], tap, L.PREC_BF16), imgs[::-1])
    assert same_bits(off, on), "tap %d: %d values differ" % (tap, int((off != on).sum()))
    assert (off[:, 1::2, 1::2] != 0).any()
    assert s0 == s1 and (p0, p1) == (0, pruned)


def test_a_long_pass_before_a_tap_leaves_no_stale_pixels(ctx, L, imgs):
    """A pruned pass leaves the odd pixels of two buffers unwritten; the next tapped pass must overwrite all of its tensor."""
    ctx.set_forward_prune(False)
    want = ctx.embed_taps(imgs[:2], 13, L.PREC_BF16)
    ctx.set_forward_prune(True)
    ctx.embed_u8(imgs[2:4], L.HEAD_POOLED, L.PREC_BF16)
    assert same_bits(ctx.embed_taps(imgs[:2], 13, L.PREC_BF16), want)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_other_precisions_are_not_pruned(ctx, L, imgs, prec):
    p = {"fp32": L.PREC_FP32, "bf16x3": L.PREC_BF16X3}[prec]
    off, on, s0, s1, p0, p1 = both(ctx, lambda: ctx.embed_u8(imgs[:2], L.HEAD_POOLED, p))
    assert same_bits(off, on) and s0 == s1 and (p0, p1) == (0, 0)


@pytest.mark.parametrize("mode,pruned", [("off", 0), ("all", 2), ("split", 1)])
def test_only_where_both_forms_take_the_same_kernels(ctx, L, imgs, mode, pruned):
    try:
        ctx.set_conv_options({"off": L.CONV_P8_OFF, "all": L.CONV_P8_ALL, "split": L.CONV_P8_AUTO | L.CONV_SPLIT}[mode])
        k0 = ctx.conv_split_launches()
        off, on, s0, s1, p0, p1 = both(ctx, lambda: ctx.embed_u8(imgs[:2], L.HEAD_POOLED, L.PREC_BF16))
        assert same_bits(off, on) and s0 == s1 and (p0, p1) == (0, pruned)
        k = ctx.conv_split_launches() - k0
        assert k % 2 == 0 and (k > 0) == (mode == "split")  # the same number of split launches with the option on and off
    finally:
        ctx.set_conv_options(L.CONV_P8_AUTO)


@pytest.fixture(scope="module")
def nine(L):
    return np.concatenate([L.synth_images(7, 40, 5, L.SYNTH_NOISE), L.synth_images(20250217, 9, 4, L.SYNTH_STRUCTURED)])


def launches_of_a_pass(prec, B):
    """The convolutions one forward pass of B images hands to the selector (conv_select.h), from the model's records: in bf16
    stage 1 runs in bneck56_kernel; the c3 of a block 0 is ONE launch over K = [mid | cin of the downsample branch]; a pruned block's two
    launches stay in the families of the unpruned layers, whose shapes stand here."""
    from tests import conv_exact as X
    from tests import resnet_blocks as RB

    recs, out = RB.topology(), []
    for i, r in enumerate(recs):
        if r.role in (0, 4) or (prec == "bf16" and r.stage == 1):
            continue
        cin = r.cin + (recs[i + 1].cin if r.role == 3 and r.block == 0 else 0)
        out.append(X.conv(B, r.hin, cin, r.cout, r.k, r.stride, res=r.role == 3 and r.block > 0))
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x3"])
def test_ragged_batches_on_two_lanes_take_the_right_plans(ctx, L, nine, prec):
    """9 images at a batch of 4: batches of 4, 4 and 1 over two lanes -- a plan for the full batch and one for the remainder.  Every row is
    the embedding that image has in a call of its own, bit for bit, in both heads; the launch counters move by what conv_exact.route says
    of the model's records for the three batches, and 2 blocks per batch are pruned in bf16, none otherwise."""
    from tests import conv_exact as X

    p = {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16, "bf16x3": L.PREC_BF16X3}[prec]
    want = np.zeros(3, np.int64)
    for B in (4, 4, 1):
        for c in launches_of_a_pass(prec, B):
            want += X.counters_of(X.route(c, prec, 1))
    try:
        ctx.set_batch(4)
        for head in (L.HEAD_POOLED, L.HEAD_DENSE0):
            s0, k0, p0 = ctx.conv_stats(), ctx.conv_split_launches(), ctx.forward_prune_stats()
            e = ctx.embed_u8(nine, head, p)
            s1, k1, p1 = ctx.conv_stats(), ctx.conv_split_launches(), ctx.forward_prune_stats()
            print("%s head %d: conv_stats +%s, split +%d, pruned +%d; route says %s" % (prec, head, tuple(a - b for a, b in zip(s1, s0)), k1 - k0, p1 - p0, tuple(want)))
            assert (s1[0] - s0[0], s1[1] - s0[1], k1 - k0) == tuple(want)
            assert p1 - p0 == (6 if prec == "bf16" else 0)
            for i in range(len(nine)):
                assert same_bits(ctx.embed_u8(nine[i:i + 1], head, p)[0], e[i]), "%s head %d: image %d differs from its embedding alone" % (prec, head, i)
    finally:
        ctx.set_batch(256)
