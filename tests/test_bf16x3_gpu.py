"""GPU tests of the split-bf16 embedding precision (ICL_PREC_BF16X3: every fp32 operand as hi + lo bf16, three bf16 MFMAs per
product, fp32 accumulate): every convolution kernel that serves it, the stem, the whole forward pass against the oracle at the fp32
parity bound (<= 1e-4 * max(1, |ref|_inf)), batch / slab / stream-lane invariance, the file path, groups and the argument checks."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_embed_gpu import SHAPES, ref_conv
from tests.test_fused_gpu import conv0_of_blob, ref_conv_hw, ref_maxpool

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    c.load_synthetic(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def blob(L):
    return L.synthetic_blob(1)


def err(y, r):
    return float(np.abs(y - r).max() / max(1.0, np.abs(r).max()))


def conv_both_kernels(ctx, L, x, w, sc, sh, stride, pad, res, relu, p8_expected):
    """The x3 convolution on the 128 x 128 kernels (P8_OFF) and on conv_p8_kernel (P8_ALL; the launch must take it when the shape is supported)."""
    out = []
    try:
        for mode in (L.CONV_P8_OFF, L.CONV_P8_ALL):
            ctx.set_conv_options(mode)
            n8 = ctx.conv_stats()[0]
            out.append(ctx.conv2d_fused(x, w, sc, sh, stride, pad, res, relu, L.PREC_BF16X3))
            if mode == L.CONV_P8_OFF:
                assert ctx.conv_stats()[0] == n8
            else:
                assert ctx.conv_stats()[0] == n8 + (1 if p8_expected else 0), "conv_p8_kernel launches"
    finally:
        ctx.set_conv_options(L.CONV_P8_AUTO)
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d-%d_k%d_s%d_h%d" % (s[0], s[1], s[2], s[3], s[5]))
def test_conv_layer_bf16x3_every_resnet_shape(ctx, L, shape):
    cin, cout, k, stride, pad, H = shape
    rng = np.random.default_rng(cin * 7 + cout + k + 3)
    B = 2 if H <= 28 else 1
    x = rng.standard_normal((B, H, H, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    Ho = (H + 2 * pad - k) // stride + 1
    res = rng.standard_normal((B, Ho, Ho, cout)).astype(np.float32)
    for r_in, relu in ((None, False), (res, True)):
        r = ref_conv(x, w, sc, sh, stride, pad, r_in, relu)
        for y in conv_both_kernels(ctx, L, x, w, sc, sh, stride, pad, r_in, relu, cout % 128 == 0):
            assert y.shape == r.shape
            assert err(y, r) <= 1e-4, err(y, r)


@pytest.mark.parametrize("B,H,cin,cout,k,stride,pad", [(1, 7, 128, 128, 3, 1, 1), (3, 7, 64, 64, 3, 1, 1), (2, 9, 256, 128, 3, 1, 1),
                                                       (3, 13, 192, 256, 1, 1, 0), (2, 11, 128, 128, 1, 2, 0), (1, 28, 192, 128, 3, 1, 1),
                                                       (3, 5, 512, 256, 3, 1, 1), (2, 10, 64, 128, 3, 2, 1)])
def test_conv_bf16x3_ragged_and_odd_shapes(ctx, L, B, H, cin, cout, k, stride, pad):
    """Partial tiles (M far from a multiple of 128 / 256 / 512), B = 1-3, widths that are no power of two, tiles that span images,
    Cout = 64, strided 3x3; with a residual and ReLU.  (The fused downsample form is exercised by the forward-pass tests below.)"""
    rng = np.random.default_rng(B * 1000 + H * 10 + k)
    x = rng.standard_normal((B, H, H, cin)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    Ho = (H + 2 * pad - k) // stride + 1
    res = rng.standard_normal((B, Ho, Ho, cout)).astype(np.float32)
    r = ref_conv(x, w, sc, sh, stride, pad, res, True)
    for y in conv_both_kernels(ctx, L, x, w, sc, sh, stride, pad, res, True, cout % 128 == 0):
        assert err(y, r) <= 1e-4, err(y, r)


@pytest.mark.parametrize("B", [1, 3])
def test_stem_pool_bf16x3_matches_oracle(ctx, L, B):
    blob = L.synthetic_blob(1)
    w, sc, sh = conv0_of_blob(blob)
    imgs = np.concatenate([L.synth_images(20250217, 3, B - 1, L.SYNTH_STRUCTURED), L.synth_images(7, 11, 1, L.SYNTH_NOISE)]) if B > 1 \
        else L.synth_images(7, 11, 1, L.SYNTH_NOISE)
    x = imgs.astype(np.float32) * np.float32(1.0 / 255.0)
    r = ref_maxpool(ref_conv_hw(x, w, sc, sh, 2, 3, True))
    y = ctx.stem_pool(imgs, L.PREC_BF16X3)
    assert y.shape == (B, 56, 56, 64)
    assert err(y, r) <= 1e-4, err(y, r)


def test_full_forward_bf16x3_matches_oracle_and_golden(ctx, L, blob):
    g = np.load(os.path.join(GOLD, "resnet50_synth_seed1.npz"))
    imgs = L.synth_images(int(g["img_seed"]), 0, 4, L.SYNTH_STRUCTURED)
    pooled = ctx.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16X3)
    dense = ctx.embed_u8(imgs, L.HEAD_DENSE0, L.PREC_BF16X3)
    assert pooled.shape == (4, 2048) and dense.shape == (4, 1000)
    worst = 0.0
    for i in range(4):
        rp, rd = O.resnet50_forward(blob, imgs[i])
        worst = max(worst, err(pooled[i], rp), err(dense[i], rd))
    worst_gold = max(err(pooled, g["pooled"]), err(dense, g["dense"]))
    print("bf16x3 max error vs oracle %.3g, vs golden %.3g (CPU emulation: ~7e-6)" % (worst, worst_gold))
    assert worst <= 1e-4 and worst_gold <= 1e-4


def test_full_forward_bf16x3_on_both_kernel_families(ctx, L, blob):
    """Every layer on the 128 x 128 kernels (P8_OFF: the fused downsample on conv_igemm_kernel's DUAL form) and every supported layer on
    conv_p8_kernel (P8_ALL: its DUAL form): both within the bound, at a ragged batch size."""
    imgs = L.synth_images(20250217, 40, 3, L.SYNTH_STRUCTURED)
    refs = [O.resnet50_forward(blob, imgs[i])[0] for i in range(3)]
    try:
        for mode in (L.CONV_P8_OFF, L.CONV_P8_ALL):
            ctx.set_conv_options(mode)
            n8 = ctx.conv_stats()[0]
            e = ctx.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16X3)
            assert (ctx.conv_stats()[0] - n8 >= 20) == (mode == L.CONV_P8_ALL)
            for i in range(3):
                assert err(e[i], refs[i]) <= 1e-4, (mode, i, err(e[i], refs[i]))
    finally:
        ctx.set_conv_options(L.CONV_P8_AUTO)


def test_bf16x3_batch_slab_and_lane_invariance(ctx, L):
    """One image embedded alone, inside a batch of 256, in the second batch (the second stream lane) and in the second 4096-image slab of
    icl_embed_u8: bit-identical rows."""
    probe = L.synth_images(31337, 0, 1, L.SYNTH_STRUCTURED)
    alone = ctx.embed_u8(probe, L.HEAD_POOLED, L.PREC_BF16X3)[0]
    n = 4096 + 40
    imgs = L.synth_images(5, 0, n, L.SYNTH_STRUCTURED)
    pos = [5, 256 + 17, 4096 + 3]
    for p in pos:
        imgs[p] = probe[0]
    out = ctx.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16X3)
    assert np.isfinite(out).all()
    for p in pos:
        assert np.array_equal(out[p], alone), p
    again = ctx.embed_u8(imgs[:300], L.HEAD_POOLED, L.PREC_BF16X3)
    assert np.array_equal(again, out[:300])


def test_bf16x3_file_path_equals_embed_u8(ctx, L, tmp_path):
    img = L.synth_images(20250217, 9, 1, L.SYNTH_STRUCTURED)[0]
    p = tmp_path / "img.ppm"
    p.write_bytes(b"P6\n224 224\n255\n" + img.tobytes())
    try:
        ctx.set_file_options(L.PREC_BF16X3, 0, 256)
        e = ctx.embed_file(str(p), L.HEAD_DENSE0)
    finally:
        ctx.set_file_options(L.PREC_FP32, 2000, 256)
    assert np.array_equal(e, ctx.embed_u8(img[None], L.HEAD_DENSE0, L.PREC_BF16X3)[0])


def test_bf16x3_group_equals_one_context(ctx, L):
    imgs = L.synth_images(77, 0, 7, L.SYNTH_STRUCTURED)
    g = L.Group([0, 0, 0])
    try:
        g.load_synthetic(1)
        e = g.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16X3)
    finally:
        g.close()
    assert np.array_equal(e, ctx.embed_u8(imgs, L.HEAD_POOLED, L.PREC_BF16X3))


@pytest.mark.parametrize("prec", [3, -1])
def test_other_prec_values_still_rejected(ctx, L, prec):
    img = L.synth_images(1, 0, 1, L.SYNTH_STRUCTURED)
    x = np.zeros((1, 4, 4, 64), np.float32)
    w = np.zeros((64, 64, 1, 1), np.float32)
    one, zero = np.ones(64, np.float32), np.zeros(64, np.float32)
    for call in (lambda: ctx.embed_u8(img, L.HEAD_POOLED, prec), lambda: ctx.stem_pool(img, prec),
                 lambda: ctx.conv2d_fused(x, w, one, zero, 1, 0, None, False, prec), lambda: ctx.set_file_options(prec, 0, 16)):
        with pytest.raises(L.ICLError) as ei:
            call()
        assert ei.value.code == L.ICL_ERR_ARG
