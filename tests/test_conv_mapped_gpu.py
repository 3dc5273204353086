"""conv_wr_kernel's mapped form (conv_wr.h, MAP; prune_map.h) through icl_conv1x1_mapped: the 1x1 convolution of a pruned bottleneck
reads a compact [B][Ho][Ho][K] tensor and keeps its residual and its output at pixel (s oy, s ox) of full-size [B][H][H][Cout] tensors.
Reference: the unmapped kernel (conv2d_fused, which lands on conv_wr_kernel for these shapes) on the same compact input and the gathered
residual -- same kernel family, same k order, so the written pixels are equal BIT FOR BIT; inputs are Gaussian, rounded to bf16, so that
a changed summation order would show.  The output goes in filled with a negative sentinel (every result is behind a ReLU, so none can
equal it); each pixel that is not a multiple of s must come back holding the sentinel's bits.

Shapes, for K = 128 / Cout = 512 and K = 256 / Cout = 1024: one image whose compact pixels are exactly one 64-pixel tile; three images of
full height 10 (M = 75: an image boundary inside a tile and a ragged last tile); an odd full height (7 -> 4); s = 1 (the map is the
identity: equal to the unmapped kernel everywhere).  One case (K = 256) has more tiles than conv_select starts workers for, so that a
worker's second tile, the refilled LDS buffer and the residual requested one tile ahead run through the map: the smallest square image
with more than 64 * workers compact pixels (conv_exact.wr_rule restates the worker rule)."""
import numpy as np
import pytest

from tests import conv_exact as CE
from tests import resnet_blocks as RB

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-1536.0)  # bf16-exact, negative
LAYERS = [(128, 512), (256, 1024)]
SHAPES = [(1, 16, 2), (3, 10, 2), (2, 7, 2), (2, 9, 1)]  # (B, full height H, s)


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)
    yield c
    c.close()


def operands(B, H, s, K, cout):
    rng = np.random.default_rng([B, H, s, K, cout])
    Ho = (H - 1) // s + 1
    x = RB.bf16_round(rng.standard_normal((B, Ho, Ho, K), np.float32))
    w = RB.bf16_round((rng.standard_normal((cout, K), np.float32) / np.sqrt(K)).astype(np.float32))
    res = RB.bf16_round(rng.standard_normal((B, H, H, cout), np.float32))
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.standard_normal(cout).astype(np.float32)
    return x, w, scale, shift, res


def one_launch(ctx, call):
    before = ctx.conv_stats()
    y = call()
    after = ctx.conv_stats()
    assert tuple(a - b for a, b in zip(after, before)) == (1, 0), (before, after)  # conv_wr_kernel / conv_p8_kernel, nothing else
    return y


def check_mapped(ctx, L, B, H, s, K, cout):
    x, w, scale, shift, res = operands(B, H, s, K, cout)
    assert CE.route(CE.conv(B, x.shape[1], K, cout, 1, res=True), "bf16", L.CONV_P8_AUTO) == "conv_wr_kernel<%d>" % K
    want = one_launch(ctx, lambda: ctx.conv2d_fused(x, w.reshape(cout, K, 1, 1), scale, shift, 1, 0, np.ascontiguousarray(res[:, ::s, ::s]), True, L.PREC_BF16))
    full = np.full((B, H, H, cout), SENTINEL, np.float32)
    got = one_launch(ctx, lambda: ctx.conv1x1_mapped(x, w, scale, shift, full, s, res, True))
    assert want.min() >= 0 and (want > 0).mean() > 0.3
    sub = got[:, ::s, ::s]
    assert sub.shape == want.shape
    bad = np.nonzero(sub.view(np.uint32) != want.view(np.uint32))
    assert not len(bad[0]), "%d of %d written values differ, first at (b, oy, ox, c) = %s" % (len(bad[0]), want.size, tuple(int(v[0]) for v in bad))
    keep = np.ones((H, H), bool)
    keep[::s, ::s] = False
    rest = got[:, keep]
    assert rest.size == B * (H * H - want.shape[1] ** 2) * cout
    assert np.all(rest.view(np.uint32) == SENTINEL.view(np.uint32)), "%d values outside the map were written" % int((rest != SENTINEL).sum())


@pytest.mark.parametrize("K,cout", LAYERS)
@pytest.mark.parametrize("B,H,s", SHAPES)
def test_mapped_equals_unmapped_on_gathered_residual(ctx, L, B, H, s, K, cout):
    Ho = (H - 1) // s + 1
    M = B * Ho * Ho
    assert (B, H, s) != SHAPES[0] or M == 64
    assert (B, H, s) != SHAPES[1] or (M == 75 and (Ho * Ho) % 64 and M % 64)
    check_mapped(ctx, L, B, H, s, K, cout)


def test_mapped_second_tile_of_a_worker(ctx, L):
    K, cout = LAYERS[1]
    ncu = ctx.device_info()[1]
    pt, workers = CE.wr_rule(K, cout, ncu, 1 << 30)
    Ho = int(np.floor(np.sqrt(pt * workers))) + 1  # the smallest square image with more than pt * workers pixels
    M = Ho * Ho
    assert (Ho - 1) ** 2 <= pt * workers < M and CE.wr_rule(K, cout, ncu, M) == (pt, workers) and -(-M // pt) > workers
    check_mapped(ctx, L, 1, 2 * Ho - 1, 2, K, cout)


def test_mapped_rejects_other_shapes(ctx, L):
    x, w, scale, shift, res = operands(1, 4, 2, 64, 256)
    with pytest.raises(L.ICLError) as ei:
        ctx.conv1x1_mapped(x, w, scale, shift, np.zeros((1, 4, 4, 256), np.float32), 2, res)
    assert ei.value.code == L.ICL_ERR_UNSUPPORTED
