"""GPU tests of bneck56_kernel's x-tile ring (imageclust_amd/csrc/resnet_fused.h): the kernel walks a strip in steps of 4
virtual rows, keeps the last three x tiles in LDS and takes conv3's side operand (identity: the residual, downsample block:
the branch's input) from those tiles instead of a second read of x from global memory.

1. The side operand alone: with W3 = 0 and shift3 = 0 the output must be bf16(max(x, 0)) (identity) or, with a 0/1 downsample
   matrix that copies channel o % 64, max(x[o % 64], 0) -- bit for bit: pixel, column shift, channel slice, no extra rounding.
2. Step-boundary shapes against the oracle's layer-by-layer bottleneck at test_fused_gpu's tolerances.
3. An image's output does not depend on the images beside it, bit for bit.

A workgroup owns one strip of 14 columns of a RUN of images: the batch is cut into min(B, CUs // strips) runs.  Small shapes give
every image its own run; the 1400-column shapes (100 strips: at most 4 runs on any device below 500 CUs) put several images
into one run, which is what makes image boundaries fall inside a tile and inside a quarter."""
import numpy as np
import pytest

from tests.test_fused_gpu import L, ctx, _bneck_ref, _bneck_weights, bf16_round  # noqa: F401  (L, ctx: fixtures)

pytestmark = pytest.mark.gpu

STEP = 4  # BN56_ROWS
WIDE = 1400

VARIANTS = pytest.mark.parametrize("ds", [False, True], ids=["identity", "downsample"])
_ids = lambda s: "b%d_h%d_w%d" % s


def _run(ctx, x, p, ds):
    return ctx.bottleneck56(x, p["w1"][:, :, 0, 0], p["bn1"], p["w2"], p["bn2"], p["w3"][:, :, 0, 0], p["bn3"],
                            p["wds"][:, :, 0, 0] if ds else None, p.get("bnds"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _side_only_weights(rng, cin, ds):
    """conv1 / conv2 random (they must not leak into the output), conv3 = 0 with shift 0; DS: a 0/1 matrix copying channel o % 64."""
    p = _bneck_weights(rng, cin, ds)
    p["w3"] = np.zeros_like(p["w3"])
    p["bn3"] = (np.ones(256, np.float32), np.zeros(256, np.float32))
    if ds:
        wds = np.zeros((256, 64, 1, 1), np.float32)
        wds[np.arange(256), np.arange(256) % 64, 0, 0] = 1.0
        p["wds"], p["bnds"] = wds, (np.ones(256, np.float32), np.zeros(256, np.float32))
    return p


SIDE_SHAPES = [(2, 56, 56), (3, 5, 29), (1, 1, 1), (4, 3, 15), (2, 7, 13), (5, 2, WIDE), (6, 1, WIDE)]


@VARIANTS
@pytest.mark.parametrize("shape", SIDE_SHAPES, ids=_ids)
def test_side_operand_is_exact(ctx, shape, ds):
    B, H, Wd = shape
    cin = 64 if ds else 256
    rng = np.random.default_rng(77 + B * 1000 + H * 10 + Wd + (1 if ds else 0))
    p = _side_only_weights(rng, cin, ds)
    x = rng.standard_normal((B, H, Wd, cin)).astype(np.float32)
    y = _run(ctx, x, p, ds)
    xb = np.maximum(bf16_round(x), 0) + np.float32(0.0)  # (+ 0.0: the kernel's ReLU turns -0 into +0)
    want = np.tile(xb, (1, 1, 1, 4)) if ds else xb  # DS: output channel o copies input channel o % 64
    bad = _bits(y) != _bits(want)
    print("side operand %s %s: %d of %d words differ" % ("ds" if ds else "id", shape, int(bad.sum()), bad.size))
    assert not bad.any(), np.argwhere(bad)[:8]


# B * (H + 1) in every residue class modulo the step (one image per run: the run is H + 1 rows; B * (H + 1) as a whole: 4, 5, 6, 7)
RESIDUE_SHAPES = [(1, 3, 20), (1, 4, 20), (3, 1, 20), (1, 6, 20), (2, 4, 30), (2, 5, 30), (2, 6, 30), (2, 7, 30)]
# several images per run: runs of 2 / 3 (B = 5), 3 (B = 6), 3 / 4 (B = 7) images; run lengths 6, 9 | 10, 15 | 6 | 12, 16 rows;
# H = 1, 2, 3: images shorter than a step, several image boundaries inside one tile and inside one quarter
RUN_SHAPES = [(5, 2, WIDE), (5, 4, WIDE), (6, 1, WIDE), (7, 3, WIDE), (9, 1, 700)]
SHORT_SHAPES = [(4, 1, 16), (3, 2, 16), (5, 3, 16)]
WIDTH_SHAPES = [(2, 5, 1), (2, 6, 13), (2, 4, 14), (3, 7, 15), (2, 9, 29)]


@VARIANTS
@pytest.mark.parametrize("shape", RESIDUE_SHAPES + RUN_SHAPES + SHORT_SHAPES + WIDTH_SHAPES, ids=_ids)
def test_step_boundaries_match_oracle(ctx, shape, ds):
    B, H, Wd = shape
    cin = 64 if ds else 256
    rng = np.random.default_rng(B * 100000 + H * 10000 + Wd + (1 if ds else 0))
    p = _bneck_weights(rng, cin, ds)
    x = rng.standard_normal((B, H, Wd, cin)).astype(np.float32)
    y = _run(ctx, x, p, ds)
    r = _bneck_ref(x, p, ds)
    assert y.shape == r.shape
    err = np.abs(y - r)
    scale = max(1.0, np.abs(r).max())
    print("bneck56 %s %s: max err %.3e median %.3e of scale %.3f" % ("ds" if ds else "id", shape, err.max(), np.median(err), scale))
    assert err.max() <= 1.2e-2 * scale, (err.max(), np.unravel_index(err.argmax(), err.shape))
    assert np.median(err) <= 2e-3 * scale


def test_residue_shapes_cover_every_class():
    assert {(B * (H + 1)) % STEP for B, H, _ in RESIDUE_SHAPES[:4]} == set(range(STEP))
    assert {(H + 1) % STEP for _, H, _ in RESIDUE_SHAPES[4:]} == set(range(STEP))


@VARIANTS
@pytest.mark.parametrize("shape", [(5, 6, 29), (5, 3, WIDE), (5, 2, WIDE)], ids=_ids)
def test_image_is_independent_of_its_neighbours(ctx, shape, ds):
    B, H, Wd = shape
    cin = 64 if ds else 256
    rng = np.random.default_rng(4242 + H * 10 + Wd + (1 if ds else 0))
    p = _bneck_weights(rng, cin, ds)
    x = rng.standard_normal((B, H, Wd, cin)).astype(np.float32)
    y = _run(ctx, x, p, ds)
    for b in range(B):
        alone = _run(ctx, x[b:b + 1], p, ds)
        assert np.array_equal(_bits(alone[0]), _bits(y[b])), "image %d of %d" % (b, B)
