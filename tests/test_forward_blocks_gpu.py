"""GPU parity of the forward pass block by block (imageclust_amd/csrc/resnet.hip forward_batch through icl_embed_taps): every
bottleneck's output as the pass holds it, against the oracle's bottleneck (resnet_blocks.block_ref: icl_ref_conv2d with the engine's
rounding points) run on the ENGINE's own previous tap, so the bounds are per block and nothing accumulates.  What is under test is
what icl_model_load_blob prepares (folded weights, the fused [W3 * s3 | Wds * sds], shift3 + shiftds) and the kernel the pass picks
per layer, which the per-layer tests, with their own weights and a forced kernel, do not reach.

Tolerances, the project's for one layer (resnet_blocks.bounds): fp32 and bf16x3 1e-4 * max(1, max|ref|); bf16 maximum 1.2e-2 and
median 2e-3, both times max(1, max|ref|).  tests/test_forward_blocks_cpu.py shows which mistakes these bounds see and on which blob:
the synthetic blob's activations double per bottleneck, so a missing BatchNorm shift is visible there in stage 1 only; the variant
blob (a bias everywhere, gammas of both signs, another epsilon, activations of order 1) is what pins the loader's folding."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import resnet_blocks as RB

pytestmark = pytest.mark.gpu
PRECS = ["bf16", "fp32", "bf16x3"]


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def imgs(L):
    return RB.tap_images(L)


class Net:
    """A context with one blob loaded, its reference model and the taps already fetched, per (precision, conv option)."""

    def __init__(self, L, blob):
        self.L, self.ctx, self.model, self.cache = L, L.Context(0), RB.read_blob(blob), {}
        self.ctx.load_blob(blob)
        self.blocks = RB.blocks_of(self.model)

    def tap(self, imgs, t, prec, mode=None):
        L = self.L
        key = (t, prec, mode)
        if key not in self.cache:
            try:
                self.ctx.set_conv_options(L.CONV_P8_AUTO if mode is None else mode)
                self.cache[key] = self.ctx.embed_taps(imgs, t, {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16, "bf16x3": L.PREC_BF16X3}[prec])
            finally:
                self.ctx.set_conv_options(L.CONV_P8_AUTO)
        return self.cache[key]

    def check_stage(self, imgs, stage, prec, mode=None, what=""):
        for t in RB.taps_of_stage(stage):
            ref = RB.block_ref(self.blocks[t - 1], self.tap(imgs, t - 1, prec, mode), prec)
            RB.check_close(self.tap(imgs, t, prec, mode), ref, prec, "%sblock %d (stage %d)" % (what, t, stage))


@pytest.fixture(scope="module")
def net(L):
    n = Net(L, L.synthetic_blob(1))
    yield n
    n.ctx.close()


@pytest.fixture(scope="module")
def vnet(L):
    n = Net(L, RB.variant_blob(L.synthetic_blob(1)))
    yield n
    n.ctx.close()


def PREC(L, prec):
    return {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16, "bf16x3": L.PREC_BF16X3}[prec]


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
@pytest.mark.parametrize("prec", PRECS)
def test_every_block_matches_oracle(net, imgs, prec, stage):
    """Default options: what production runs (bf16: the fused stage-1 bottlenecks, conv_wr / conv_p8 / halo / igemm as AUTO picks)."""
    net.check_stage(imgs, stage, prec)


@pytest.mark.parametrize("stage", [2, 3, 4])
@pytest.mark.parametrize("mode", ["p8_all", "p8_off"])
def test_every_block_bf16_per_kernel_family(net, L, imgs, mode, stage):
    """bf16 with every eligible layer on conv_p8_kernel, and with none: the dual launch of each family inside the real pass."""
    net.check_stage(imgs, stage, "bf16", L.CONV_P8_ALL if mode == "p8_all" else L.CONV_P8_OFF, mode + " ")


@pytest.mark.parametrize("stage", [1, 2, 3, 4])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_every_block_matches_oracle_variant_blob(vnet, imgs, prec, stage):
    """The variant blob through icl_model_load_blob: pins the folding arithmetic (bias * scale into the shift, negative scales into the
    folded and fused weights, bn_eps) where the synthetic blob cannot.  All four stages: this blob is the one on which a missing
    downsample shift shows in every stage."""
    vnet.check_stage(imgs, stage, prec, what="variant ")


def test_loader_and_bottleneck56_pack_alike(vnet, imgs):
    """Stage 1, bf16: the pass on the loader's wfold / wfused / shift_fused and icl_bottleneck56 on the same block's raw weights with
    the folded scales and shifts run one kernel on one input, with weights from the same packer functions (resnet_pack.h): equal bits."""
    for t in (1, 2, 3):
        c = vnet.blocks[t - 1]
        ds = {} if len(c) == 3 else dict(wds=c[3].W.reshape(256, -1), bnds=(c[3].scale, c[3].shift))
        y = vnet.ctx.bottleneck56(vnet.tap(imgs, t - 1, "bf16"), c[0].W.reshape(64, -1), (c[0].scale, c[0].shift), c[1].W, (c[1].scale, c[1].shift),
                                  c[2].W.reshape(256, 64), (c[2].scale, c[2].shift), **ds)
        assert (t == 1) == bool(ds)
        assert np.array_equal(vnet.tap(imgs, t, "bf16"), y), "block %d: first difference at %s" % (
            t, tuple(int(v[0]) for v in np.nonzero(vnet.tap(imgs, t, "bf16") != y)))


@pytest.mark.parametrize("prec", PRECS)
def test_tap0_is_the_stem(net, vnet, L, imgs, prec):
    assert np.array_equal(net.tap(imgs, 0, prec), net.ctx.stem_pool(imgs, PREC(L, prec)))
    if prec != "bf16x3":  # the variant blob's conv0 (bias, negative scales) against the oracle's stem; bf16x3 runs the fp32 stem
        RB.check_close(vnet.tap(imgs, 0, prec), RB.stem_ref(vnet.model, imgs, prec), prec, "variant stem + maxpool")


@pytest.mark.parametrize("prec", PRECS)
def test_heads_follow_tap16(net, L, imgs, prec):
    """HEAD_POOLED is the mean over the 49 pixels of tap 16 (an fp32 sum of 49 non-negative terms: 49 * 2^-24 relative, bound 1e-5 *
    max|ref|); HEAD_DENSE0 is the oracle's icl_ref_fc of the engine's pooled vector within 1e-4 * max(1, max|ref|)."""
    pooled = net.ctx.embed_u8(imgs, L.HEAD_POOLED, PREC(L, prec))
    ref = net.tap(imgs, 16, prec).astype(np.float64).mean(axis=(1, 2))
    err = np.abs(pooled - ref).max()
    print("pooled %s: max err %.3e, bound %.3e" % (prec, err, 1e-5 * np.abs(ref).max()))
    assert err <= 1e-5 * np.abs(ref).max()
    dense = net.ctx.embed_u8(imgs, L.HEAD_DENSE0, PREC(L, prec))
    for b in range(len(imgs)):
        r = np.zeros(1000, np.float32)
        O.lib().icl_ref_fc(np.ascontiguousarray(pooled[b]), 2048, net.model.fcw, net.model.fcb, 1000, r)
        assert np.abs(dense[b] - r).max() <= 1e-4 * max(1.0, np.abs(r).max()), (prec, b)


@pytest.mark.parametrize("prec", PRECS)
def test_tapping_leaves_no_state(net, L, imgs, prec):
    p = PREC(L, prec)
    e0 = net.ctx.embed_u8(imgs, L.HEAD_POOLED, p)
    t16 = net.ctx.embed_taps(imgs, 16, p)
    for t in (5, 0, 14):
        net.ctx.embed_taps(imgs[:1], t, p)
    assert np.array_equal(net.ctx.embed_taps(imgs, 16, p), t16)
    assert np.array_equal(net.ctx.embed_u8(imgs, L.HEAD_POOLED, p), e0)


def test_taps_reject_bad_arguments(net, L, imgs):
    out = np.zeros(4, np.float32)
    for tap in (-1, 17):
        with pytest.raises(L.ICLError) as ei:
            L.check(net.ctx.h, net.ctx.L.icl_embed_taps(net.ctx.h, L.PREC_BF16, imgs.ctypes.data, 2, tap, out.ctypes.data))
        assert ei.value.code == L.ICL_ERR_ARG
    try:
        net.ctx.set_batch(1)
        with pytest.raises(L.ICLError) as ei:
            net.ctx.embed_taps(imgs, 0, L.PREC_BF16)
        assert ei.value.code == L.ICL_ERR_ARG
    finally:
        net.ctx.set_batch(256)
