"""Helpers of the per-block parity tests of the forward pass (no GPU, no test in here): an ICLW blob reader that folds BatchNorm as
the engine's loader does, the oracle's bottleneck with the engine's rounding points (block_ref), a float64 reference of the
dual-operand convolution (dual_ref), the test inputs both the GPU tests and their CPU "teeth" test use, and the tolerance check.

Everything is built from oracle/resnet_ref.c's icl_ref_conv2d / icl_ref_maxpool3x3s2 and numpy; nothing here loads the engine.

Known mistakes.  block_ref and dual_ref take `mistake=`: the name of one deliberate error, applied inside the same code that forms the
reference, so that tests/test_forward_blocks_cpu.py can show that the GPU tests' bounds would see it (or, for "t2_unrounded", that
they cannot).  block_ref: "ds_scale_s3" (downsample weights scaled by bn3's scale), "no_shiftds" (shift3 without the downsample
shift), "t2_unrounded" (bf16: t2 kept in fp32), "wrap_column" (the 3x3 layer's last output column reads, for its right-hand taps,
the pixel that follows in memory -- column 0 of the next row -- instead of zero padding).  dual_ref: "gather_row_plus1" (second
operand gathered at (oy * stride2 + 1, ox * stride2)), "odd_h2" (the second operand's pixel (b, oy, ox) taken apart with H2 //
stride2 rows and columns per image instead of Ho: right for an even H2, wrong for an odd one), "drop_last64" (the last 64 channels
of x2 left out), "zero_ragged_rows" (output rows from 256 * (M // 256) on left at zero)."""
import collections

import numpy as np

from oracle import oracle as O

Rec = collections.namedtuple("Rec", "cin cout k stride pad hin hout role stage block")
Layer = collections.namedtuple("Layer", "rec W scale shift")  # W: OIHW fp32, scale / shift: the folded BatchNorm (+ bias), fp32
Model = collections.namedtuple("Model", "layers raw fcw fcb eps has_bias")
HEADER_BYTES = 80
NBLOCKS = (3, 4, 6, 3)

# (B, Ho, H2, stride2, Cin, Cin2, Cout) of the dual-operand tests: the three ResNet shapes (stage 4 with M = 147: one ragged tile), K = 128
# (conv_p8_kernel's prologue and peeled K-tiles only, operand switch at K-tile 1, odd H2, tiles that span images), a switch at an odd
# K-tile, stride2 = 1 with three channel tiles, and two shapes on the 512 x 128 layout (Cout = 128 * odd) no model layer selects
DUAL_SHAPES = [(3, 7, 14, 2, 512, 1024, 2048), (2, 14, 28, 2, 256, 512, 1024), (1, 28, 56, 2, 128, 256, 512), (5, 9, 17, 2, 64, 64, 256),
               (3, 7, 13, 2, 192, 64, 256), (2, 12, 12, 1, 128, 256, 768), (4, 11, 21, 2, 128, 128, 384), (2, 23, 45, 2, 64, 192, 128)]


def bf16_round(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.view(np.float32)


# ---- the blob ---------------------------------------------------------------------------------------------------------------
def topology():
    """The 53 convolutions in canonical order, from the oracle's icl_ref_resnet50_topology."""
    buf = np.zeros((64, 10), np.int32)
    n = O.lib().icl_ref_resnet50_topology(buf.ctypes.data)
    return [Rec(*(int(v) for v in row)) for row in buf[:n]]


def fold(raw, eps):
    """BatchNorm folded to y = x * scale + shift in float64, the conv bias folded into the shift, each rounded to fp32 once -- the
    arithmetic of icl_model_load_blob."""
    s = raw["gamma"].astype(np.float64) / np.sqrt(raw["var"].astype(np.float64) + np.float64(eps))
    sh = raw["beta"].astype(np.float64) - raw["mean"].astype(np.float64) * s
    if raw["bias"] is not None:
        sh = sh + raw["bias"].astype(np.float64) * s
    return s.astype(np.float32), sh.astype(np.float32)


def read_blob(blob):
    """An ICLW blob (include/icl_model_format.h) -> Model: per convolution Layer(rec, W_oihw, scale, shift) and the raw tensors."""
    b = np.frombuffer(blob, np.uint8)
    eps = np.frombuffer(b[8:12].tobytes(), np.float32)[0]
    has_bias = b[16:80].copy()
    p = np.frombuffer(b[HEADER_BYTES:].tobytes(), np.float32)
    pos, layers, raws = 0, [], []

    def take(n):
        nonlocal pos
        pos += n
        return p[pos - n:pos]

    for i, rec in enumerate(topology()):
        raw = {"W": take(rec.cout * rec.cin * rec.k * rec.k).reshape(rec.cout, rec.cin, rec.k, rec.k).copy()}
        raw["bias"] = take(rec.cout).copy() if has_bias[i] else None
        for name in ("gamma", "beta", "mean", "var"):
            raw[name] = take(rec.cout).copy()
        sc, sh = fold(raw, eps)
        layers.append(Layer(rec, raw["W"], sc, sh))
        raws.append(raw)
    fcw = take(1000 * 2048).reshape(1000, 2048).copy()
    fcb = take(1000).copy()
    assert pos == p.size, "blob has %d floats, the topology accounts for %d" % (p.size, pos)
    return Model(layers, raws, fcw, fcb, float(eps), has_bias)


def write_blob(raws, fcw, fcb, eps):
    """Raw tensors -> ICLW blob (uint8 array); a layer carries a bias where its raw["bias"] is not None."""
    head = np.zeros(HEADER_BYTES, np.uint8)
    head[0:16] = np.frombuffer(np.array([0x574C4349, 1], np.uint32).tobytes() + np.float32(eps).tobytes() + np.uint32(len(raws)).tobytes(), np.uint8)
    parts = []
    for i, raw in enumerate(raws):
        head[16 + i] = raw["bias"] is not None
        parts.append(raw["W"].ravel())
        if raw["bias"] is not None:
            parts.append(raw["bias"])
        parts += [raw[name] for name in ("gamma", "beta", "mean", "var")]
    payload = np.concatenate(parts + [fcw.ravel(), fcb]).astype(np.float32)
    return np.concatenate([head, np.frombuffer(payload.tobytes(), np.uint8)])


def variant_blob(blob):
    """The blob again with what the synthetic one lacks: a bias ~ N(0, 0.1) on every convolution, gamma of either sign
    (+-U(0.5, 1.5)) and bn_eps = 1e-3.  Its activations also stay of order 1 through all 16 bottlenecks (the running variance of
    every c3 is multiplied by 16 and of every downsample convolution by 2, i.e. their scales divided by 4 and 1.41): in the
    synthetic blob they double per bottleneck, up to 2e4, and a tolerance relative to max|ref| then cannot see a BatchNorm shift of
    0.5 beyond stage 1."""
    m = read_blob(blob)
    rng = np.random.default_rng(20250218)
    raws = []
    for raw, layer in zip(m.raw, m.layers):
        c = raw["gamma"].size
        raw = dict(raw, bias=(0.1 * rng.standard_normal(c)).astype(np.float32),
                   gamma=(rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32))
        if layer.rec.role >= 3:
            raw["var"] = (raw["var"] * (16 if layer.rec.role == 3 else 2)).astype(np.float32)
        raws.append(raw)
    return write_blob(raws, m.fcw, m.fcb, 1e-3)


def blocks_of(model):
    """The 16 bottlenecks: [c1, c2, c3] or, for block 0 of a stage, [c1, c2, c3, ds]."""
    out, i = [], 1
    while i < len(model.layers):
        n = 4 if model.layers[i].rec.block == 0 else 3
        out.append(model.layers[i:i + n])
        i += n
    return out


def stage_of_tap(tap):
    """Stage (1..4) of bottleneck `tap` (1..16)."""
    return 1 + sum(tap > e for e in np.cumsum(NBLOCKS)[:3])


def taps_of_stage(stage):
    lo = int(sum(NBLOCKS[:stage - 1]))
    return list(range(lo + 1, lo + NBLOCKS[stage - 1] + 1))


# ---- the oracle's layers on NHWC batches ----------------------------------------------------------------------------------------
def ref_conv(x_nhwc, w, scale, shift, stride, pad, relu, wrap=False):
    """conv + folded BatchNorm (+ ReLU) by icl_ref_conv2d on [B][H][W][C].  wrap (mistake "wrap_column", 3x3 / pad 1 only): the padding
    column right of the image holds the pixel that follows in memory, column 0 of the next row (of the next image after the last row)."""
    B, H, Wd, Cin = x_nhwc.shape
    Cout, _, k, _ = w.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (Wd + 2 * pad - k) // stride + 1
    if wrap:
        assert k == 3 and pad == 1 and stride == 1
        flat = np.concatenate([x_nhwc.reshape(B * H * Wd, Cin), np.zeros((1, Cin), np.float32)])
        xp = np.zeros((B, H + 2, Wd + 2, Cin), np.float32)
        xp[:, 1:H + 1, 1:Wd + 1] = x_nhwc
        xp[:, 1:H + 1, Wd + 1] = flat[(np.arange(B * H) + 1) * Wd].reshape(B, H, Cin)
        x_nhwc, H, Wd, pad = xp, H + 2, Wd + 2, 0
    out = np.empty((B, Ho, Wo, Cout), np.float32)
    w = np.ascontiguousarray(w, np.float32)
    for b in range(B):
        x = np.ascontiguousarray(x_nhwc[b].transpose(2, 0, 1), np.float32)
        y = np.zeros((Cout, Ho, Wo), np.float32)
        O.lib().icl_ref_conv2d(x, Cin, H, Wd, w, None, Cout, k, stride, pad, y, Ho, Wo)
        y = (y * scale[:, None, None] + shift[:, None, None]).transpose(1, 2, 0)
        out[b] = np.maximum(y, 0) if relu else y
    return out


def ref_maxpool(y_nhwc):
    B, H, Wd, Cc = y_nhwc.shape
    out = np.empty((B, H // 2, Wd // 2, Cc), np.float32)
    for b in range(B):
        x = np.ascontiguousarray(y_nhwc[b].transpose(2, 0, 1))
        o = np.zeros((Cc, H // 2, Wd // 2), np.float32)
        O.lib().icl_ref_maxpool3x3s2(x, Cc, H, Wd, o, H // 2, Wd // 2)
        out[b] = o.transpose(1, 2, 0)
    return out


def stem_ref(model, imgs, prec="fp32"):
    """The oracle's conv0 -> BN -> ReLU -> maxpool on the RGB / 255 image; bf16: on the bf16-rounded image with the scale folded into
    the weights before they are rounded, as the engine's bf16 stem takes them."""
    L0 = model.layers[0]
    x = imgs.reshape(-1, 224, 224, 3).astype(np.float32) * np.float32(1.0 / 255.0)
    if prec == "bf16":
        return ref_maxpool(ref_conv(bf16_round(x), bf16_round(L0.W * L0.scale[:, None, None, None]), np.ones(64, np.float32), L0.shift, 2, 3, True))
    return ref_maxpool(ref_conv(x, L0.W, L0.scale, L0.shift, 2, 3, True))


def block_ref(layers, x_nhwc, prec, mistake=None):
    """One bottleneck (layers: [c1, c2, c3] or [c1, c2, c3, ds]) on x by the oracle's convolution, with the engine's rounding points.
    prec "fp32" / "bf16x3": no rounding; block 0 is the sum of the two branches, each with its own BatchNorm.
    prec "bf16": x, the weights, t1 and t2 rounded to bf16.  Stage 1 (one fused launch per bottleneck): every scale folded into the
    weights before they are rounded.  Stages 2-4: c1 / c2 (and the c3 of an identity block) with bf16(W) and the fp32 scale in the
    epilogue; block 0's c3 + ds as bf16([W3 * s3 | Wds * sds]) with shift3 + shiftds; identity blocks add the bf16 residual."""
    assert prec in ("fp32", "bf16", "bf16x3") and mistake in (None, "ds_scale_s3", "no_shiftds", "t2_unrounded", "wrap_column")
    c1, c2, c3 = layers[:3]
    ds = layers[3] if len(layers) == 4 else None
    bf = prec == "bf16"
    r = bf16_round if bf else (lambda a: np.asarray(a, np.float32))
    fold_w = lambda L, sc: (r(L.W * sc[:, None, None, None]), np.ones(L.rec.cout, np.float32))

    def conv(L, xin, relu, wrap=False):
        w, sc = fold_w(L, L.scale) if bf and L.rec.stage == 1 else (r(L.W), L.scale)
        return ref_conv(xin, w, sc, L.shift, L.rec.stride, L.rec.pad, relu, wrap)

    x = r(x_nhwc)
    t1 = r(conv(c1, x, True))
    t2 = conv(c2, t1, True, wrap=mistake == "wrap_column")
    if mistake != "t2_unrounded":
        t2 = r(t2)
    if ds is None:
        return np.maximum(conv(c3, t2, False) + x, 0)
    sds = c3.scale if mistake == "ds_scale_s3" else ds.scale
    w3, s3 = fold_w(c3, c3.scale) if bf else (c3.W, c3.scale)
    wd, sd = fold_w(ds, sds) if bf else (ds.W, sds)
    sh = c3.shift if mistake == "no_shiftds" else c3.shift + ds.shift
    y = ref_conv(t2, w3, s3, sh, 1, 0, False) + ref_conv(x, wd, sd, np.zeros_like(sh), ds.rec.stride, 0, False)
    return np.maximum(y, 0)


def chain_ref(model, x0, first=1, last=16, prec="fp32"):
    """block_ref chained from tap first - 1 (x0) through bottleneck `last` -> {tap: tensor}."""
    bl, taps, x = blocks_of(model), {}, x0
    for t in range(first, last + 1):
        x = taps[t] = block_ref(bl[t - 1], x, prec)
    return taps


# ---- the dual-operand convolution -------------------------------------------------------------------------------------------------
def dual_case(shape):
    """Inputs of one dual-operand test: random normal activations, He-scaled weights (fan-in Cin + Cin2), a BatchNorm-like scale and shift."""
    B, Ho, H2, s2, Cin, Cin2, Cout = shape
    rng = np.random.default_rng(list(shape))
    sd = np.sqrt(2.0 / (Cin + Cin2))
    return dict(x=rng.standard_normal((B, Ho, Ho, Cin)).astype(np.float32), w1=(sd * rng.standard_normal((Cout, Cin))).astype(np.float32),
                x2=rng.standard_normal((B, H2, H2, Cin2)).astype(np.float32), w2=(sd * rng.standard_normal((Cout, Cin2))).astype(np.float32),
                stride2=s2, scale=rng.uniform(0.5, 1.5, Cout).astype(np.float32), shift=(0.1 * rng.standard_normal(Cout)).astype(np.float32))


def dual_ref(x, w1, x2, w2, stride2, scale, shift, relu=True, mistake=None):
    """relu?((x . w1 + x2[:, ::stride2, ::stride2] . w2) * scale + shift) in float64 -> [B][Ho][Ho][Cout]."""
    assert mistake in (None, "gather_row_plus1", "odd_h2", "drop_last64", "zero_ragged_rows")
    B, Ho, _, Cin = x.shape
    _, H2, _, Cin2 = x2.shape
    M, Cout = B * Ho * Ho, w1.shape[0]
    f = lambda a: np.asarray(a, np.float64)
    if mistake in ("gather_row_plus1", "odd_h2"):  # the gather on the flat tensor, as a kernel addresses it; pixels past the end read zero
        m = np.arange(M)
        hq = H2 // stride2 if mistake == "odd_h2" else Ho
        b, oy, ox = m // (hq * hq), (m // hq) % hq, m % hq
        idx = (b * H2 + oy * stride2 + (mistake == "gather_row_plus1")) * H2 + ox * stride2
        flat = np.concatenate([f(x2).reshape(B * H2 * H2, Cin2), np.zeros((1, Cin2))])
        g = flat[np.minimum(idx, B * H2 * H2)]
    else:
        g = f(x2)[:, ::stride2, ::stride2][:, :Ho, :Ho].reshape(M, Cin2)
    w2 = f(w2)
    if mistake == "drop_last64":
        g, w2 = g[:, :-64], w2[:, :-64]
    y = (f(x).reshape(M, Cin) @ f(w1).T + g @ w2.T) * f(scale) + f(shift)
    if relu:
        y = np.maximum(y, 0)
    if mistake == "zero_ragged_rows":
        y[256 * (M // 256):] = 0
    return y.reshape(B, Ho, Ho, Cout)


# ---- inputs and bounds of the per-block tests ---------------------------------------------------------------------------------------
def tap_images(L):
    """The batch of the per-block tests: one SYNTH_NOISE and one SYNTH_STRUCTURED image."""
    return np.concatenate([L.synth_images(7, 11, 1, L.SYNTH_NOISE), L.synth_images(20250217, 3, 1, L.SYNTH_STRUCTURED)])


def bounds(prec, ref):
    """(bound on the maximum error, bound on the median error or None): the project's tolerances for ONE layer.  fp32 and bf16x3:
    1e-4 * max(1, max|ref|).  bf16 against a reference on bf16-rounded operands and intermediates: 1.2e-2 * max(1, max|ref|) -- the
    2^-8 output rounding plus the rare one-ulp flip of a rounded intermediate -- and a median of 2e-3 * max(1, max|ref|)."""
    s = max(1.0, float(np.abs(ref).max()))
    return (1.2e-2 * s, 2e-3 * s) if prec == "bf16" else (1e-4 * s, None)


def errors(y, ref):
    err = np.abs(np.asarray(y, np.float64) - np.asarray(ref, np.float64))
    return err, float(err.max()), float(np.median(err))


def check_close(y, ref, prec, what):
    """Asserts the bounds of `prec` and returns (max error, median error) relative to max(1, max|ref|); the failure names `what`, the
    criterion and the position (image, y, x, channel) of the largest error."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    err, emax, emed = errors(y, ref)
    bmax, bmed = bounds(prec, ref)
    pos = tuple(int(v) for v in np.unravel_index(err.argmax(), err.shape))
    s = max(1.0, float(np.abs(ref).max()))
    print("%s %s: max err %.3e (bound %.3e) median %.3e%s, max|ref| %.3f" % (what, prec, emax, bmax, emed, "" if bmed is None else " (bound %.3e)" % bmed, s))
    assert emax <= bmax, "%s (%s): MAXIMUM error %.4e > %.4e at (image, y, x, channel) = %s: got %r, reference %r" % (what, prec, emax, bmax, pos, float(y[pos]), float(ref[pos]))
    if bmed is not None:
        assert emed <= bmed, "%s (%s): MEDIAN error %.4e > %.4e (largest error %.4e at (image, y, x, channel) = %s)" % (what, prec, emed, bmed, emax, pos)
    return emax / s, emed / s
