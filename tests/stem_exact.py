"""Helpers of the bit-exact stem tests (no GPU, no test in here), in the style of tests/conv_exact.py: models whose conv0 + BatchNorm is exact,
images on which every stem kernel has one correct bit pattern per pooled output, that output, a numpy model of the kernels' persistent
unit walk with planted mistakes, and a comparison that says where the differing pixels sit in the kernels' own coordinates.

The stem reads the LOADED model, so the exact operands come in as a blob (blob_of): conv0's raw tensors of the synthetic blob are replaced
by small integers (or one power of two per output channel), gamma = +-{0.5, 1, 2}, mean = 0, beta in eighths, var = 1 - 2^-10 and
bn_eps = 2^-10, for which resnet_blocks.fold -- the loader's float64 arithmetic -- gives scale == gamma and shift == beta exactly (asserted).
bf16(W), bf16(W * scale) and the fp32 epilogue acc * scale + shift then carry no rounding of their own.

Three kinds of images (224 x 224 x 3 bytes; conv0_of / images_of):
  binary  every byte 0 or 255, integer weights.  fl32(255) * fl32(1 / 255) == 1 (asserted), so x is 0 or 1 in every precision and every partial
          sum is a multiple of 1/8 far below 2^24 eighths: exact in fp32, bf16x3 and bf16 under any summation order.
  grid    bytes from {0} u [16, 255], integer weights, bf16 only: bf16(fl32(px) * fl32(1 / 255)) is a multiple of 2^-11 and at most 1
          (asserted), every product a multiple of 2^-12.  The bf16 case with many-valued pixels.
  onehot  every byte value 0 .. 255; each output channel has ONE non-zero tap, +-2^k, and the tap positions of the three "hot" blobs cover all
          147 (c, kh, kw).  A conv output is one exact product plus the shift: in the bf16 kernels that sum is exact in fp32 (asserted), in the
          fp32 kernels it is ONE rounding of an exactly known number (the product and product * scale are exact, so a fused and an unfused
          multiply-add agree), and the even channels have shift 0, where nothing is rounded at all.  Pins the byte -> float conversion
          (multiply by (float)(1.0 / 255.0); round to nearest even for bf16), the gather address of every tap and the zero padding.
budget asserts sum |w s| |x| + |shift| < 2^24 quanta per output for the summed cases.  Every image is dark in its first rows and bright in
its last ones: where a workgroup walks from one unit to the next, the row it would wrongly carry over is larger than what it must compute.

Reference (exact_ref): float64 im2col product, + shift, ReLU, the precision's single rounding (bf16: round to nearest even; bf16x3: hi + lo,
conv_exact.x3_store), maxpool 3x3 / 2 pad 1.

kernel_model restates the kernels in numpy -- pixel conversion, fp32 accumulation, the two epilogues (stem2_pool_kernel: bf16(W * scale) with
the shift as the accumulator's initial value; the others: acc * scale + shift), rounding, and pooling unit by unit along the walk of a
grid of G workgroups (unit = image * 8 + strip; workgroup w takes units w, w + G, ...) -- and takes `mistake=`: one of MISTAKES.
tests/test_stem_exact_cpu.py shows that these inputs report every one of them."""
import functools

import numpy as np

from tests import conv_exact as CE
from tests import resnet_blocks as RB

BN_EPS = 2.0 ** -10
BLOBS = ("int", "hot0", "hot1", "hot2")
KINDS_OF = {"int": ("binary", "grid"), "hot0": ("onehot",), "hot1": ("onehot",), "hot2": ("onehot",)}
PRECS_OF = {"binary": ("fp32", "bf16x3", "bf16"), "grid": ("bf16",), "onehot": ("fp32", "bf16x3", "bf16")}
# (images, cap on the stem's grid): each workgroup walks one strip of three successive images (the carried row's columns coincide); workgroup 0
# walks units 0, 5, 10, 15 (the strip changes, the walk crosses the image boundary); one workgroup walks all 8 strips; the production grid
WALKS = ((3, 8), (2, 5), (1, 1), (3, 0))
NIMG = 3
MISTAKES = ("carry_leak", "prefetch_same_image", "px_truncated", "px_divided", "truncation", "round_half_up", "shift_after_rounding", "dropped_tap",
            "col16_pooled", "pad_neighbour")
WALK_MISTAKES = ("carry_leak", "prefetch_same_image")  # need a workgroup that walks a second unit
BUDGET = float(1 << 24)


def walk_id(w):
    return "b%d_cap%d" % w


def tap_of(blob, c):
    """(input channel, kh, kw) of output channel c's one tap in blob "hot<j>": a stride coprime to 147, so that 192 channels visit all 147."""
    i = ((int(blob[3]) * 64 + c) * 40 + 3) % 147
    return i // 49, (i // 7) % 7, i % 7


@functools.lru_cache(maxsize=None)
def conv0_of(blob):
    """conv0's raw tensors of blob -> dict(W, gamma, beta, mean, var, bias=None, scale, shift); read only."""
    assert blob in BLOBS
    rng = np.random.default_rng([20250601, BLOBS.index(blob)])
    gamma = (rng.choice([0.5, 1.0, 2.0], 64) * rng.choice([-1.0, 1.0], 64)).astype(np.float32)
    if blob == "int":
        W = rng.integers(-8, 9, (64, 3, 7, 7)).astype(np.float32)
        beta = (rng.integers(-16, 65, 64) / 8.0).astype(np.float32)
    else:
        W = np.zeros((64, 3, 7, 7), np.float32)
        for c in range(64):
            # three channels of four with a positive product, one with a negative one (its output is positive where the pixel is SMALL)
            W[(c,) + tap_of(blob, c)] = 2.0 ** rng.integers(-1, 2) * (-1.0 if c % 4 == 3 else 1.0) * np.sign(gamma[c])
        beta = (rng.integers(1, 17, 64) / 8.0).astype(np.float32)
        beta[0::2] = 0  # nothing is rounded in these channels: the output is the converted pixel times a power of two
        beta[3::4] = np.maximum(beta[3::4], 1.0)
    raw = dict(W=W, bias=None, gamma=gamma, beta=beta, mean=np.zeros(64, np.float32), var=np.full(64, 1.0 - BN_EPS, np.float32))
    scale, shift = RB.fold(raw, np.float32(BN_EPS))
    assert np.array_equal(scale, gamma) and np.array_equal(shift, beta), "the loader's fold is not exact"
    ws = W * scale[:, None, None, None]
    for a in (W, ws):  # stem_pool_kernel<BF16> / stem_conv_kernel<BF16> store bf16(W), stem2_pool_kernel bf16(W * scale)
        assert np.array_equal(RB.bf16_round(a), a)
    assert np.array_equal(ws.astype(np.float64), W.astype(np.float64) * scale.astype(np.float64)[:, None, None, None])
    if blob != "int":
        assert ((W != 0).reshape(64, -1).sum(axis=1) == 1).all()
    out = dict(raw, scale=scale, shift=shift)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def taps_covered():
    """The tap positions of the three hot blobs together."""
    return {tap_of(b, c) for b in BLOBS[1:] for c in range(64)}


def blob_of(name, model):
    """model (resnet_blocks.read_blob of the synthetic blob) with conv0 replaced -> ICLW blob, the way resnet_blocks.variant_blob builds one."""
    c0 = conv0_of(name)
    raws = [dict(model.raw[0], **{k: np.array(c0[k]) for k in ("W", "gamma", "beta", "mean", "var")}, bias=None)] + list(model.raw[1:])
    return RB.write_blob(raws, model.fcw, model.fcb, BN_EPS)


@functools.lru_cache(maxsize=None)
def images_of(kind):
    """NIMG images [NIMG][224][224][3] u8 of `kind`, sparse, dark in rows 0 .. 7, bright in rows 208 .. 223; read only."""
    rng = np.random.default_rng([20250602, ("binary", "grid", "onehot").index(kind)])
    shape = (NIMG, 224, 224, 3)
    density = np.full(224, 0.12)
    density[:8], density[208:] = 0.03, 0.6
    on = rng.random(shape) < density[None, :, None, None]
    if kind == "binary":
        val = np.full(shape, 255)
    elif kind == "grid":
        val = rng.integers(16, 256, shape)
        val[:, :8] = rng.integers(16, 48, (NIMG, 8, 224, 3))
        val[:, 208:] = rng.integers(192, 256, (NIMG, 16, 224, 3))
    else:
        val = rng.integers(1, 256, shape)
        val[:, :8] = rng.integers(1, 48, (NIMG, 8, 224, 3))
        val[:, 208:] = rng.integers(192, 256, (NIMG, 16, 224, 3))
    img = np.where(on, val, 0).astype(np.uint8)
    if kind == "binary":
        assert set(np.unique(img)) == {0, 255}
    elif kind == "grid":
        assert set(np.unique(img)) == {0} | set(range(16, 256))
    else:
        assert all(len(np.unique(im)) == 256 for im in img), "an image lacks a byte value"
    img.setflags(write=False)
    return img


# ---- arithmetic ----------------------------------------------------------------------------------------------------------------------
def pixels(img, prec, mistake=None):
    """bytes -> the conv's input in `prec` (fp32, as float32): fl32(px) * fl32(1 / 255), for bf16 rounded to nearest even."""
    b = img.astype(np.float32)
    x = b / np.float32(255.0) if mistake == "px_divided" else b * np.float32(1.0 / 255.0)
    if prec != "bf16":
        return x
    if mistake == "px_truncated":
        return (np.ascontiguousarray(x).view(np.uint32) & 0xFFFF0000).view(np.float32)
    return RB.bf16_round(x)


def check_pixels():
    """The claims about the conversion, on all 256 byte values."""
    b = np.arange(256, dtype=np.uint8)
    assert np.float32(255) * np.float32(1.0 / 255.0) == np.float32(1.0)
    x = pixels(b, "bf16").astype(np.float64)
    g = x[16:] * 2.0 ** 11
    assert x[0] == 0 and np.array_equal(g, np.rint(g)) and x.max() == 1.0 and (np.diff(x) >= 0).all()
    assert np.array_equal(pixels(b, "fp32")[[0, 255]], np.array([0, 1], np.float32))


def im2col_stem(x, pad_neighbour=False):
    """[B][224][224][3] -> [B * 112 * 112][147] float64 in the order (kh, kw, c), 7 x 7 / 2 pad 3; pad_neighbour (a planted mistake): the
    three padding columns left and right hold the image's nearest column instead of zero."""
    if not pad_neighbour:
        return CE.im2col(x, 7, 2, 3)
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (3, 3), (0, 0), (0, 0)))
    xp = np.pad(xp, ((0, 0), (0, 0), (3, 3), (0, 0)), mode="edge")
    return CE.im2col(xp, 7, 2, 0)


def maxpool(y):
    """[B][H][W][C] -> maxpool 3x3 / 2 pad 1 (padding never wins)."""
    B, H, W, C = y.shape
    yp = np.full((B, H + 2, W + 2, C), -np.inf, y.dtype)
    yp[:, 1:-1, 1:-1] = y
    out = np.full((B, H // 2, W // 2, C), -np.inf, y.dtype)
    for a in range(3):
        for b in range(3):
            out = np.maximum(out, yp[:, a:a + H - 1:2, b:b + W - 1:2])
    return out


def budget(cols, ws, shift, what):
    """max over the outputs of (sum |x| |w s| + |shift|) in quanta of that output channel, asserted below 2^24: every partial sum in any order,
    the shift included, is then an integer below 2^24 times the quantum -- exact in fp32."""
    q = CE.quantum(np.unique(cols)) * CE.row_quantum(ws)
    nz = shift != 0
    if nz.any():
        q[nz] = np.minimum(q[nz], CE.row_quantum(shift[nz].reshape(-1, 1)))
    span = float((((np.abs(cols) @ np.abs(ws).T).max(axis=0) + np.abs(shift)) / q).max())
    assert span < BUDGET, "%s: sum |w s| |x| + |shift| = %.0f quanta, not below 2^24" % (what, span)
    return span


@functools.lru_cache(maxsize=16)
def exact_ref(blob, kind, prec):
    """-> dict(want: the one correct pooled output [NIMG][56][56][64] in `prec`, v32: the pooled exact value before the output rounding (fp32
    onehot with a shift: its one fp32 rounding), conv: the rounded conv output [NIMG][112][112][64], span: the budget used, or None)."""
    assert kind in KINDS_OF[blob] and prec in PRECS_OF[kind]
    what = "stem %s %s %s" % (blob, kind, prec)
    check_pixels()
    c0 = conv0_of(blob)
    f64 = lambda a: np.asarray(a, np.float64)
    x = pixels(images_of(kind), prec)
    cols, oshape = im2col_stem(x)
    ws = CE.wmat(f64(c0["W"]) * f64(c0["scale"])[:, None, None, None])
    shift = f64(c0["shift"])
    span = None
    if kind == "onehot" and prec != "bf16":
        # one product p per output: p + shift in float64 must have lost nothing (two-sum), then fp32 rounds it once
        p = cols @ ws.T
        v = p + shift
        assert np.array_equal(v - shift, p) and np.array_equal(v - p, np.broadcast_to(shift, p.shape)), "%s: float64 does not hold p + shift" % what
        assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
        v32 = np.maximum(v, 0).astype(np.float32)
        zs = shift == 0
        assert np.array_equal(v32[:, zs].astype(np.float64), np.maximum(v[:, zs], 0))
    else:
        span = budget(cols, ws, shift, what)
        v32 = CE.to_f32_exact(np.maximum(cols @ ws.T + shift, 0), what)
    v32 = v32.reshape(oshape + (64,))
    conv = {"fp32": v32, "bf16": RB.bf16_round(v32), "bf16x3": CE.x3_store(v32)}[prec]
    if prec == "bf16x3" and kind == "binary":
        assert np.array_equal(conv, v32), "%s: an output has more than hi + lo bits" % what
    out = dict(want=maxpool(conv), v32=maxpool(v32), conv=conv, span=span)
    for a in (out["want"], out["v32"], out["conv"]):
        a.setflags(write=False)
    return out


def onehot_pins_every_byte(blob="hot0"):
    """Every one of the 256 conversions is a pooled output of a zero-shift channel with a positive product, in fp32 and in bf16: the set of such
    outputs divided by the channel's weight is exactly the set of converted byte values."""
    c0 = conv0_of(blob)
    ws = (c0["W"] * c0["scale"][:, None, None, None]).reshape(64, -1).sum(axis=1)
    for prec in ("fp32", "bf16"):
        r = exact_ref(blob, "onehot", prec)
        seen = set()
        for c in np.nonzero((c0["shift"] == 0) & (ws > 0))[0]:
            seen |= set(np.unique(r["want"][..., c] / ws[c]).tolist())
        assert seen == set(pixels(np.arange(256, dtype=np.uint8), prec).tolist()), (prec, len(seen))


# ---- the kernels in numpy --------------------------------------------------------------------------------------------------------------
def _round_out(v32, prec, how="rne"):
    if prec == "fp32":
        return v32
    if prec == "bf16x3":
        return CE.x3_store(v32)
    u = np.ascontiguousarray(v32, np.float32).view(np.uint32)
    return {"rne": RB.bf16_round(v32), "truncation": (u & 0xFFFF0000).view(np.float32), "round_half_up": ((u + 0x8000) & 0xFFFF0000).view(np.float32)}[how]


def dropped_tap_of(blob):
    """(output channel, input channel, kh, kw) of the weight the mistake "dropped_tap" loses: a non-zero one."""
    c0 = conv0_of(blob)
    c = 5
    tap = tap_of(blob, c) if blob != "int" else tuple(int(v[0]) for v in np.nonzero(c0["W"][c]))
    assert c0["W"][(c,) + tap] != 0
    return (c,) + tap


def kernel_model(blob, kind, prec, B, grid, folded=False, mistake=None):
    """The stem + maxpool of images_of(kind)[:B] as a kernel computes it on a persistent grid of `grid` workgroups (0: one per unit).
    folded (bf16): stem2_pool_kernel's form -- bf16(W * scale), the shift is the accumulator's initial value; else acc * scale + shift in
    fp32.  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    assert not (folded and prec != "bf16")
    f32 = lambda a: np.asarray(a, np.float32)
    c0 = conv0_of(blob)
    img = images_of(kind)[:B]
    x = pixels(img, prec, mistake)
    cols, oshape = im2col_stem(x, pad_neighbour=mistake == "pad_neighbour")
    cols = f32(cols)
    W = np.array(c0["W"])
    if mistake == "dropped_tap":
        W[dropped_tap_of(blob)] = 0
    scale, shift = c0["scale"], c0["shift"]
    r = RB.bf16_round if prec == "bf16" else f32
    if folded:
        w = CE.wmat(r(W * scale[:, None, None, None])).astype(np.float32)
        sc = np.ones(64, np.float32)
    else:
        w, sc = CE.wmat(r(W)).astype(np.float32), scale
    if folded and mistake != "shift_after_rounding":
        v = f32(shift + f32(cols @ w.T))
    else:
        v = f32(cols @ w.T) * sc
        if mistake == "shift_after_rounding":
            v = _round_out(v, prec)
        v = f32(v + shift)
    v = np.maximum(v, 0)
    conv = _round_out(v, prec, mistake if mistake in ("truncation", "round_half_up") else "rne").reshape(oshape + (64,))
    out = maxpool(conv)
    G = grid if grid else B * 8
    for u in range(B * 8):
        b, s = u >> 3, u & 7
        cs = slice(7 * s, 7 * s + 7)
        if mistake == "col16_pooled" and s < 7:  # conv column 14 s + 14, the strip's 16th, joins the last pooled column's window
            extra = maxpool(conv[b:b + 1, :, 14 * s + 14:14 * s + 15].repeat(2, axis=2))[0, :, 0]
            out[b, :, 7 * s + 6] = np.maximum(out[b, :, 7 * s + 6], extra)
        if u < G or mistake not in WALK_MISTAKES:
            continue
        bp, sp = (u - G) >> 3, (u - G) & 7  # the unit this workgroup walked before
        if mistake == "carry_leak":  # pooled row 0 also takes the carry buffer: the previous unit's conv row 111, at the same strip offsets
            for pc in range(7):
                for kw in range(3):
                    ci = 2 * pc + kw
                    if (s == 0 and ci == 0) or not 0 <= 14 * sp - 1 + ci < 112:
                        continue
                    out[b, 0, 7 * s + pc] = np.maximum(out[b, 0, 7 * s + pc], conv[bp, 111, 14 * sp - 1 + ci])
        elif bp != b:  # prefetch_same_image: tile 0 of this unit is computed from the previous unit's image (conv rows 0 .. 7)
            top = np.array(conv[b:b + 1, :12])
            top[0, :8] = conv[bp, :8]
            out[b, :5, cs] = maxpool(top)[0, :5, cs]
    return out


# ---- the comparison ------------------------------------------------------------------------------------------------------------------
def stem_report(got, want, v32, what):
    """None if got == want element for element, else conv_exact.mismatch_report's message followed by the differing positions in the stem
    kernels' coordinates: (image, pooled row mod 4 -- the row inside a tile --, pooled column mod 7 -- the column inside a strip --, channel mod
    16 -- the lane group / wave's channel), each distinct position with its count, and the tiles (pooled row // 4) and strips they fall in."""
    msg = CE.mismatch_report(got, want, v32, what)
    if msg is None:
        return None
    bad = np.argwhere(got != want)
    key = np.stack([bad[:, 0], bad[:, 1] % 4, bad[:, 2] % 7, bad[:, 3] % 16], axis=1)
    uniq, n = np.unique(key, axis=0, return_counts=True)
    order = np.argsort(-n, kind="stable")[:24]
    lines = [msg, "(image, pooled row mod 4, pooled column mod 7, channel mod 16): count -- %d distinct, the most frequent:" % len(uniq)]
    lines += ["  %s: %d" % (tuple(int(v) for v in uniq[i]), int(n[i])) for i in order]
    for name, idx, m in (("tile (pooled row // 4)", bad[:, 1] // 4, 14), ("strip (pooled column // 7)", bad[:, 2] // 7, 8)):
        h = np.bincount(idx, minlength=m)
        lines.append("%s: %s" % (name, " ".join("%d:%d" % (i, k) for i, k in enumerate(h) if k)))
    return "\n".join(lines)


def assert_exact(got, want, v32, what):
    msg = stem_report(got, want, v32, what)
    assert msg is None, msg


def report_line(kernel, blob, kind, prec, B, cap, v32, got, want):
    r, t, up = CE.rounding_shares(v32)
    return "stem_exact: %-36s %-6s %-5s %-6s B %d cap %d  rounded %4.1f %% ties %4.1f %% (up %4.1f %%)  mismatches %d" % (
        kernel, prec, blob, kind, B, cap, 100 * r, 100 * t, 100 * up, int((got != want).sum()))
