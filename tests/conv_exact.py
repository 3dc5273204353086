"""Helpers of the bit-exact convolution tests (no GPU, no test in here): inputs whose every product, every partial sum in any order and
whole epilogue are exactly representable in fp32, the one correct output per element, and a comparison whose failure message says where
the differing elements sit.

Why equality.  exact_case draws x and w from small integers, the scale from powers of two and the shift from multiples of 1/8.  Every
term of an accumulator is then a multiple of one quantum q, and exact_matmul asserts max(sum |x| |w|) < 2^22 q: fp32 addition of exactly
representable operands with an exactly representable sum is exact under any rounding and any association, so a kernel's K-tile order,
tile shape, split or fusion cannot change the accumulator.  The epilogue acc * scale + shift (+ residual) is asserted to survive
float64 -> fp32 -> float64, so fp32 holds it exactly as well.  What is left is the one rounding a kernel is allowed:
  fp32    none: the number itself;
  bf16    round-to-nearest-even of that number (resnet_blocks.bf16_round);
  bf16x3  the storage form hi = bf16(v), lo = bf16(v - hi), read back as hi + lo (BF16X3::split, host_join32): the number itself
          wherever it has at most 16 significant bits (every "small" case: asserted), and the same two roundings of an exactly known
          number where it has more (the "x_split" / "w_split" cases, whose sums reach 2^19).
The shares of outputs that need rounding, that are exact ties and that are ties rounding upwards are asserted per case (finish), so
a case cannot pass because nothing in it had to be rounded.  Two exceptions, both stated where they are made: the split-operand cases
run in bf16x3 only and their sums of 2^17 to 2^19 with three fractional bits are almost never ties, so they assert the share of
non-zero lo parts instead; and the bottleneck's output, three layers deep, has about 1 % ties, asserted in absolute numbers.

kernel_model restates a kernel's arithmetic in numpy (split operands, three products, K chunks of 64, epilogue, rounding) and takes
`mistake=`: one deliberate error from MISTAKES.  tests/test_conv_exact_cpu.py shows that the exact comparison reports every one of
them and that resnet_blocks.bounds lets several through."""
import collections
import functools

import numpy as np

from tests import resnet_blocks as RB

SPAN = float(1 << 22)
# one deliberate error each, applied inside kernel_model
MISTAKES = ("truncation", "round_half_up", "residual_after_rounding", "scale_shift_bf16", "bf16_partial_sums", "dropped_product",
            "neighbour_shift", "lo_ignored", "relu_before_residual")

Conv = collections.namedtuple("Conv", "B H cin cout k stride res relu kind")


def conv(B, H, cin, cout, k, stride=1, res=False, relu=True, kind="small"):
    return Conv(B, H, cin, cout, k, stride, res, relu, kind)


def conv_id(c):
    return "b%d_h%d_c%d-%d_k%d_s%d%s%s%s" % (c.B, c.H, c.cin, c.cout, c.k, c.stride, "_res" if c.res else "", "" if c.relu else "_norelu",
                                             "" if c.kind == "small" else "_" + c.kind)


# ---- the cases of tests/test_conv_exact_gpu.py, by the route they are meant for (test_conv_exact_cpu.py checks exact_ref's conditions on each) ----
IGEMM_CASES = [conv(3, 7, 64, 64, 3), conv(2, 9, 64, 192, 1, relu=False), conv(1, 14, 256, 128, 1, 2), conv(2, 7, 128, 256, 1, res=True, relu=False)]
HALO_CASES = [conv(3, 7, 128, 128, 3), conv(2, 9, 256, 128, 3, relu=False), conv(1, 28, 192, 128, 3)]
# (2, 23, 256, 128, 1): bf16 takes conv_wr_kernel (K = 256, Cout = 128 is its shape too, and conv_select asks it first), bf16x3
# conv_p8_kernel's 512 x 128 layout; (2, 23, 384, 128, 1) is the same hazard at a K conv_wr_kernel does not take
P8_CASES = [conv(2, 23, 256, 128, 1, res=True), conv(2, 23, 384, 128, 1, res=True), conv(3, 14, 128, 384, 3, relu=False),
            conv(11, 7, 128, 256, 3, res=True), conv(7, 14, 512, 768, 1, relu=False), conv(3, 12, 384, 256, 1, res=True), conv(2, 14, 512, 256, 1, 2)]
SPLIT_CASES = [conv(1, 7, 512, 512, 3), conv(11, 7, 2048, 512, 1, relu=False), conv(6, 14, 2048, 512, 1, 2), conv(5, 5, 256, 768, 3, res=True)]
WR_SHAPES = [(3, 9, 128, 512), (5, 7, 256, 1024), (1, 33, 512, 128), (4, 7, 512, 2048)]
WR_CASES = [conv(B, H, cin, cout, 1, res=res, relu=relu) for (B, H, cin, cout) in WR_SHAPES for res in (True, False) for relu in (True, False)]
X3_SPLIT_CASES = [conv(2, 9, 128, 256, 1, res=True, kind=kind) for kind in ("x_split", "w_split")] + \
                 [conv(3, 7, 64, 128, 3, relu=False, kind=kind) for kind in ("x_split", "w_split")]
DUAL_CASES = [(RB.DUAL_SHAPES[3], True), (RB.DUAL_SHAPES[4], False), (RB.DUAL_SHAPES[6], True), (RB.DUAL_SHAPES[7], False)]  # (shape, relu)
BNECK_CASES = [(3, 9, 20), (1, 7, 14), (2, 16, 3)]  # (B, H, W), each in both forms


def wr_rule(K, cout, ncu, M):
    """conv_select's rule for conv_wr_kernel (conv_select.h) -> (pixels per tile, workers) for a K -> cout layer of M pixels on ncu compute units."""
    ns, pt = {128: (256, 64), 256: (128, 64), 512: (128, 32)}[K]
    nslices = cout // ns
    nworkers = max(8, (2 * ncu // nslices) & ~7)
    ntiles = -(-M // pt)
    return pt, min(nworkers, -(-ntiles // 8) * 8)


def wr_walk_case(K, ncu):
    """The smallest 9 x 9-image batch at which every conv_wr_kernel worker of a K -> 2048 layer walks at least three tiles (the double
    buffer is reused, the prefetched residual is used, a tile past the end is requested) and the last tile is ragged."""
    pt, nworkers = wr_rule(K, 2048, ncu, 1 << 30)
    B = -(-(3 * nworkers * pt + 1) // 81)
    while (B * 81) % pt == 0:
        B += 1
    c = conv(B, 9, K, 2048, 1, res=True)
    assert wr_rule(K, 2048, ncu, B * 81) == (pt, nworkers) and -(-B * 81 // pt) > 3 * nworkers
    return c


def route(c, prec, mode, split=False):
    """The kernel conv_select (imageclust_amd/csrc/conv_select.h; launch_conv_t and the forward plan launch what it chooses) picks for
    convolution c in `prec` under ICL_CONV_P8_* `mode` (0 off, 1 auto, 2 all; split: | ICL_CONV_SPLIT), restated independently from its
    conv_wr_eligible, conv_p8_eligible, conv_p8_split_eligible and halo rule.  tests/test_conv_select_cpu.py checks the header's choice
    against it without a GPU; the GPU tests check it against the launch counters (conv_stats: [0] conv_wr_kernel and conv_p8_kernel,
    [1] the 128 x 128 kernels; conv_split_launches), which cannot tell the kernels of one counter apart."""
    x3 = prec == "bf16x3"
    K, Ho = c.k * c.k * c.cin, (c.H + 2 * (c.k // 2) - c.k) // c.stride + 1
    if prec == "bf16" and mode and c.k == 1 and c.stride == 1 and K in (128, 256, 512) and c.cout % (256 if K == 128 else 128) == 0 \
            and not (K == 512 and 128 < c.cout < 2048):
        return "conv_wr_kernel<%d>" % K
    Ke = 2 * K if x3 else K
    if prec != "fp32" and mode and c.cout % 128 == 0 and Ke % 128 == 0 and (mode == 2 or Ke // 64 >= 4):
        if split and not x3 and c.cout % 256 == 0 and Ho * Ho <= 49 and K % 256 == 0 and K >= 2048:
            return "conv_p8_kernel<256x256, split>"
        return "conv_p8_kernel<%s>" % ("256x256" if c.cout % 256 == 0 else "512x128")
    wide = 128 if c.cout % 128 == 0 else 64
    rows = (c.H - 1 + 127) // c.H + 3
    if c.k == 3 and c.stride == 1 and (2 * c.cin if x3 else c.cin) >= 128 and ((rows * (c.H + 2) + 7) // 8 + 3) // 4 <= 12:
        return "conv3x3_halo_kernel<%d>" % wide
    return "conv_igemm_kernel<%d>" % wide


def counters_of(kernel):
    """(conv_stats()[0] increment, conv_stats()[1] increment, conv_split_launches() increment) of one launch of `kernel`."""
    first = kernel.startswith(("conv_wr", "conv_p8"))
    return int(first), int(not first), int("split" in kernel)


# ---- exact arithmetic -------------------------------------------------------------------------------------------------------
def quantum(a):
    """The largest power of two that divides every element of a (float64)."""
    a = np.asarray(a, np.float64)
    for e in range(16, -40, -1):
        s = a / 2.0 ** e
        if np.array_equal(s, np.rint(s)):
            return 2.0 ** e
    raise AssertionError("no dyadic quantum")


def im2col(x, k, stride, pad):
    """[B][H][W][C] -> [B * Ho * Wo][k * k * C] in the kernels' K order (kh, kw, c), float64, zero padding."""
    B, H, W, C = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, C), np.float64)
    xp[:, pad:pad + H, pad:pad + W] = x
    cols = [xp[:, a:a + (Ho - 1) * stride + 1:stride, b:b + (Wo - 1) * stride + 1:stride] for a in range(k) for b in range(k)]
    return np.concatenate(cols, axis=3).reshape(B * Ho * Wo, k * k * C), (B, Ho, Wo)


def wmat(w):
    """OIHW -> [Cout][k * k * Cin] in the K order of im2col, float64."""
    return np.ascontiguousarray(np.asarray(w, np.float64).transpose(0, 2, 3, 1)).reshape(w.shape[0], -1)


def row_quantum(w):
    """quantum of every row of w [N][K]."""
    q, todo = np.zeros(w.shape[0]), np.ones(w.shape[0], bool)
    for e in range(16, -40, -1):
        s = w / 2.0 ** e
        ok = todo & (s == np.rint(s)).all(axis=1)
        q[ok] = 2.0 ** e
        todo &= ~ok
    assert not todo.any(), "no dyadic quantum"
    return q


def exact_matmul(a, w, what):
    """a [M][K] . w [N][K]^T in float64, with the span condition asserted: every term of output channel n (one accumulator per output
    element) is a multiple of q[n] = quantum(a) * quantum(w[n]) and max(sum |a| |w[n]|) < 2^22 q[n], so every partial sum in any
    order is an integer below 2^22 times q[n] -- exact in fp32 (and in float64)."""
    span = float(((np.abs(a) @ np.abs(w).T).max(axis=0) / (quantum(a) * row_quantum(w))).max())
    assert span < SPAN, "%s: max(sum |x| |w|) = %.0f quanta, not below 2^22" % (what, span)
    return a @ w.T


def to_f32_exact(v, what):
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v), "%s: %d values are not representable in fp32" % (what, int((v32.astype(np.float64) != v).sum()))
    return v32


def split(a):
    """fp32 -> (hi, lo) of the split bf16 storage: hi = bf16(a), lo = bf16(a - hi)."""
    a = np.ascontiguousarray(a, np.float32)
    hi = RB.bf16_round(a)
    return hi, RB.bf16_round(a - hi)


def x3_store(v32):
    hi, lo = split(v32)
    return hi + lo


def rounding_shares(v32):
    """(share that needs rounding to bf16, share of exact ties, share of ties that round upwards -- to the even neighbour of larger magnitude)."""
    u = np.ascontiguousarray(v32, np.float32).view(np.uint32)
    low = u & 0xFFFF
    tie = low == 0x8000
    return float((low != 0).mean()), float(tie.mean()), float((tie & (((u >> 16) & 1) == 1)).mean())


def finish(v, prec, relu, what, shares):
    """The exact epilogue value v (float64) -> (the one correct output in `prec`, v in fp32), with the conditions on v asserted.
    shares "conv": at least 25 % of the outputs need rounding, 5 % are ties and 2 % ties that round upwards, and hi + lo holds every
    output.  "chain" (the bottleneck's output, three layers deep: its values span 2^20 quanta, and a tie needs every bit below the
    bf16 ulp but the first to be zero, so ties are about 1 % there): 25 % need rounding, and at least 200 ties and 100 ties
    upwards in absolute numbers -- a wrong tie rule cannot go unseen.  None: the split-operand cases (bf16x3 only)."""
    assert shares in (None, "conv", "chain")
    if relu:
        v = np.maximum(v, 0)
    else:
        assert (v < 0).any(), "%s: no negative output in a case without ReLU" % what
    v32 = to_f32_exact(v, what)
    r, t, up = rounding_shares(v32)
    msg = "%s: %.1f %% of the outputs need rounding, %.1f %% are ties, %.1f %% ties upwards" % (what, 100 * r, 100 * t, 100 * up)
    if shares == "conv":
        assert r >= 0.25 and t >= 0.05 and up >= 0.02, msg + " (25 / 5 / 2 % wanted)"
        assert np.array_equal(x3_store(v32), v32), "%s: an output has more than hi + lo bits" % what
    elif shares == "chain":
        assert r >= 0.25 and t * v32.size >= 200 and up * v32.size >= 100, msg + " (25 %, 200 and 100 elements wanted)"
    return {"fp32": v32, "bf16": RB.bf16_round(v32), "bf16x3": x3_store(v32)}[prec], v32


# ---- one convolution ---------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


def _bn(rng, c, smax=3, shmax=64):
    """scale = 2^-s, s in 0..smax per channel; shift a multiple of 1/8 in [-shmax / 4, shmax].  (Not centred: a ReLU turns every
    negative value into the same exact 0, and with a centred shift a ReLU case of K <= 256 has too few outputs left that need
    rounding -- 19-25 % against 28-35 % with this draw, measured on the cases below.)"""
    return (2.0 ** -rng.integers(0, smax + 1, c)).astype(np.float32), (rng.integers(-2 * shmax, 8 * shmax + 1, c) / 8.0).astype(np.float32)


@functools.lru_cache(maxsize=2)
def exact_case(shape, kind="small", seed=0):
    """shape = (B, H, Cin, Cout, k, stride) -> dict(x, w, scale, shift, res, acc, ...).  kind "small": x integers in [-8, 8], w integers in
    [-4, 4]; "x_split": x integers in [-2000, 2000] (hi + lo exact, lo != 0 for about two thirds), w small; "w_split": the mirror image.
    scale[c] = 2^-s, s in 0..3; shift[c] a multiple of 1/8 in [-16, 64] (see _bn); the residual integers in [-128, 128].  All fp32; everything
    but the split operand is bf16-representable.  acc is the exact accumulator (float64, [B][Ho][Ho][Cout]), span condition asserted.
    The result is shared between the precisions and options of a case: nobody writes to it."""
    B, H, cin, cout, k, stride = shape
    assert kind in ("small", "x_split", "w_split")
    rng = np.random.default_rng([seed, B, H, cin, cout, k, stride, ("small", "x_split", "w_split").index(kind)])
    x = _ints(rng, *((-2000, 2000) if kind == "x_split" else (-8, 8)), (B, H, H, cin))
    w = _ints(rng, *((-2000, 2000) if kind == "w_split" else (-4, 4)), (cout, cin, k, k))
    scale, shift = _bn(rng, cout)
    cols, oshape = im2col(x, k, stride, k // 2)
    acc = exact_matmul(cols, wmat(w), "conv %s %s" % (shape, kind)).reshape(oshape + (cout,))
    res = _ints(rng, -128, 128, oshape + (cout,))
    for name, a in (("x", x), ("w", w)):
        hi, lo = split(a)
        assert np.array_equal(hi.astype(np.float64) + lo, a), "%s is not hi + lo" % name
        if kind == name + "_split":
            assert (lo != 0).mean() >= 0.5, "lo of %s is non-zero for %.0f %% only" % (name, 100 * (lo != 0).mean())
        else:
            assert not lo.any()
    for a in (scale, res):  # (a shift such as 63.875 has nine bits: no kernel stores it in bf16)
        assert np.array_equal(RB.bf16_round(a), a)
    out = dict(x=x, w=w, scale=scale, shift=shift, res=res, acc=acc, stride=stride, pad=k // 2, M=acc.size // cout, K=k * k * cin, N=cout)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def case_of(c, seed=0):
    return exact_case((c.B, c.H, c.cin, c.cout, c.k, c.stride), c.kind, seed)


def exact_ref(c, prec, seed=0):
    """The one correct output of convolution case c (a Conv) in `prec` -> (wanted, exact fp32 value before the output rounding)."""
    d = case_of(c, seed)
    v = d["acc"] * d["scale"].astype(np.float64) + d["shift"].astype(np.float64)
    if c.res:
        v = v + d["res"]
    return finish(v, prec, c.relu, "conv %s" % conv_id(c), "conv" if c.kind == "small" else None)


def _round(v32, prec, how):
    if prec == "fp32":
        return v32
    u = np.ascontiguousarray(v32, np.float32).view(np.uint32)
    one = {"rne": RB.bf16_round, "truncation": lambda a: (u & 0xFFFF0000).view(np.float32), "round_half_up": lambda a: ((u + 0x8000) & 0xFFFF0000).view(np.float32)}[how]
    if prec == "bf16":
        return one(v32)
    return x3_store(v32)


def kernel_model(c, prec, mistake=None, seed=0):
    """The convolution as a kernel computes it, in numpy: operands in the storage of `prec` (bf16x3: hi and lo, three products, wl.xl dropped),
    fp32 accumulation over K chunks of 64, the epilogue acc * scale + shift (+ residual), ReLU, one rounding.  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    d = case_of(c, seed)
    f32 = lambda a: np.asarray(a, np.float32)
    if prec == "bf16x3":
        (xh, xl), (wh, wl) = split(d["x"]), split(d["w"])
    else:
        r = RB.bf16_round if prec == "bf16" else f32
        xh, wh = r(d["x"]), r(d["w"])
        xl, wl = np.zeros_like(xh), np.zeros_like(wh)
    if mistake == "lo_ignored":
        xl, wl = np.zeros_like(xh), np.zeros_like(wh)
    (ch, oshape), cl = im2col(xh, c.k, c.stride, c.k // 2), im2col(xl, c.k, c.stride, c.k // 2)[0]
    mh, ml = wmat(wh), wmat(wl)
    acc = np.zeros((ch.shape[0], c.cout), np.float32)
    for k0 in range(0, ch.shape[1], 64):
        s = slice(k0, k0 + 64)
        acc = f32(acc + f32(ch[:, s] @ mh[:, s].T + ch[:, s] @ ml[:, s].T + cl[:, s] @ mh[:, s].T))
        if mistake == "bf16_partial_sums":
            acc = RB.bf16_round(acc)
    scale, shift, res = d["scale"], d["shift"], d["res"].reshape(-1, c.cout)
    if mistake == "dropped_product":  # one product of one output element whose value is small and positive
        v = d["acc"].reshape(-1, c.cout) * scale + shift + (res if c.res else 0)
        m, n = np.unravel_index(np.where(v > 0, v, np.inf).argmin(), v.shape)
        p = (ch[m] + cl[m]) * (mh[n] + ml[n])
        kk = np.where(p != 0, np.abs(p), np.inf).argmin()
        acc[m, n] -= np.float32(p[kk])
    if mistake == "scale_shift_bf16":
        scale, shift = RB.bf16_round(scale), RB.bf16_round(shift)
    if mistake == "neighbour_shift":
        shift = np.roll(shift, 1)
    v = f32(acc * scale + shift)
    if mistake == "residual_after_rounding":
        v = _round(v, prec, "rne")
    if mistake == "relu_before_residual" and c.relu:
        v = np.maximum(v, 0)
    if c.res:
        v = f32(v + res)
    if c.relu:
        v = np.maximum(v, 0)
    return _round(v, prec, mistake if mistake in ("truncation", "round_half_up") else "rne").reshape(oshape + (c.cout,))


# ---- the dual-operand launch: two products, one epilogue --------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def dual_case(shape, seed=0):
    """Inputs of icl_conv2d_dual at resnet_blocks.DUAL_SHAPES' shape, drawn as exact_case draws them, and the exact accumulator."""
    B, Ho, H2, s2, cin, cin2, cout = shape
    rng = np.random.default_rng([seed] + list(shape))
    x, x2 = _ints(rng, -8, 8, (B, Ho, Ho, cin)), _ints(rng, -8, 8, (B, H2, H2, cin2))
    w1, w2 = _ints(rng, -4, 4, (cout, cin)), _ints(rng, -4, 4, (cout, cin2))
    scale, shift = _bn(rng, cout)
    g = x2[:, ::s2, ::s2][:, :Ho, :Ho]
    a = np.concatenate([x.reshape(-1, cin), g.reshape(-1, cin2)], axis=1).astype(np.float64)
    acc = exact_matmul(a, np.concatenate([w1, w2], axis=1).astype(np.float64), "dual %s" % (shape,)).reshape(B, Ho, Ho, cout)
    return dict(x=x, w1=w1, x2=x2, w2=w2, stride2=s2, scale=scale, shift=shift, acc=acc, M=B * Ho * Ho, K=cin + cin2, N=cout)


def dual_ref(shape, relu, prec, seed=0):
    d = dual_case(shape, seed)
    return finish(d["acc"] * d["scale"].astype(np.float64) + d["shift"].astype(np.float64), prec, relu, "dual %s" % (shape,), "conv")


# ---- the fused stage-1 bottleneck ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def bneck_case(shape, ds, seed=0):
    """Inputs of icl_bottleneck56 ((B, H, W); ds: the downsample form, Cin = 64) and its one correct bf16 output.  sc1 = 2^-2 (2^-1 for
    Cin = 64), sc2 = 2^-4, shifts within [-2, 8] and w2 in [-2, 2] keep t1 a multiple of 2^-3 and t2 a multiple of 2^-7 of moderate
    size, and sc3 / scds are 1 or 1/2, so that the span condition holds for c2 and c3 too (exact_matmul asserts it; every scale is folded into the weights, as the kernel's
    packing does).  t1 and t2 are the round-to-nearest-even of their exact values, as the kernel keeps them in bf16: each must have
    at least 25 % of its non-zero values rounded and 100 ties of its own."""
    B, H, W = shape
    cin = 64 if ds else 256
    rng = np.random.default_rng([seed, B, H, W, int(ds)])
    f64 = lambda a: np.asarray(a, np.float64)
    x = _ints(rng, -8, 8, (B, H, W, cin))
    p = {"w1": _ints(rng, -4, 4, (64, cin)), "w2": _ints(rng, -2, 2, (64, 64, 3, 3)), "w3": _ints(rng, -4, 4, (256, 64))}
    p["bn1"], p["bn2"], p["bn3"] = _bn(rng, 64, 0, 8), _bn(rng, 64, 0, 8), _bn(rng, 256, 1)
    p["bn1"], p["bn2"] = (p["bn1"][0] / (2 if ds else 4), p["bn1"][1]), (p["bn2"][0] / 16, p["bn2"][1])
    what = "bottleneck %s %s" % (shape, "downsample" if ds else "identity")
    fold = lambda w, bn: f64(w) * f64(bn[0]).reshape((-1,) + (1,) * (w.ndim - 1))  # a power of two times a small integer: bf16 holds it

    def rnd(v, name):
        v32 = to_f32_exact(np.maximum(v, 0), what + " " + name)
        r, t, _ = rounding_shares(v32[v32 > 0])
        assert r >= 0.25 and t * (v32 > 0).sum() >= 100, "%s %s: %.1f %% of the non-zero values need rounding, %.1f %% are ties" % (what, name, 100 * r, 100 * t)
        return f64(RB.bf16_round(v32))

    xm = f64(x).reshape(-1, cin)
    t1 = rnd(exact_matmul(xm, fold(p["w1"], p["bn1"]), what + " c1") + f64(p["bn1"][1]), "t1").reshape(B, H, W, 64)
    t2 = rnd(exact_matmul(im2col(t1, 3, 1, 1)[0], wmat(fold(p["w2"], p["bn2"])), what + " c2") + f64(p["bn2"][1]), "t2")
    if ds:
        p["wds"], p["bnds"] = _ints(rng, -4, 4, (256, 64)), _bn(rng, 256, 1)
        a, w = np.concatenate([t2, xm], axis=1), np.concatenate([fold(p["w3"], p["bn3"]), fold(p["wds"], p["bnds"])], axis=1)
        v = exact_matmul(a, w, what + " c3 + ds") + f64(to_f32_exact(f64(p["bn3"][1]) + f64(p["bnds"][1]), what + " shift"))
    else:
        v = exact_matmul(t2, fold(p["w3"], p["bn3"]), what + " c3") + f64(p["bn3"][1]) + xm
    for name in ("w1", "w2", "w3", "wds"):
        if name in p:
            fw = fold(p[name], p["bn" + name[1:]]).astype(np.float32)
            assert np.array_equal(RB.bf16_round(fw), fw)
    want, v32 = finish(v.reshape(B, H, W, 256), "bf16", True, what, "chain")
    return dict(x=x, p=p, want=want, v32=v32, M=B * H * W)


# ---- the comparison -------------------------------------------------------------------------------------------------------------
def mismatch_report(got, want, v32, what):
    """None if got == want element for element (np.array_equal: -0 equals +0), else the failure message: the count, the first position with
    both bit patterns and whether the wanted value was a tie, and histograms of the differing positions modulo the kernels' tile sizes."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)
    pos = tuple(int(v) for v in bad[0])
    bits = lambda a: int(np.asarray(a[pos], np.float32).view(np.uint32))
    tie = (int(np.asarray(v32[pos], np.float32).view(np.uint32)) & 0xFFFF) == 0x8000
    pix = (bad[:, 0] * got.shape[1] + bad[:, 1]) * got.shape[2] + bad[:, 2]
    lines = ["%s: %d of %d elements differ" % (what, len(bad), got.size),
             "first at (image, y, x, channel) = %s: got 0x%08x (%r), wanted 0x%08x (%r) = the rounding of %r, %s" %
             (pos, bits(got), float(got[pos]), bits(want), float(want[pos]), float(v32[pos]), "a tie" if tie else "no tie")]
    for name, idx, mods in (("pixel", pix, (16, 32, 64, 256)), ("channel", bad[:, 3], (8, 16, 32, 128))):
        for m in mods:
            h = np.bincount(idx % m, minlength=m)
            lines.append("%s mod %d: %s" % (name, m, " ".join("%d:%d" % (i, n) for i, n in enumerate(h) if n)))
    return "\n".join(lines)


def assert_exact(got, want, v32, what):
    msg = mismatch_report(got, want, v32, what)
    assert msg is None, msg
