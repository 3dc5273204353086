"""Helpers of the bit-exact tests of the FAST-mode distance matrix (no GPU, no test in here): dist_split_kernel, dist_gemm_tile<BF16> and
dist_store_rows of imageclust_amd/csrc/distance_mfma.hip, modelled on tests/conv_exact.py.

Why equality.  exact_rows draws every coordinate as m * 2^-4 with integer m of at most 11 significant bits, so e = hi + lo holds with
hi = bf16(e), lo = bf16(e - hi), every product of two parts is a multiple of one quantum q = 2^-8 and every square too.  expected asserts
max(sum (|hi_a| + |lo_a|)(|hi_b| + |lo_b|)) < 2^22 q and every row norm < 2^23 q: fp32 addition of exactly representable operands with
an exactly representable sum is exact under any rounding and any association, so the order in which the matrix cores, the k-steps and
the norm's summation tree add cannot change a bit.  0.5 (n_a + n_b) is then a multiple of 2^-9 below 2^24 of them and the difference to
the dot product is asserted to survive float64 -> fp32 -> float64: there is ONE correct bit pattern per entry,
    0.5 (|a|^2 + |b|^2) - (a.b - la.lb)   stored as +0 where it is not positive, +0 on the diagonal.
The lo.lo product the kernel leaves out on purpose stands in the expected value exactly, so the comparison pins WHICH three products are
computed.  The shares expected returns (coordinates with lo != 0, pairs with la.lb != 0, clamped entries, entries that differ from the
plain 0.5 |a - b|^2) are asserted per case by the tests, so a case cannot pass because nothing in it was exercised.

kernel_model restates the kernel in numpy and takes `mistake=`: one deliberate error from MISTAKES.  tests/test_dist_exact_cpu.py shows
that the exact comparison reports every one of them and that the scale-relative 2e-5 of test_mfma_distance_tile_error_bound lets
several through.

float_rows / error_bound: ordinary and adversarial floats for the invariance tests and the entry-wise bound against fp64."""
import functools
import math

import numpy as np

from tests import resnet_blocks as RB

SPAN = float(1 << 22)  # as tests/conv_exact.py
Q = 2.0 ** -4          # every coordinate of exact_rows is an integer multiple of it
TILE = 128             # dist_mfma_kernel's tile
KINDS = ("small", "split", "duplicates", "clamp", "zero_rows")
# one deliberate error each, applied inside kernel_model
MISTAKES = ("lo_ignored", "dropped_segment", "lolo_included", "truncating_split", "dropped_last_kstep", "neighbour_row", "no_clamp",
            "negative_zero_kept", "norms_from_hi", "diagonal_not_zero", "pad_not_zero")

# ---- the cases of tests/test_dist_exact_gpu.py (test_dist_exact_cpu.py checks expected's conditions and the floors on each) ----
NS = (1, 2, 127, 128, 129, 257, 300)   # one ragged tile, one full tile, a second tile row of one row, an interior tile, a ragged third row
DS = (1, 63, 64, 65, 100, 192)
LONG_CASE = (129, 2048, "sparse")      # 96 k-steps: both stages of the double buffer are reused many times
EXACT_CASES = [(n, d, kind) for n in NS for d in DS for kind in (KINDS if d == 100 else ("split",))] + [LONG_CASE]
PITCH_CASE = (131, 100, "split")
PITCHES = (131, 132, 133, 135, 136)    # ld = n, n + 1, n + 2, n + 4, n + 5: 132 and 136 take the 16-byte stores
PACKED_CASE = (300, 100, "split")


def case_id(c):
    return "n%d_d%d_%s" % c


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _odd(rng, bits, shape, top=None):
    """Odd integers of exactly `bits` significant bits (below `top` where given) and random sign: lo != 0 for bits >= 9."""
    m = rng.integers(1 << (bits - 2), (top or 1 << bits) // 2, shape) * 2 + 1
    return m * rng.choice((-1, 1), shape)


def _split(rng, n, d, eleven=True):
    """|m| <= 3 everywhere; in EVERY row column 0 holds a 10-bit tie 4j + 2 (lo = +-2) and the LAST column (the last k-step) a 9-bit odd value (lo = +-1), so
    la.lb = +-4 +- 1 from these two alone never cancels; each group of 8 consecutive rows has two columns of its own with 10-bit values
    below 768 (against another group's rows: hi.lo on one side, lo.hi on the other); every 16th row has one 11-bit value in a column where every
    other row is small.  The magnitudes are what the span condition allows: 2047 * 2047 alone would be 2^22."""
    m = rng.integers(-3, 4, (n, d))
    ns = min(2, d)
    if ns:
        m[:, 0] = (4 * rng.integers(128, 255, n) + 2) * rng.choice((-1, 1), n)
    if ns > 1:
        m[:, d - 1] = _odd(rng, 9, n)
    rest = d - ns
    half = rest // 2 if rest >= 2 else rest  # the groups' columns come from the first half of the rest, the 11-bit ones from the second
    if rest > 0:
        for g0 in range(0, n, 8):
            rows = np.arange(g0, min(g0 + 8, n))
            cols = 1 + rng.choice(half, min(2, half), replace=False)
            m[np.ix_(rows, cols)] = _odd(rng, 10, (len(rows), len(cols)), top=768)
        own = 1 + half + rng.permutation(rest - half)
        for t, r in enumerate(range(5, n, 16)):
            if eleven and t < len(own):
                m[r, own[t]] = _odd(rng, 11, ())
    return m


def _clamp(rng, n, d):
    """Rows 2p and 2p + 1 are equal but for column 0, a 10-bit value (bf16 spacing 4) in every row: 4j + 2, a tie whose lo is +2 (j even) or
    -2 (j odd), next to 4j + 3 (lo -1) or 4j + 1 (lo +1).  0.5 |a - b|^2 + la.lb = (0.5 - 2) q: negative, stored as +0."""
    m = np.repeat(rng.integers(-3, 4, ((n + 1) // 2, d)), 2, axis=0)[:n]
    if d:
        j = np.repeat(rng.integers(128, 255, (n + 1) // 2), 2)[:n]
        odd_row = np.arange(n) % 2 == 1
        m[:, 0] = 4 * j + 2 + np.where(odd_row, np.where(j % 2 == 0, 1, -1), 0)
    return m


@functools.lru_cache(maxsize=8)
def exact_rows(n, d, seed=0, kind="split"):
    """fp32 rows [n][d] whose every coordinate is m * 2^-4 with integer m:
      small       |m| <= 3: lo == 0;
      split       small plus a few coordinates per row of 9 to 11 significant bits (_split); "sparse" is the same draw under the name the
                  d = 2048 case uses, where those few columns are too small a share for split's floors;
      duplicates  split rows without the 11-bit values (two copies of one would reach the span alone), four copies of each, shuffled: the
                  correct entry of a pair of copies is sum lo^2, not 0;
      clamp       pairs whose exact value is negative (_clamp);
      zero_rows   split rows, about a third of them (and row 0) all zero.
    The result is shared between the tests: nobody writes to it."""
    assert kind in KINDS + ("sparse",)
    rng = np.random.default_rng([seed, n, d, (KINDS + ("sparse",)).index(kind)])
    if kind == "small":
        m = rng.integers(-3, 4, (n, d))
    elif kind == "clamp":
        m = _clamp(rng, n, d)
    elif kind == "duplicates":
        m = np.repeat(_split(rng, (n + 3) // 4, d, eleven=False), 4, axis=0)[:n][rng.permutation(n)]
    else:
        m = _split(rng, n, d)
        if kind == "zero_rows":
            m[rng.random(n) < 0.3] = 0
            m[0] = 0
    E = (m * Q).astype(np.float32)
    E.setflags(write=False)
    return E


def mog(n, d, seed, k=None, sigma=0.1):
    """The one input family of test_mfma_distance_tile_error_bound (tests/test_fast_mode_gpu.py): a mixture of Gaussians."""
    rng = np.random.default_rng(seed)
    k = k or max(1, n // 20)
    cen = rng.standard_normal((k, d)).astype(np.float32)
    lab = rng.integers(0, k, n)
    return (cen[lab] + sigma * rng.standard_normal((n, d))).astype(np.float32)


FLOAT_KINDS = ("normal", "offset", "duplicates", "near_duplicates", "zero_rows", "huge_coordinate", "tiny", "large")
BOUND_SHAPES = ((130, 64), (257, 100), (129, 2048))


@functools.lru_cache(maxsize=4)
def float_rows(n, d, kind, seed=0):
    """Ordinary fp32 rows: standard normal; + 100 (cancellation, coherent split residuals); exact duplicates (8 copies); near duplicates
    (* (1 + 1e-6 g)); rows of zeros; one coordinate * 1e4; the whole input * 1e-15 and * 1e15."""
    assert kind in FLOAT_KINDS
    rng = np.random.default_rng([20260117, seed, n, d])
    g = rng.standard_normal((n, d)).astype(np.float32)
    if kind == "offset":
        g = (g + 100.0).astype(np.float32)
    elif kind == "duplicates":
        g = np.ascontiguousarray(np.repeat(g[:(n + 7) // 8], 8, axis=0)[:n])
    elif kind == "near_duplicates":
        g = (np.repeat(g[:(n + 7) // 8], 8, axis=0)[:n].astype(np.float64) * (1 + 1e-6 * rng.standard_normal((n, d)))).astype(np.float32)
    elif kind == "zero_rows":
        g[rng.random(n) < 0.5] = 0.0
        g[0] = 0.0
    elif kind == "huge_coordinate":
        g[:, -1] *= 1e4
    elif kind == "tiny":
        g = (g * 1e-15).astype(np.float32)
    elif kind == "large":
        g = (g * 1e15).astype(np.float32)
    g.setflags(write=False)
    return g


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------------
def split(E, truncate=False):
    """fp32 -> (hi, lo) as dist_split_kernel: hi = bf16(e), lo = bf16(e - hi), round to nearest even (truncate: the planted mistake)."""
    E = np.ascontiguousarray(E, np.float32)
    rnd = (lambda a: (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32)) if truncate else RB.bf16_round
    hi = rnd(E)
    return hi, rnd(E - hi)


def _quanta(a, what):
    m = np.asarray(a, np.float64) / Q
    assert np.array_equal(m, np.rint(m)), "%s is not a multiple of 2^-4 everywhere" % what
    return m


def expected(E):
    """(the one correct dense lower triangle [n][n] fp32 -- +0 above the diagonal --, shares) of rows E, with the conditions that make
    equality legitimate asserted.  All arithmetic is on integers held in float64 (every sum is far below 2^53)."""
    E = np.ascontiguousarray(E, np.float32)
    n, d = E.shape
    hi, lo = split(E)
    assert np.array_equal(hi.astype(np.float64) + lo, E.astype(np.float64)), "e != hi + lo for %d coordinates" % int((hi.astype(np.float64) + lo != E).sum())
    m, mh, ml = _quanta(E, "E"), _quanta(hi, "hi"), _quanta(lo, "lo")
    mag = np.abs(mh) + np.abs(ml)
    span = float((mag @ mag.T)[~np.eye(n, dtype=bool)].max(initial=0.0))  # pairs i != j: the diagonal's accumulator is never stored
    assert span < SPAN, "max sum (|hi| + |lo|)(|hi| + |lo|) = %.0f quanta, not below 2^22" % span
    nrm = (m * m).sum(axis=1)
    assert float(nrm.max(initial=0.0)) < 2.0 ** 23, "a row norm of %.0f quanta, not below 2^23" % nrm.max()
    lolo = ml @ ml.T
    plain = nrm[:, None] + nrm[None, :] - 2.0 * (m @ m.T)   # |a - b|^2, i.e. 0.5 |a - b|^2 in units of 2^-9
    v = plain + 2.0 * lolo                                     # 0.5 (|a|^2 + |b|^2) - (a.b - la.lb) in units of 2^-9
    below = np.tri(n, n, -1, dtype=bool)
    out = np.where(below & (v > 0), v, 0.0) * 2.0 ** -9        # the clamp to +0, the diagonal +0
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(np.float64), out), "%d values are not representable in fp32" % int((out32.astype(np.float64) != out).sum())
    pairs = max(int(below.sum()), 1)
    shares = {"lo_nonzero": float((lo != 0).mean()) if E.size else 0.0, "lolo_pairs": float((below & (lolo != 0)).sum()) / pairs,
              "clamped": int((below & (v < 0)).sum()), "not_plain": int((below & (np.maximum(v, 0.0) != plain)).sum())}
    return out32, shares


def kernel_model(E, mistake=None):
    """dist_split_kernel + dist_mfma_kernel<1> in numpy -> the dense lower triangle [n][n] fp32: rows padded to dp (a multiple of 64, at
    least 64), the split, the norms sum e^2 in fp32, ONE product of A' = [hi | hi | lo] with B' = [hi | lo | hi] over K' = 3 dp in k-steps
    of 64 with an fp32 accumulator, 0.5 (n_i + n_j) - c, the clamp, the diagonal.  (The order inside a k-step and inside the norm's tree
    is not restated: on exact_rows it cannot matter.)  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    E = np.ascontiguousarray(E, np.float32)
    n, d = E.shape
    dp = max((d + 63) // 64 * 64, 64)
    P = np.zeros((n, dp), np.float32)
    P[:, :d] = E
    if mistake == "pad_not_zero":  # columns d..dp read on in memory: the next rows' data (zeros behind the last row)
        flat = np.concatenate([E.ravel(), np.zeros(dp, np.float32)])
        P = np.stack([flat[r * d:r * d + dp] for r in range(n)])
    hi, lo = split(P, truncate=mistake == "truncating_split")
    if mistake == "lo_ignored":
        lo = np.zeros_like(lo)
    nrm = ((hi * hi) if mistake == "norms_from_hi" else (P * P)).sum(axis=1, dtype=np.float32)
    z = np.zeros_like(lo)
    A = np.concatenate([hi, hi, z if mistake == "dropped_segment" else lo] + ([lo] if mistake == "lolo_included" else []), axis=1).astype(np.float64)
    B = np.concatenate([hi, lo, hi] + ([lo] if mistake == "lolo_included" else []), axis=1).astype(np.float64)
    if mistake == "neighbour_row":  # the last row of every tile stages the row behind it (zeros behind the last one)
        last = np.arange(TILE - 1, n, TILE)
        A[last] = np.concatenate([A, np.zeros((1, A.shape[1]))])[last + 1]
    K = A.shape[1] - (64 if mistake == "dropped_last_kstep" else 0)
    acc = np.zeros((n, n), np.float32)
    for k0 in range(0, K, 64):
        acc = (acc + (A[:, k0:k0 + 64] @ B[:, k0:k0 + 64].T).astype(np.float32)).astype(np.float32)
    v = np.float32(0.5) * (nrm[:, None] + nrm[None, :]) - acc
    assert v.dtype == np.float32
    if mistake == "no_clamp":
        out = v
    elif mistake == "negative_zero_kept":  # "v * (v > 0)": a negative estimate times 0 is -0
        out = np.where(v > 0, v, np.where(v == v, v * np.float32(0.0), v))
    else:
        out = np.where(v > 0, v, np.where(v == v, np.float32(0.0), v))
    if mistake != "diagonal_not_zero":
        out = np.where(np.eye(n, dtype=bool), np.float32(0.0), out)
    return np.where(np.tri(n, n, 0, dtype=bool), out, np.float32(0.0)).astype(np.float32)


# ---- the comparison -----------------------------------------------------------------------------------------------------------
def _where(i, j):
    edge = lambda r, name: ", first %s of the tile" % name if r % TILE == 0 else (", last %s of the tile" % name if r % TILE == TILE - 1 else "")
    return "tile (%d, %d)%s%s" % (i // TILE, j // TILE, edge(i, "row"), edge(j, "column"))


def same_bits(got, want, what="D"):
    """None if the two fp32 arrays [n][m] agree bit for bit (-0 is not +0, a NaN equals only its own payload), else the failure message:
    the count, the first (i, j) with both bit patterns, the 128-tile it sits in and whether it is on the tile's first or last row or column."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape and got.ndim == 2, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if not len(bad):
        return None
    i, j = int(bad[0][0]), int(bad[0][1])
    return "%s: %d of %d entries differ, first at (i, j) = (%d, %d): got 0x%08x (%r), wanted 0x%08x (%r), %s" % (
        what, len(bad), got.size, i, j, int(got.view(np.uint32)[i, j]), float(got[i, j]), int(want.view(np.uint32)[i, j]), float(want[i, j]), _where(i, j))


def assert_same_bits(got, want, what="D"):
    msg = same_bits(got, want, what)
    assert msg is None, msg


SENTINEL = 0x7FC0D157  # a quiet NaN with a payload: what every cell of the output buffer holds before the call


def buffer_report(buf, n, ld, want, what="D"):
    """The whole output buffer of icl_distance_mfma_dev (uint32, at least n * ld words, prefilled with SENTINEL) against the dense lower
    triangle `want` [n][n]: entries j <= i must have want's bits, EVERY other cell -- above the diagonal, the pad columns n..ld, whatever
    follows the last row -- must still hold the sentinel.  None, or the failure message."""
    buf = np.ascontiguousarray(buf, np.uint32).ravel()
    assert buf.size >= n * ld and ld >= n
    rows = buf[:n * ld].reshape(n, ld)
    lower = np.tri(n, ld, 0, dtype=bool)
    msg = same_bits(np.where(lower[:, :n], rows[:, :n], 0).view(np.float32), np.where(lower[:, :n], np.ascontiguousarray(want, np.float32).view(np.uint32), 0).view(np.float32), what)
    if msg:
        return msg
    touched = np.argwhere(~lower & (rows != SENTINEL))
    if len(touched):
        i, j = int(touched[0][0]), int(touched[0][1])
        return "%s: %d cells outside the lower triangle were written, first at (i, j) = (%d, %d) of pitch %d: 0x%08x, %s%s" % (
            what, len(touched), i, j, ld, int(rows[i, j]), _where(i, j), ", a pad column" if j >= n else "")
    tail = np.flatnonzero(buf[n * ld:] != SENTINEL)
    if len(tail):
        return "%s: %d words behind the last row were written, first %d words past the end" % (what, len(tail), int(tail[0]))
    return None


# ---- bounds on ordinary floats -----------------------------------------------------------------------------------------------------
SPLIT_COEFF = 3.01 * 2.0 ** -16  # |a.b - (ha.hb + ha.lb + la.hb)| <= SPLIT_COEFF sum |a_k b_k|: e - hi = lo + r with |lo + r| <= 2^-8 |e|, |r| <= 2^-16 |e|,
                                 # and what is left out is la.lb + ra.b + (a - ra).rb: three terms of at most 2^-16 |a_k b_k| each (1 % for the second order)


def three_products(E):
    """(a.b, ha.hb + ha.lb + la.hb, sum |a_k b_k|) for all pairs, in float64."""
    hi, lo = (a.astype(np.float64) for a in split(E))
    e = np.asarray(E, np.float64)
    return e @ e.T, hi @ hi.T + hi @ lo.T + lo @ hi.T, np.abs(e) @ np.abs(e).T


def reference(E):
    """0.5 |a - b|^2 in GEMM form in float64 (its own error, about d * 2^-53 of the scale, is far below every bound here), the scale
    0.5 (|a|^2 + |b|^2) and sum |a_k b_k|."""
    e = np.asarray(E, np.float64)
    sq = (e * e).sum(axis=1)
    scale = 0.5 * (sq[:, None] + sq[None, :])
    return scale - e @ e.T, scale, np.abs(e) @ np.abs(e).T


def error_bound(E):
    """B_ij of tests/test_dist_exact_gpu.py:
        (3.01 * 2^-16 + 2 * 3 dp * 2^-24) sum |a_k b_k|  +  ((ceil(dp / 256) + 10) + 3) * 2^-24 * 0.5 (|a|^2 + |b|^2)
    the split; each of the 3 dp accumulations of a product off by at most 2^-23 of the running sum, rounded or truncated (an ASSUMPTION:
    the matrix cores' internal accumulation is not specified); the norms (one square, ceil(dp / 256) - 1 additions per thread, six shuffle
    steps and two adds of the four wave sums: at most ceil(dp / 256) + 10 roundings) and the three fp32 operations of 0.5 (n_i + n_j) - c."""
    d = np.asarray(E).shape[1]
    dp = max((d + 63) // 64 * 64, 64)
    _, scale, absdot = reference(E)
    return (SPLIT_COEFF + 2 * 3 * dp * 2.0 ** -24) * absdot + ((math.ceil(dp / 256) + 10) + 3) * 2.0 ** -24 * scale
