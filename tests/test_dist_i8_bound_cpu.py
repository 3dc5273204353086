"""The bound arithmetic of dist_bound_i8_kernel's epilogue (imageclust_amd/csrc/dist_i8_bound.h) on the CPU: tests/dist_i8_bound_main.cpp, a
stand-alone program (its own main) that includes the header alone, built with a plain host C++17 compile and run as a child process on the
cases below.  Its E_ab -- the separable form s_a p_b + s_b p_a + s_a s_b C_D + kappa n_a + kappa n_b -- is compared with the header comment
of distance_i8.hip, m_ab + 16 u (1 + 64 u)(n_a + n_b), evaluated in exact rational arithmetic on the same inputs: never below it, and above
it by no more than the (1 + 1e-12) factor and its own roundings.  L and U are checked against the chain (T -+ E_ab) they stand for, in exact
arithmetic on the program's own T and E_ab: 0 <= L <= max(0, (T - E_ab)(1 - g')), L within its two safety factors and one float rounding of
that value, and U(L) >= (T + E_ab)(1 + g').  No GPU."""
import os
import shutil
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc")) or "/opt/rocm/bin/hipcc"
LIMIT_S = 300
U24 = Fr(1, 1 << 24)
KAPPA = 16 * U24 * (1 + 64 * U24)


def gprime(d):
    """g' of the bound (ward.hip): (1 + u)^(D + 2) - 1, rounded up, as the float the kernel gets."""
    return float(np.float32(((1.0 + 2.0 ** -24) ** (d + 2) - 1.0) * (1 + 1e-6)))


def cases():
    """(e_a, e_b, L1_a, L1_b, n_a, n_b, D, I): e None = a zero row.  Random rows, the extremes of the exponents, zero rows, D = 1 and 2048,
    L1 at its maximum D s, dot products of both signs and at the Cauchy-Schwarz limit."""
    rng = np.random.default_rng(20250613)
    f32 = lambda v: float(np.float32(v))
    out = []

    def row(e, d, full=False):
        if e is None:
            return 0.0, 0.0
        s = 2.0 ** e
        l1 = f32(d * s if full else rng.uniform(0, d * s))
        return l1, f32(rng.uniform(0.0, d * s * s))

    def add(ea, eb, d, full=False, sign=1, tight=False):
        (l1a, na), (l1b, nb) = row(ea, d, full), row(eb, d, full)
        imax = d << 26  # |sum A_k B_k| <= D 2^40, of which I carries the classes from 2^14 up
        if ea is None or eb is None:
            I = 0
        elif tight:  # c = (n_a + n_b) / 2, as for a = b: T = 0 up to rounding, T - E_ab < 0
            I = int(min(imax, (na + nb) / 2 / (2.0 ** (ea + eb - 26))))
        else:  # |c| <= sqrt(n_a n_b) (Cauchy-Schwarz) and |I| within its range
            I = sign * int(min(imax, rng.uniform(0, 1) * np.sqrt(na * nb) / (2.0 ** (ea + eb - 26))))
        out.append((ea, eb, l1a, l1b, na, nb, d, I))

    for d in (1, 64, 100, 2048):
        for _ in range(40):
            add(int(rng.integers(-12, 12)), int(rng.integers(-12, 12)), d, sign=int(rng.choice([-1, 1])))
        for ea, eb in ((-60, -60), (50, 50), (-60, 50), (50, -60), (0, 0), (1, -1)):
            add(ea, eb, d)
            add(ea, eb, d, full=True, sign=-1)
            add(ea, eb, d, tight=True)
        for ea, eb in ((None, None), (None, 3), (-60, None), (50, None)):
            add(ea, eb, d)
    return out


def exact_eab(ea, eb, l1a, l1b, na, nb, d):
    """m_ab + 16 u (1 + 64 u)(n_a + n_b) of distance_i8.hip's header comment, exactly."""
    sa, sb = (Fr(2) ** ea if ea is not None else Fr(0)), (Fr(2) ** eb if eb is not None else Fr(0))
    t21, t40 = Fr(1, 1 << 21), Fr(1, 1 << 40)
    m = t21 * (sa * (Fr(l1b) + d * sb * t21) + sb * Fr(l1a)) + sa * sb * t40 * d * ((1 << 20) + (1 << 12))
    return m + KAPPA * (Fr(na) + Fr(nb)), sa, sb


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    assert os.path.exists(HIPCC), "no hipcc: its clang is the host compiler"
    exe = str(tmp_path_factory.mktemp("dist_i8_bound") / "dist_i8_bound")
    r = subprocess.run([HIPCC, "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "dist_i8_bound_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, r.stderr[-3000:]
    cs = cases()
    text = "".join("%s %s %s %s %s %s %d %d %s\n" % ("z" if ea is None else ea, "z" if eb is None else eb, l1a.hex(), l1b.hex(), na.hex(), nb.hex(), d, I,
                                                   gprime(d).hex()) for (ea, eb, l1a, l1b, na, nb, d, I) in cs)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=LIMIT_S)
    assert r.returncode == 0, "exit %d\n%s" % (r.returncode, r.stderr[-3000:])
    rows = [tuple(float.fromhex(v) for v in ln.split()) for ln in r.stdout.strip().split("\n")]
    assert len(rows) == len(cs) and r.stderr.strip() == "%d cases" % len(cs)
    return list(zip(cs, rows))


def test_cases_cover_the_extremes():
    cs = cases()
    assert {c[6] for c in cs} == {1, 64, 100, 2048}
    assert any(c[0] == -60 and c[1] == 50 for c in cs) and any(c[0] is None and c[1] is None for c in cs) and any(c[0] is None and c[1] is not None for c in cs)
    assert any(c[0] is not None and c[2] == float(np.float32(c[6] * 2.0 ** c[0])) for c in cs)  # L1 = D s
    assert any(c[7] < 0 for c in cs) and any(c[7] > 0 for c in cs)


def test_eab_is_never_below_the_exact_bound_and_not_looser(results):
    for (ea, eb, l1a, l1b, na, nb, d, I), (E, T, L, U) in results:
        want, sa, sb = exact_eab(ea, eb, l1a, l1b, na, nb, d)
        assert Fr(E) >= want, (ea, eb, d, E, float(want))
        assert Fr(E) <= want * (1 + Fr(2, 10 ** 12)), (ea, eb, d, E, float(want))  # the (1 + 1e-12) factor and a few units of 2^-53
        t = (Fr(na) + Fr(nb)) / 2 - sa * sb * Fr(1, 1 << 26) * I
        assert abs(Fr(T) - t) <= Fr(1, 1 << 51) * ((Fr(na) + Fr(nb)) / 2 + abs(sa * sb * Fr(1, 1 << 26) * I)), (ea, eb, d, T, float(t))


def test_lower_and_upper_bracket_the_chain(results):
    claims = clamped = 0
    for (ea, eb, l1a, l1b, na, nb, d, I), (E, T, L, U) in results:
        g = Fr(gprime(d))
        lo, hi = (Fr(T) - Fr(E)) * (1 - g), (Fr(T) + Fr(E)) * (1 + g)
        assert L >= 0 and Fr(L) <= max(Fr(0), lo), (ea, eb, d, L, float(lo))
        assert np.float32(L) == L and np.float32(U) == U
        if lo > Fr(1, 10 ** 29):  # a claim is made, and it is the chain's value less two safety factors and one float rounding
            assert Fr(L) >= lo * (1 - Fr(2, 10 ** 12)) * (1 - Fr(1, 1 << 23)), (ea, eb, d, L, float(lo))
            claims += 1
        else:
            clamped += int(L == 0)
        assert Fr(U) >= hi, (ea, eb, d, U, float(hi))
        assert Fr(U) <= (Fr(L) * (1 + 3 * g) + Fr(20001, 10000) * Fr(E) + Fr(2, 10 ** 30)) * (1 + 2 * g) * (1 + Fr(1, 1 << 22)), (ea, eb, d, U)
    assert claims >= 100 and clamped >= 20, (claims, clamped)
