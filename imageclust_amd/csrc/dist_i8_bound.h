// dist_i8_bound.h -- the bound arithmetic of dist_bound_i8_kernel's epilogue (distance_i8.hip, whose header comment has the proof): the
// per-row factors, E_ab in separable form, the stored lower bound L and the scan-side upper bound U(L).  Plain C++ in double, no HIP
// type: a host compile can include it, and tests/dist_i8_bound_main.cpp evaluates it on the CPU against exact rational arithmetic.
// (ward.hip's wupper keeps its own float form of E_ab for the scans.)
//
// The unit that includes it is compiled with the default -ffp-contract: a contracted a * b + c drops a rounding, it never adds one, and
// every rounding of these expressions is paid for by the (1 +- 1e-12) factors below.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DI8B_HD __host__ __device__ __forceinline__
#else
#define DI8B_HD inline
#endif

#define DI8B_NOEXP INT32_MIN              /* ex[] of a row that is all zeros or not finite: s counts as 0 */
#define DI8B_MAXF 3.40282346638528859811704183484516925e+38f/* "no claim" (ICL_MAXF) */

// kappa = 16 u (1 + 64 u), u = 2^-24: the share of E_ab that the computed norms, the centring and the conversions take per unit of n_a + n_b
DI8B_HD double di8_kappa() { return 16.0 * 5.9604644775390625e-08 * (1.0 + 64.0 * 5.9604644775390625e-08); }

// s = 2^e from the integer exponent (e = DI8B_NOEXP: 0).  e is a float's frexp exponent, -148 .. 128: always a normal double.
DI8B_HD double di8_pow2(int e)
{
    const uint64_t bits = e == DI8B_NOEXP ? 0ull : (uint64_t)(unsigned)(e + 1023) << 52;
    double s;
    memcpy(&s, &bits, sizeof s);
    return s;
}

// What the bound needs of one row a: s_a (or 0), s_a 2^-26 (the scale of the integer dot product), 2^-21 L1_a, kappa n_a, n_a.
// Scalings by powers of two are exact; kappa n_a is the one rounding in here.
struct di8_side {
    double s, s26, p, k, n;
};
DI8B_HD di8_side di8_side_of(int e, float l1, float nrm)
{
    di8_side r;
    r.s = di8_pow2(e);
    r.s26 = r.s * 1.4901161193847656e-08;         // 2^-26
    r.p = (double)l1 * 4.76837158203125e-07;      // 2^-21
    r.n = (double)nrm;
    r.k = di8_kappa() * r.n;
    return r;
}

// C_D = D 2^-42 + D (2^20 + 2^12) 2^-40: the second-order term of the two roundings to 21 bits and the digit classes left out, per
// unit of s_a s_b.  Exact in double for D <= 2048 (D (2^22 + 2^14 + 1) has 34 bits).
DI8B_HD double di8_cd(int d) { return (double)d * 2.2737367544323206e-13 + (double)d * (1048576.0 + 4096.0) * 9.094947017729282e-13; }

// E_ab = s_a (2^-21 L1_b) + s_b (2^-21 L1_a) + s_a s_b C_D + kappa n_a + kappa n_b: the header's m_ab + 16 u (1 + 64 u)(n_a + n_b) with the
// row and column factors taken out.  The first three products are exact or carry one rounding each (s is a power of two), the sums
// round: at most six roundings of non-negative terms, i.e. a relative error below 7 * 2^-53, against the factor (1 + 1e-12).
DI8B_HD double di8_eab(const di8_side &a, const di8_side &b, double cd)
{
    return (a.s * b.p + b.s * a.p + (a.s * b.s) * cd + (a.k + b.k)) * (1.0 + 1e-12);
}

// T = (n_a + n_b) / 2 - c,  c = 2^(e_a + e_b - 26) I  (I = 128 hi + lo, exact in double: < 2^38; the scaling is exact)
DI8B_HD double di8_T(const di8_side &a, const di8_side &b, double I) { return 0.5 * (a.n + b.n) - (a.s26 * b.s) * I; }

// Directed roundings of a POSITIVE double to float, without a branch: round to nearest, then step one float towards the side wanted
// where the nearest float lies on the other side (a positive float's neighbours are its bit pattern -+ 1).  v beyond FLT_MAX: the
// nearest float is inf, the step below it FLT_MAX.  Callers discard the result for v <= 0 and NaN.
DI8B_HD float di8_f32_rz_pos(double v) // the largest float not above v
{
    const float f = (float)v;
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    u -= (double)f > v ? 1u : 0u;
    float r;
    memcpy(&r, &u, sizeof r);
    return r;
}
DI8B_HD float di8_f32_ru_pos(double v) // the smallest float not below v (v <= FLT_MAX)
{
    const float f = (float)v;
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    u += (double)f < v ? 1u : 0u;
    float r;
    memcpy(&r, &u, sizeof r);
    return r;
}

// The stored lower bound: (T - E_ab)(1 - g'), pushed down against this expression's own double roundings and rounded toward zero;
// 0 ("no claim") in the subnormal range and for overflowing norms (also NaN).  The caller sets the sign bit.
DI8B_HD float di8_lower(double T, double Eab, double ns, double gam)
{
    const double Ld = (T - Eab) * (1.0 - gam) * (1.0 - 1e-12);
    const float L = di8_f32_rz_pos(Ld);
    return (Ld > 1e-30 && ns < 1e37) ? L : 0.0f;
}

// The scans' upper bound from the stored L: R <= (T + E_ab)(1 + g') and T - E_ab <= L (1 + 2 g') (or <= 1e-30 where L was clamped
// to 0), in double, rounded up; DI8B_MAXF where it overflows (inf / NaN: no claim).
DI8B_HD float di8_upper(float L, double Eab, double gam)
{
    const double U = ((double)L * (1.0 + 3.0 * gam) + 2.0001 * Eab + 2e-30) * (1.0 + 2.0 * gam);
    const float Uf = di8_f32_ru_pos(U); // (U >= 2e-30)
    return U < 3.0e38 ? Uf : DI8B_MAXF;
}
