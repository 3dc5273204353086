// A stand-alone program around imageclust_amd/csrc/dist_i8_bound.h (the bound arithmetic of dist_bound_i8_kernel's epilogue), built by
// tests/test_dist_i8_bound_cpu.py with a plain host C++17 compile.  One case per line of standard input:
//     e_a e_b L1_a L1_b n_a n_b D I g'
// (e: the row's exponent, or "z" for a zero row; L1, n: floats; I = 128 hi + lo: an integer; floating-point values in C99 hex notation)
// and per case one line of output: E_ab, T, L, U(L) in hex notation -- exactly what the epilogue computes for that pair.
#include "../imageclust_amd/csrc/dist_i8_bound.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

int main()
{
    char ea[64], eb[64], l1a[64], l1b[64], na[64], nb[64], gs[64];
    int d;
    long long I;
    int n = 0;
    while (scanf("%63s %63s %63s %63s %63s %63s %d %lld %63s", ea, eb, l1a, l1b, na, nb, &d, &I, gs) == 9) {
        const int xa = strcmp(ea, "z") ? atoi(ea) : DI8B_NOEXP, xb = strcmp(eb, "z") ? atoi(eb) : DI8B_NOEXP;
        const di8_side a = di8_side_of(xa, strtof(l1a, nullptr), strtof(na, nullptr));
        const di8_side b = di8_side_of(xb, strtof(l1b, nullptr), strtof(nb, nullptr));
        const double gam = (double)strtof(gs, nullptr);
        const double E = di8_eab(a, b, di8_cd(d)), T = di8_T(a, b, (double)I);
        const float L = di8_lower(T, E, a.n + b.n, gam), U = di8_upper(L, E, gam);
        printf("%a %a %a %a\n", E, T, (double)L, (double)U);
        ++n;
    }
    fprintf(stderr, "%d cases\n", n);
    return 0;
}
