// apart_bits.h -- the host rules of icl_cluster_many_apart (include/imageclust.h, DESIGN.md "Constrained seeded clustering"): which
// keep-apart constraints a problem accepts, and the table its kernels then see.  One problem of m seeds carries apart_class[m] (0: none;
// two different seeds of one non-zero class are apart) and a list of (i, j) seed pairs, each apart.  The table is the BIT ROWS: m rows of
// ab_words(m) 32-bit words, bit j of row i set when seeds i and j are apart -- symmetric, zero diagonal, zero beyond column m.  The merge
// kernels of ward_many.hip keep it up to date: a merged cluster's row is the OR of its parents'.
// Host only, no HIP type and no icl_ctx: a plain host C++17 compile can include it alone, and tests/apart_bits_main.cpp checks every
// rule below on the CPU under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

inline int64_t ab_words(int64_t m) { return (m + 31) / 32; }
inline size_t ab_table_bytes(int64_t m) { return (size_t)(m * ab_words(m)) * 4; }
inline bool ab_bit(const uint32_t *rows, int64_t m, int64_t i, int64_t j) { return rows[i * ab_words(m) + (j >> 5)] >> (j & 31) & 1u; }

// What ICL_ERR_ARG covers for one problem apart from the pointers: the reason, or an empty string.  cls may be null (all 0); pairs holds
// npairs (i, j) entries, and may be null when npairs is 0.
inline std::string ab_bad_arg(int64_t m, const int32_t *cls, const int32_t *pairs, int64_t npairs)
{
    char b[160];
    if (npairs < 0) return "a negative number of pairs";
    if (npairs > 0 && !pairs) return "apart_pairs is null";
    for (int64_t i = 0; cls && i < m; ++i)
        if (cls[i] < 0) {
            snprintf(b, sizeof b, "apart_class of seed %lld is %d", (long long)i, cls[i]);
            return b;
        }
    for (int64_t q = 0; q < npairs; ++q) {
        const int32_t i = pairs[2 * q], j = pairs[2 * q + 1];
        if (i < 0 || j < 0 || i >= m || j >= m || i == j) {
            snprintf(b, sizeof b, "pair %lld is (%d, %d) in a problem of %lld seeds", (long long)q, i, j, (long long)m);
            return b;
        }
    }
    return std::string();
}

// The bit rows of a problem that ab_bad_arg accepts, into rows[m * ab_words(m)] (every word is written).  Returns whether any bit is set.
// Either order of a pair and duplicates give the same table.  A class of c members costs c (c - 1) bits, whatever m is.
inline bool ab_expand(int64_t m, const int32_t *cls, const int32_t *pairs, int64_t npairs, uint32_t *rows)
{
    const int64_t W = ab_words(m);
    for (int64_t q = 0; q < m * W; ++q) rows[q] = 0;
    bool any = false;
    auto set = [&](int64_t i, int64_t j) {
        rows[i * W + (j >> 5)] |= 1u << (j & 31);
        rows[j * W + (i >> 5)] |= 1u << (i & 31);
        any = true;
    };
    for (int64_t q = 0; q < npairs; ++q) set(pairs[2 * q], pairs[2 * q + 1]);
    if (cls) { // the members of each class, seed order within it
        std::vector<std::pair<int32_t, int32_t>> mem;
        for (int64_t i = 0; i < m; ++i)
            if (cls[i] > 0) mem.emplace_back(cls[i], (int32_t)i);
        std::sort(mem.begin(), mem.end());
        for (size_t a = 0; a < mem.size();) {
            size_t e = a;
            while (e < mem.size() && mem[e].first == mem[a].first) ++e;
            for (size_t x = a; x < e; ++x)
                for (size_t y = x + 1; y < e; ++y) set(mem[x].second, mem[y].second);
            a = e;
        }
    }
    return any;
}
