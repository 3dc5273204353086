// pairs_between_plan.h -- the host arithmetic of icl_pairs_between (pairs_between.hip): what ICL_ERR_ARG covers, the prefix over the count
// pass's per-segment counts, a hit's rank inside its tile's 128-bit row mask, and the body of icl_pairs_between_from_matrix.  Plain C++
// with no HIP in it: tests/pairs_between_main.cpp compiles it with the host compiler alone, under the sanitizers.  pb_mask_rank is also
// what the fill kernel calls, so the place of a hit is stated once.
#pragma once
#include <cstdint>

#include "pairs_select.h"

#define PB_ROWS 128 // rows of a band, columns of a tile (DT_TILE of ward_exact_tile.h; pairs_between.hip asserts that they agree)

// What ICL_ERR_ARG covers apart from the operands' pointers, shared by the three forms: the reason, or nullptr.
inline const char *pb_bad_arg(int64_t nq, int64_t n, float threshold, const int32_t *q_size, const int32_t *l_size, const int64_t *exclude,
                              const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (nq < 0 || n < 0) return "negative nq or n";
    if (n >= (1LL << 31)) return "n must be below 2^31";
    if (threshold != threshold) return "the threshold is NaN";
    if (cap < 0) return "negative cap";
    if (!row_ptr || !total) return "a null pointer";
    if ((!col || !val) && (col || val || cap != 0)) return "col and val may be null only together and with cap == 0 (the size query)";
    for (int64_t i = 0; q_size && i < nq; ++i)
        if (q_size[i] <= 0) return "a q_size entry is not above 0";
    for (int64_t j = 0; l_size && j < n; ++j)
        if (l_size[j] <= 0) return "an l_size entry is not above 0";
    for (int64_t i = 0; exclude && i < nq; ++i)
        if (exclude[i] < -1 || exclude[i] >= n) return "an exclude entry is outside [-1, n)";
    return nullptr;
}

// The prefix over the count pass's figures, in (i, s) order: seg_count[i * splits + s] hits of query i in split s's column range ->
// seg_ptr[i * splits + s], the place of that segment's first hit (nq * splits + 1 entries, the last one the total),
// row_ptr[i] = seg_ptr[i * splits] (nq + 1 entries) and *total.  Splits are column ranges in ascending order, so row i's segments laid
// end to end in s order are row i ascending in j.
inline void pb_prefix(int64_t nq, int splits, const int32_t *seg_count, int64_t *seg_ptr, int64_t *row_ptr, int64_t *total)
{
    int64_t p = 0;
    for (int64_t i = 0; i < nq; ++i) {
        row_ptr[i] = p;
        for (int s = 0; s < splits; ++s) {
            seg_ptr[i * splits + s] = p;
            p += seg_count[i * splits + s];
        }
    }
    seg_ptr[nq * splits] = p;
    row_ptr[nq] = p;
    *total = p;
}

// The hits of a row in one tile are bit c (0 .. 127, the column inside the tile) of four 32-bit words: the number of hits of lower
// column than c.  A hit's place in col / val is  seg_ptr[i * splits + s] + (the row's hits in the segment's tiles walked before) + this.
PS_HD int pb_mask_rank(const uint32_t m[4], int c)
{
    const int w = c >> 5;
    int r = __builtin_popcount(m[w] & ((1u << (c & 31)) - 1u));
    for (int q = 0; q < 4; ++q)
        if (q < w) r += __builtin_popcount(m[q]);
    return r;
}

// The body of icl_pairs_between_from_matrix: the rule (ps_listed_between), the CSR layout and the capacity convention on values the caller
// holds.  Returns 0 (ICL_OK) or -1 (ICL_ERR_ARG, nothing written unless *total > cap: then row_ptr and *total are complete).
inline int pb_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, float threshold, const int64_t *exclude, int64_t *row_ptr,
                          int32_t *col, float *val, int64_t cap, int64_t *total)
{
    if (pb_bad_arg(nq, n, threshold, nullptr, nullptr, exclude, row_ptr, col, val, cap, total) || ld < n || (nq > 0 && n > 0 && !D)) return -1;
    int64_t t = 0;
    for (int64_t i = 0; i < nq; ++i)
        for (int64_t j = 0; j < n; ++j) t += ps_listed_between(j, exclude ? exclude[i] : -1, D[i * ld + j], threshold) ? 1 : 0;
    const bool fits = t <= cap;
    int64_t p = 0;
    for (int64_t i = 0; i < nq; ++i) {
        row_ptr[i] = p;
        for (int64_t j = 0; j < n; ++j)
            if (ps_listed_between(j, exclude ? exclude[i] : -1, D[i * ld + j], threshold)) {
                if (fits) {
                    col[p] = (int32_t)j;
                    val[p] = D[i * ld + j];
                }
                ++p;
            }
    }
    row_ptr[nq] = p;
    *total = p;
    return fits || (!col && !val) ? 0 : -1;
}
