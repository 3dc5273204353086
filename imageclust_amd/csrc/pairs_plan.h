// pairs_plan.h -- the host arithmetic of the two threshold joins of pairs.hip, icl_pairs_within and icl_pairs_between: what ICL_ERR_ARG
// covers, the empty result, the prefix over the count pass's figures, a hit's rank inside its tile's 128-bit row mask, and the body of
// the two _from_matrix entry points.  Plain C++ with no HIP in it: tests/pairs_plan_main.cpp compiles it with the host compiler alone,
// under the sanitizers.  pairs_mask_rank is also what the fill kernel calls, so the place of a hit is stated once.  Which pairs are
// listed is pairs_select.h's business alone; the two rule objects below only say which columns of a row are offered to it.
#pragma once
#include <cstdint>

#include "pairs_select.h"

#define PAIRS_ROWS 128 // rows of a band, columns of a tile (DT_TILE of ward_exact_tile.h; pairs.hip asserts that they agree)

// What ICL_ERR_ARG covers on the output side, shared by all six checked forms: the reason, or nullptr.
inline const char *pairs_bad_out(float threshold, const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (threshold != threshold) return "the threshold is NaN";
    if (cap < 0) return "negative cap";
    if (!row_ptr || !total) return "a null pointer";
    if ((!col || !val) && (col || val || cap != 0)) return "col and val may be null only together and with cap == 0 (the size query)";
    return nullptr;
}

// ... and what each family adds apart from the operands' pointers, shared by its three forms.
inline const char *pairs_within_bad_arg(int64_t n, float threshold, const int64_t *row_ptr, const void *col, const void *val, int64_t cap,
                                        const int64_t *total)
{
    if (n < 0) return "negative n";
    if (n >= (1LL << 31)) return "n must be below 2^31";
    return pairs_bad_out(threshold, row_ptr, col, val, cap, total);
}

inline const char *pairs_between_bad_arg(int64_t nq, int64_t n, float threshold, const int32_t *q_size, const int32_t *l_size, const int64_t *exclude,
                                         const int64_t *row_ptr, const void *col, const void *val, int64_t cap, const int64_t *total)
{
    if (nq < 0 || n < 0) return "negative nq or n";
    if (n >= (1LL << 31)) return "n must be below 2^31";
    if (const char *why = pairs_bad_out(threshold, row_ptr, col, val, cap, total)) return why;
    for (int64_t i = 0; q_size && i < nq; ++i)
        if (q_size[i] <= 0) return "a q_size entry is not above 0";
    for (int64_t j = 0; l_size && j < n; ++j)
        if (l_size[j] <= 0) return "an l_size entry is not above 0";
    for (int64_t i = 0; exclude && i < nq; ++i)
        if (exclude[i] < -1 || exclude[i] >= n) return "an exclude entry is outside [-1, n)";
    return nullptr;
}

// The result of a call with no pair to evaluate: nrows empty rows.
inline void pairs_empty(int64_t nrows, int64_t *row_ptr, int64_t *total)
{
    for (int64_t i = 0; i <= nrows; ++i) row_ptr[i] = 0;
    *total = 0;
}

// The prefix over the count pass's figures, in (i, s) order: seg_count[i * splits + s] hits of row i in split s's column range ->
// seg_ptr[i * splits + s], the place of that segment's first hit (nrows * splits + 1 entries, the last one the total),
// row_ptr[i] = seg_ptr[i * splits] (nrows + 1 entries) and *total.  Splits are column ranges in ascending order, so row i's segments laid
// end to end in s order are row i ascending in j.  icl_pairs_within has one segment per row: splits = 1, seg_ptr a copy of row_ptr.
inline void pairs_prefix(int64_t nrows, int splits, const int32_t *seg_count, int64_t *seg_ptr, int64_t *row_ptr, int64_t *total)
{
    int64_t p = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        row_ptr[i] = p;
        for (int s = 0; s < splits; ++s) {
            seg_ptr[i * splits + s] = p;
            p += seg_count[i * splits + s];
        }
    }
    seg_ptr[nrows * splits] = p;
    row_ptr[nrows] = p;
    *total = p;
}

// The hits of a row in one tile are bit c (0 .. 127, the column inside the tile) of four 32-bit words: the number of hits of lower
// column than c.  A hit's place in col / val is  seg_ptr[i * splits + s] + (the row's hits in the segment's tiles walked before) + this.
PS_HD int pairs_mask_rank(const uint32_t m[4], int c)
{
    const int w = c >> 5;
    int r = __builtin_popcount(m[w] & ((1u << (c & 31)) - 1u));
    for (int q = 0; q < 4; ++q)
        if (q < w) r += __builtin_popcount(m[q]);
    return r;
}

// What a _from_matrix form offers to pairs_select.h: columns 0 .. ncols(i) of row i, and listed(i, j, v).
struct pairs_rule_within { // the strict lower triangle
    float threshold;
    int64_t ncols(int64_t i) const { return i; }
    bool listed(int64_t i, int64_t j, float v) const { return ps_listed(i, j, v, threshold); }
};

struct pairs_rule_between { // the rectangle without each row's excluded column
    int64_t n;
    const int64_t *exclude; // may be null: none
    float threshold;
    int64_t ncols(int64_t) const { return n; }
    bool listed(int64_t i, int64_t j, float v) const { return ps_listed_between(j, exclude ? exclude[i] : -1, v, threshold); }
};

// The body of both _from_matrix entry points behind their argument checks: the rule, the CSR layout and the capacity convention on
// values the caller holds (D: nrows rows of ld floats).  Returns 0 (ICL_OK) or -1 (ICL_ERR_ARG: *total > cap with buffers given; row_ptr
// and *total are complete, col and val untouched).
template <class Rule>
inline int pairs_from_matrix(const float *D, int64_t nrows, int64_t ld, const Rule &rule, int64_t *row_ptr, int32_t *col, float *val, int64_t cap,
                             int64_t *total)
{
    int64_t t = 0;
    for (int64_t i = 0; i < nrows; ++i)
        for (int64_t j = 0; j < rule.ncols(i); ++j) t += rule.listed(i, j, D[i * ld + j]) ? 1 : 0;
    const bool fits = t <= cap;
    int64_t p = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        row_ptr[i] = p;
        for (int64_t j = 0; j < rule.ncols(i); ++j)
            if (rule.listed(i, j, D[i * ld + j])) {
                if (fits) {
                    col[p] = (int32_t)j;
                    val[p] = D[i * ld + j];
                }
                ++p;
            }
    }
    row_ptr[nrows] = p;
    *total = p;
    return fits || (!col && !val) ? 0 : -1;
}

inline int pairs_within_from_matrix(const float *D, int64_t n, int64_t ld, float threshold, int64_t *row_ptr, int32_t *col, float *val, int64_t cap,
                                    int64_t *total)
{
    if (pairs_within_bad_arg(n, threshold, row_ptr, col, val, cap, total) || ld < n || (n > 1 && !D)) return -1;
    return pairs_from_matrix(D, n, ld, pairs_rule_within{threshold}, row_ptr, col, val, cap, total);
}

inline int pairs_between_from_matrix(const float *D, int64_t nq, int64_t n, int64_t ld, float threshold, const int64_t *exclude, int64_t *row_ptr,
                                     int32_t *col, float *val, int64_t cap, int64_t *total)
{
    if (pairs_between_bad_arg(nq, n, threshold, nullptr, nullptr, exclude, row_ptr, col, val, cap, total) || ld < n || (nq > 0 && n > 0 && !D)) return -1;
    return pairs_from_matrix(D, nq, ld, pairs_rule_between{n, exclude, threshold}, row_ptr, col, val, cap, total);
}
