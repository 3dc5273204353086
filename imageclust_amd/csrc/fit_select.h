// fit_select.h -- the rules of icl_cluster_fit (include/imageclust.h) that are not arithmetic, stated once for the host and the device:
// which library columns a row's alternatives never see, and the packed keys under which an integer minimum / maximum picks a
// cluster's representative and worst row.  fit.hip's band walk, its reduction kernels and icl_cluster_fit_from_matrix all call the
// functions below; what a row's list keeps and in which order stays nearest_select.h's business (ns_left_out, ns_insert, ns_fill_tail).
// The from_matrix body lives here too, as plain host code, so that tests/fit_select_main.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#include "nearest_select.h"

#define FS_KMAX NS_KMAX /* k_alt is 0 .. 64 */

// c_size carries the seeded API's sign: s > 0 a cluster of s items, s < 0 a frozen cluster of -s items.
NS_HD bool fs_frozen(int32_t c_size) { return c_size < 0; }
NS_HD int64_t fs_items(int32_t c_size) { return c_size < 0 ? -(int64_t)c_size : (int64_t)c_size; }

// The columns row i's alternatives never see: its own cluster (own, -1: none), every frozen cluster, and nearest_select.h's size ban.
NS_HD bool fs_left_out(int64_t j, int64_t own, int64_t q_size, int32_t c_size, int32_t max_size)
{
    return fs_frozen(c_size) || ns_left_out(j, own, q_size, (int64_t)c_size, max_size);
}

// The ordered bit image of an own cost: u32 values that compare as the floats do with `<` (-0 and +0 are one value), every NaN on top.
NS_HD uint32_t fs_ordered_bits(float v)
{
    if (v != v) return 0xffffffffu;
    if (v == 0.0f) return 0x80000000u;
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Keys of (own cost, row), row < 2^31.  The MINIMUM of a cluster's fs_key_rep is its representative: smallest cost, numbers before
// NaN, ties to the lowest row.  The MAXIMUM of its fs_key_worst is its worst row: largest cost, NaN above every number, ties to the
// lowest row again (the row is stored inverted).  No real key equals an empty value: the image of a number is never 0, a row never
// 2^32 - 1.
#define FS_REP_EMPTY 0xffffffffffffffffull
#define FS_WORST_EMPTY 0ull
NS_HD uint64_t fs_key_rep(float own, int64_t row) { return ((uint64_t)fs_ordered_bits(own) << 32) | (uint32_t)row; }
NS_HD uint64_t fs_key_worst(float own, int64_t row) { return ((uint64_t)fs_ordered_bits(own) << 32) | (uint32_t)~(uint32_t)row; }
NS_HD int32_t fs_rep_row(uint64_t key) { return key == FS_REP_EMPTY ? -1 : (int32_t)(uint32_t)key; }
NS_HD int32_t fs_worst_row(uint64_t key) { return key == FS_WORST_EMPTY ? -1 : (int32_t)~(uint32_t)key; }

// What ICL_ERR_ARG covers apart from the pointers: the reason, or nullptr.  (Host.)
inline const char *fs_bad_arg(int64_t nq, int64_t K, int32_t k_alt, const int32_t *q_size, const int32_t *cluster_of, const int32_t *c_size)
{
    if (nq < 0 || K < 0) return "negative nq or K";
    if (K >= (1LL << 31) || nq >= (1LL << 31)) return "nq and K must be below 2^31";
    if (k_alt < 0 || k_alt > FS_KMAX) return "k_alt must be 0 .. 64";
    if (nq > 0 && !cluster_of) return "cluster_of is null";
    for (int64_t i = 0; q_size && i < nq; ++i)
        if (q_size[i] <= 0) return "a q_size entry is not above 0";
    for (int64_t j = 0; c_size && j < K; ++j)
        if (c_size[j] == 0) return "a c_size entry is 0";
    for (int64_t i = 0; i < nq; ++i)
        if (cluster_of[i] < -1 || cluster_of[i] >= K) return "a cluster_of entry is outside [-1, K)";
    return nullptr;
}

// icl_cluster_fit_from_matrix: the rules above applied to values the caller holds, D[i * ld + j] pair (i, j)'s.  Returns false, with
// nothing written, for the arguments ICL_ERR_ARG covers.  (Host.)
inline bool fs_fit_from_matrix(const float *D, int64_t nq, int64_t K, int64_t ld, const int32_t *q_size, const int32_t *cluster_of,
                               const int32_t *c_size, int32_t k_alt, int32_t max_size, float *own, int32_t *alt_idx, float *alt_val,
                               int32_t *listed, int32_t *rep, int32_t *worst)
{
    if (fs_bad_arg(nq, K, k_alt, q_size, cluster_of, c_size) || ld < K) return false;
    if (nq > 0 && (!own || (k_alt > 0 && (!alt_idx || !alt_val)) || (K > 0 && !D))) return false;
    for (int64_t j = 0; j < K; ++j) {
        if (listed) listed[j] = 0;
        if (rep) rep[j] = -1;
        if (worst) worst[j] = -1;
    }
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t c = cluster_of[i], sq = q_size ? q_size[i] : 1;
        own[i] = c < 0 ? NS_MAXF : D[i * ld + c];
        if (k_alt > 0) {
            float *rv = alt_val + i * k_alt;
            int32_t *rj = alt_idx + i * k_alt;
            int cnt = 0;
            for (int64_t j = 0; j < K; ++j)
                if (!fs_left_out(j, c, sq, c_size ? c_size[j] : 1, max_size)) ns_insert(rv, rj, k_alt, cnt, D[i * ld + j], (int32_t)j);
            ns_fill_tail(rv, rj, k_alt, cnt);
        }
        if (c < 0) continue;
        if (listed) ++listed[c];
        // (rep / worst hold rows here, so the keys are rebuilt from them: the same comparisons the device's atomics make)
        if (rep && (rep[c] < 0 || fs_key_rep(own[i], i) < fs_key_rep(own[rep[c]], rep[c]))) rep[c] = (int32_t)i;
        if (worst && (worst[c] < 0 || fs_key_worst(own[i], i) > fs_key_worst(own[worst[c]], worst[c]))) worst[c] = (int32_t)i;
    }
    return true;
}
