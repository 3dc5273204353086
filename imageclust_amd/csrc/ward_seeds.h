// ward_seeds.h -- the host rules that the clustering calls share, each said once: CalculateOptimalClusters (ward_optimal_k), which seeded
// problems a call accepts and what its kernels then see (ward_seed_admit: icl_cluster_seeded in ward.hip, icl_cluster_many_seeded in
// ward_many.hip), and the reference's final cluster list from a merge log (ward_final_list: every clustering call, seeded or not).
// Host only, no HIP type and no icl_ctx: a plain host C++17 compile can include it alone, and tests/ward_seeds_main.cpp checks every
// rule below on the CPU under the sanitizers.
#pragma once
#include "../../include/imageclust.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// CalculateOptimalClusters (clustering.go:168-186).  min/max < 1 divide by zero in the reference (implementation-defined int
// conversion of +Inf); rejected here.
inline int ward_optimal_k(int64_t total, int64_t min_size, int64_t max_size, int64_t *k)
{
    if (!k) return ICL_ERR_ARG;
    if (min_size < 1 || max_size < 1) return ICL_ERR_CONSTRAINT;
    if (total < min_size) return ICL_ERR_CONSTRAINT;
    const int64_t lo = (int64_t)std::ceil((double)total / (double)max_size);
    const int64_t hi = (int64_t)std::floor((double)total / (double)min_size);
    if (lo > hi) return ICL_ERR_CONSTRAINT;
    *k = lo < hi ? (lo + hi) / 2 : lo;
    return ICL_OK;
}

// One seeded problem (DESIGN.md "Seeded clustering"): m seeds, seed_size[i] items each, negative for a frozen seed (no entry is 0: the
// entry points check that with the arguments).  N = the items of all seeds.
struct ward_admission {
    int status = ICL_OK; // ICL_ERR_UNSUPPORTED: N >= 2^30, or the first unfrozen seed above max_size (the reference would split it,
                         // clustering.go:251-258); ICL_ERR_CONSTRAINT: CalculateOptimalClusters' (nil, false)
    std::string why;     // of a refusal, without the caller's prefix
    int64_t N = 0, k = 0; // k: k_target when above 0, else CalculateOptimalClusters(N)
    // the max_size the kernels see, clamped to [1, N]: no size sum of unfrozen seeds is above N, so the clamp bans none of them, and a frozen
    // seed's effective size fits the packed column words
    int32_t kmax = 1;
};
// eff[m] (written for an accepted problem only): the sizes the kernels see -- a seed's items, or kmax for a frozen seed, the largest
// size the ban still refuses with every partner.
inline ward_admission ward_seed_admit(int64_t m, const int32_t *seed_size, int32_t min_size, int32_t max_size, int32_t k_target, int32_t *eff)
{
    ward_admission a;
    int64_t big = -1;
    for (int64_t i = 0; i < m; ++i) {
        a.N += std::llabs((long long)seed_size[i]);
        if (seed_size[i] > max_size && big < 0) big = i;
    }
    char b[200];
    b[0] = 0;
    if (a.N >= ((int64_t)1 << 30)) {
        a.status = ICL_ERR_UNSUPPORTED;
        snprintf(b, sizeof b, "%lld items in all", (long long)a.N);
    } else if (big >= 0) {
        a.status = ICL_ERR_UNSUPPORTED;
        snprintf(b, sizeof b, "seed %lld holds %d items, above maxSize (%d), and is not frozen", (long long)big, seed_size[big], max_size);
    } else if (k_target > 0) {
        a.k = k_target;
    } else if (ward_optimal_k(a.N, min_size, max_size, &a.k) != ICL_OK) {
        a.status = ICL_ERR_CONSTRAINT;
        snprintf(b, sizeof b, "cannot satisfy cluster size constraints with total items (%lld), minSize (%d), and maxSize (%d)", (long long)a.N,
                 min_size, max_size);
    }
    a.why = b;
    if (a.status != ICL_OK) return a;
    a.kmax = (int32_t)std::min<int64_t>(std::max<int64_t>(max_size, 1), std::max<int64_t>(a.N, 1));
    for (int64_t i = 0; i < m; ++i) eff[i] = seed_size[i] < 0 ? a.kmax : seed_size[i];
    return a;
}

// What ward_final_list found: a list, a row of size 0 (at: the row), or a log that names a cluster that does not exist, is dead, or
// twice in one pair (at: the step; a, b: its pair).  ward_list_text: the reason of the last two.
struct ward_list_result {
    enum { OK, ZERO_SIZE, CORRUPT } kind = OK;
    int64_t at = 0;
    int32_t a = 0, b = 0;
    int64_t largest = 0; // items of the largest final cluster, dropped ones included (0: no cluster)
};
inline std::string ward_list_text(const ward_list_result &r)
{
    char b[120];
    if (r.kind == ward_list_result::ZERO_SIZE) snprintf(b, sizeof b, "seed %lld has size 0", (long long)r.at);
    else snprintf(b, sizeof b, "corrupt merge log at step %lld (%d,%d)", (long long)r.at, r.a, r.b);
    return b;
}

// The reference's final cluster list (clustering.go:265-280 and SURVEY.md 8a C11) from m rows and a log of nmerge (a, b) pairs of
// creation ids (row i: i, the t-th merge: m + t): the surviving rows in index order, then the merged clusters in creation order; the
// members of Merge(a, b) are a's then b's (:31); a cluster whose ITEM count is below min_size is dropped and consumes no id.  A row
// counts |sizes[i]| items, or 1 where sizes is null: images are seeds of one item.  Out: cluster_id[m] and rank[m] (-1 for a dropped
// row), n_clusters and, where finals is not null, (creation id, rank-0 row) of every final cluster, dropped ones included.  Nothing
// is written unless the result is OK.
inline ward_list_result ward_final_list(int64_t m, const int32_t *sizes, int32_t min_size, const int32_t *pairs, int64_t nmerge, int32_t *cluster_id,
                                        int32_t *rank, int32_t *n_clusters, std::vector<int32_t> *finals)
{
    ward_list_result r;
    const int64_t M = m + nmerge;
    std::vector<int32_t> left((size_t)M, -1), right((size_t)M, -1);
    std::vector<int64_t> size((size_t)M, 1);
    std::vector<uint8_t> alive((size_t)M, 1);
    for (int64_t i = 0; sizes && i < m; ++i) {
        size[i] = std::llabs((long long)sizes[i]);
        if (!size[i]) {
            r.kind = ward_list_result::ZERO_SIZE, r.at = i;
            return r;
        }
    }
    for (int64_t t = 0; t < nmerge; ++t) {
        const int32_t a = pairs[2 * t], b = pairs[2 * t + 1];
        const int64_t c = m + t;
        if (a < 0 || b < 0 || a >= c || b >= c || a == b || !alive[a] || !alive[b]) {
            r.kind = ward_list_result::CORRUPT, r.at = t, r.a = a, r.b = b;
            return r;
        }
        left[c] = a;
        right[c] = b;
        size[c] = size[a] + size[b];
        alive[a] = alive[b] = 0;
    }
    for (int64_t i = 0; i < m; ++i) cluster_id[i] = rank[i] = -1;
    int32_t cid = 0;
    std::vector<int32_t> stack;
    if (finals) finals->clear();
    for (int64_t c = 0; c < M; ++c) {
        if (!alive[c]) continue;
        r.largest = std::max(r.largest, size[c]);
        if (finals) {
            int64_t f = c;
            while (f >= m) f = left[f];
            finals->push_back((int32_t)c);
            finals->push_back((int32_t)f);
        }
        if (size[c] < min_size) continue; // clustering.go:268-271
        int32_t next = 0;
        stack.assign(1, (int32_t)c);
        while (!stack.empty()) {
            const int32_t x = stack.back();
            stack.pop_back();
            if (x < m) {
                cluster_id[x] = cid;
                rank[x] = next++;
            } else {
                stack.push_back(right[x]); // visited after left: a's rows first
                stack.push_back(left[x]);
            }
        }
        ++cid;
    }
    *n_clusters = cid;
    return r;
}
