// pairs_plan_main.cpp -- the host side of icl_pairs_within and icl_pairs_between: imageclust_amd/csrc/pairs_plan.h (what ICL_ERR_ARG
// covers, the prefix over the count pass's figures, a hit's rank in its row mask, the body of both _from_matrix entry points) and the two
// rules of pairs_select.h in a stand-alone host program (no GPU, no HIP) that tests/test_pairs_between_cpu.py builds with the address and
// undefined-behaviour sanitizers and runs.  Every output lives in a heap block of exactly its size, so a write past an end is reported.
// The results are checked against the rules written out the slow way.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/band_plan.h"
#include "../imageclust_amd/csrc/pairs_plan.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#define CHECK(cond, ...)                                       \
    do {                                                       \
        if (!(cond)) {                                         \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);    \
            fprintf(stderr, __VA_ARGS__);                      \
            fprintf(stderr, " [%s]\n", #cond);                 \
            exit(1);                                           \
        }                                                      \
    } while (0)

static uint64_t rng_state = 0;
static uint64_t rnd() // splitmix64
{
    uint64_t x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

static bool same_bits(float a, float b)
{
    uint32_t x, y;
    __builtin_memcpy(&x, &a, 4);
    __builtin_memcpy(&y, &b, 4);
    return x == y;
}

static const float INF = std::numeric_limits<float>::infinity();

static float some_value()
{
    const float set[] = {0.0f, -0.0f, 1.0f, 2.0f, 2.0f, 3.5f, -1.0f, INF, -INF, std::nanf(""), 3.4028234663852886e38f, 7.0f};
    return set[rnd() % (sizeof set / sizeof set[0])];
}

// the rule, written out: not the excluded column, a number, and not above the threshold
static bool listed_slowly(int64_t j, int64_t ex, float v, float thr)
{
    if (ex >= 0 && j == ex) return false;
    if (std::isnan(v)) return false;
    return !(v > thr);
}

static void rule()
{
    const float nan = std::nanf("");
    CHECK(ps_listed_between(3, -1, 0.0f, -0.0f) && ps_listed_between(3, -1, -0.0f, 0.0f), "a threshold of -0 admits zero values");
    CHECK(!ps_listed_between(3, 3, 0.0f, 1.0f) && ps_listed_between(2, 3, 0.0f, 1.0f), "the excluded column");
    CHECK(!ps_listed_between(0, -1, nan, INF) && ps_listed_between(0, -1, INF, INF) && ps_listed_between(0, -1, -INF, -INF), "NaN and Inf");
    CHECK(!ps_listed_between(0, -1, 1.0f, 0.5f) && !ps_listed_between(0, -1, 0.0f, -1.0f), "above the threshold");
    for (int q = 0; q < 20000; ++q) {
        const int64_t j = (int64_t)(rnd() % 5), ex = (int64_t)(rnd() % 6) - 1;
        const float v = some_value(), t = some_value();
        if (std::isnan(t)) continue;
        CHECK(ps_listed_between(j, ex, v, t) == listed_slowly(j, ex, v, t), "j=%lld ex=%lld v=%g t=%g", (long long)j, (long long)ex, v, t);
    }
    CHECK(ps_listed(3, 2, 1.0f, 1.0f) && !ps_listed(2, 3, 1.0f, 1.0f), "the self-join's rule is as it was");
    printf("rule: ok\n");
}

static void from_matrix_sweep()
{
    for (int round = 0; round < 400; ++round) {
        const int64_t nq = (int64_t)(rnd() % 9), n = (int64_t)(rnd() % 11), ld = n + (int64_t)(rnd() % 3);
        std::vector<float> D((size_t)(nq * ld));
        for (float &v : D) v = some_value();
        std::vector<int64_t> ex((size_t)nq);
        for (int64_t &e : ex) e = n ? (int64_t)(rnd() % (uint64_t)(n + 1)) - 1 : -1;
        const bool with_ex = rnd() % 2;
        float thr = some_value();
        if (std::isnan(thr)) thr = INF;
        // the slow statement
        std::vector<int64_t> want_ptr((size_t)nq + 1, 0);
        std::vector<int32_t> want_col;
        std::vector<float> want_val;
        for (int64_t i = 0; i < nq; ++i) {
            for (int64_t j = 0; j < n; ++j)
                if (listed_slowly(j, with_ex ? ex[(size_t)i] : -1, D[(size_t)(i * ld + j)], thr)) {
                    want_col.push_back((int32_t)j);
                    want_val.push_back(D[(size_t)(i * ld + j)]);
                }
            want_ptr[(size_t)i + 1] = (int64_t)want_col.size();
        }
        const int64_t total = (int64_t)want_col.size();
        // the size query, a buffer one short, a buffer of exactly total: each output in a block of exactly its size
        for (int mode = 0; mode < 3; ++mode) {
            const int64_t cap = mode == 0 ? 0 : mode == 1 ? total - 1 : total;
            if (cap < 0) continue;
            int64_t *rp = (int64_t *)malloc((size_t)(nq + 1) * 8);
            int32_t *col = mode ? (int32_t *)malloc((size_t)(cap ? cap : 1) * 4) : nullptr; // (a block of no bytes may be no block at all)
            float *val = mode ? (float *)malloc((size_t)(cap ? cap : 1) * 4) : nullptr;
            int64_t tot = -5;
            const int rc = pairs_between_from_matrix(nq && n ? D.data() : nullptr, nq, n, ld, thr, with_ex ? ex.data() : nullptr, rp, col, val, cap, &tot);
            CHECK(tot == total, "round %d mode %d: total %lld, want %lld", round, mode, (long long)tot, (long long)total);
            for (int64_t i = 0; i <= nq; ++i) CHECK(rp[i] == want_ptr[(size_t)i], "round %d: row_ptr[%lld]", round, (long long)i);
            CHECK(rc == (mode == 1 ? -1 : 0), "round %d mode %d: code %d", round, mode, rc);
            if (mode == 2)
                for (int64_t p = 0; p < total; ++p)
                    CHECK(col[p] == want_col[(size_t)p] && same_bits(val[p], want_val[(size_t)p]), "round %d: place %lld", round, (long long)p);
            free(rp);
            free(col);
            free(val);
        }
    }
    printf("from_matrix sweep: ok\n");
}

static void prefix_and_placement()
{
    for (int round = 0; round < 300; ++round) {
        const int64_t nq = 1 + (int64_t)(rnd() % 300), n = 1 + (int64_t)(rnd() % 900);
        const int64_t nbands = (nq + PAIRS_ROWS - 1) / PAIRS_ROWS, ntiles = (n + PAIRS_ROWS - 1) / PAIRS_ROWS;
        const int forced = (int)(rnd() % 9), cus = 1 + (int)(rnd() % 256);
        const int splits = band_splits(forced, cus, nbands, ntiles);
        CHECK(splits >= 1 && splits <= ntiles, "splits %d of %lld tiles", splits, (long long)ntiles);
        // hits: a sparse, a dense or a full rectangle
        const int density = (int)(rnd() % 3);
        std::vector<uint8_t> H((size_t)(nq * n));
        for (uint8_t &h : H) h = density == 2 ? 1 : density == 1 ? rnd() % 2 : rnd() % 40 == 0;
        // the segments are column ranges in ascending order that cover every tile once
        int64_t covered = 0;
        for (int s = 0; s < splits; ++s) {
            CHECK(s * ntiles / splits == covered && (s + 1) * ntiles / splits > covered, "split %d starts where the last one ended and is not empty", s);
            covered = (s + 1) * ntiles / splits;
        }
        CHECK(covered == ntiles, "the splits cover the tiles");
        // the count pass's figures, as its workgroups leave them
        int32_t *seg_count = (int32_t *)malloc((size_t)(nq * splits) * 4);
        for (int64_t i = 0; i < nq; ++i)
            for (int s = 0; s < splits; ++s) {
                int32_t c = 0;
                for (int64_t j = s * ntiles / splits * PAIRS_ROWS; j < (s + 1) * ntiles / splits * PAIRS_ROWS && j < n; ++j) c += H[(size_t)(i * n + j)];
                seg_count[i * splits + s] = c;
            }
        int64_t *seg_ptr = (int64_t *)malloc((size_t)(nq * splits + 1) * 8), *row_ptr = (int64_t *)malloc((size_t)(nq + 1) * 8), total = -1;
        pairs_prefix(nq, splits, seg_count, seg_ptr, row_ptr, &total);
        CHECK(row_ptr[0] == 0 && row_ptr[nq] == total && seg_ptr[nq * splits] == total, "the ends of the prefix");
        // the fill pass's placement, workgroup by workgroup in a scrambled order: every place written exactly once, rows ascending
        int32_t *col = (int32_t *)malloc((size_t)(total ? total : 1) * 4);
        uint8_t *seen = (uint8_t *)calloc((size_t)(total ? total : 1), 1);
        std::vector<int64_t> order((size_t)(nbands * splits));
        for (size_t q = 0; q < order.size(); ++q) order[q] = (int64_t)q;
        for (size_t q = order.size(); q > 1; --q) std::swap(order[q - 1], order[rnd() % q]);
        for (int64_t block : order) {
            const int64_t band = block % nbands, split = block / nbands;
            std::vector<int32_t> cur(PAIRS_ROWS, 0);
            for (int64_t t = split * ntiles / splits; t < (split + 1) * ntiles / splits; ++t)
                for (int r = 0; r < PAIRS_ROWS; ++r) {
                    const int64_t i = band * PAIRS_ROWS + r;
                    if (i >= nq) continue;
                    uint32_t m[4] = {0, 0, 0, 0};
                    for (int c = 0; c < PAIRS_ROWS; ++c)
                        if (t * PAIRS_ROWS + c < n && H[(size_t)(i * n + t * PAIRS_ROWS + c)]) m[c >> 5] |= 1u << (c & 31);
                    const int64_t sg = i * splits + split, len = seg_ptr[sg + 1] - seg_ptr[sg];
                    int in_tile = 0;
                    for (int c = 0; c < PAIRS_ROWS; ++c) {
                        if (!((m[c >> 5] >> (c & 31)) & 1u)) continue;
                        CHECK(pairs_mask_rank(m, c) == in_tile, "rank of column %d", c);
                        const int64_t p = cur[(size_t)r] + in_tile++;
                        CHECK(p < len, "a place beyond the segment");
                        CHECK(!seen[seg_ptr[sg] + p], "a place written twice");
                        seen[seg_ptr[sg] + p] = 1;
                        col[seg_ptr[sg] + p] = (int32_t)(t * PAIRS_ROWS + c);
                    }
                    cur[(size_t)r] += in_tile;
                }
        }
        for (int64_t i = 0; i < nq; ++i) {
            int64_t p = row_ptr[i];
            for (int64_t j = 0; j < n; ++j)
                if (H[(size_t)(i * n + j)]) {
                    CHECK(p < row_ptr[i + 1] && seen[p] && col[p] == j, "round %d: row %lld place %lld", round, (long long)i, (long long)p);
                    ++p;
                }
            CHECK(p == row_ptr[i + 1], "round %d: row %lld's length", round, (long long)i);
        }
        free(seg_count);
        free(seg_ptr);
        free(row_ptr);
        free(col);
        free(seen);
    }
    printf("prefix and placement: ok\n");
}

static void bad_arguments()
{
    const int64_t nq = 3, n = 4;
    std::vector<float> D((size_t)(nq * n), 0.0f);
    int64_t *rp = (int64_t *)malloc((size_t)(nq + 1) * 8), tot = -5;
    int32_t *col = (int32_t *)malloc(12 * 4);
    float *val = (float *)malloc(12 * 4);
    for (int64_t i = 0; i <= nq; ++i) rp[i] = 77;
    for (int q = 0; q < 12; ++q) {
        col[q] = 77;
        val[q] = 77.0f;
    }
    const int64_t ex_ok[3] = {-1, 0, 3}, ex_hi[3] = {-1, 4, 0}, ex_lo[3] = {-2, 0, 0};
    const float nan = std::nanf("");
    struct bad {
        const char *name;
        int rc;
    } cases[] = {
        {"null D", pairs_between_from_matrix(nullptr, nq, n, n, 1.0f, ex_ok, rp, col, val, 12, &tot)},
        {"null row_ptr", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, nullptr, col, val, 12, &tot)},
        {"null total", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, col, val, 12, nullptr)},
        {"null col", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, nullptr, val, 12, &tot)},
        {"null val", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, col, nullptr, 12, &tot)},
        {"null both with a cap", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, nullptr, nullptr, 1, &tot)},
        {"negative nq", pairs_between_from_matrix(D.data(), -1, n, n, 1.0f, nullptr, rp, col, val, 12, &tot)},
        {"negative n", pairs_between_from_matrix(D.data(), nq, -1, n, 1.0f, nullptr, rp, col, val, 12, &tot)},
        {"n of 2^31", pairs_between_from_matrix(D.data(), nq, 1LL << 31, 1LL << 31, 1.0f, nullptr, rp, col, val, 12, &tot)},
        {"short ld", pairs_between_from_matrix(D.data(), nq, n, n - 1, 1.0f, ex_ok, rp, col, val, 12, &tot)},
        {"exclude of n", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_hi, rp, col, val, 12, &tot)},
        {"exclude below -1", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_lo, rp, col, val, 12, &tot)},
        {"NaN threshold", pairs_between_from_matrix(D.data(), nq, n, n, nan, ex_ok, rp, col, val, 12, &tot)},
        {"negative cap", pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, col, val, -1, &tot)},
    };
    for (const bad &b : cases) CHECK(b.rc == -1, "%s", b.name);
    for (int64_t i = 0; i <= nq; ++i) CHECK(rp[i] == 77, "row_ptr untouched");
    for (int q = 0; q < 12; ++q) CHECK(col[q] == 77 && val[q] == 77.0f, "col and val untouched");
    CHECK(tot == -5, "total untouched");
    const int32_t qs_bad[3] = {1, 0, 1}, ls_bad[4] = {1, 1, 1, -2};
    CHECK(pairs_between_bad_arg(nq, n, 1.0f, qs_bad, nullptr, nullptr, rp, col, val, 12, &tot) && pairs_between_bad_arg(nq, n, 1.0f, nullptr, ls_bad, nullptr, rp, col, val, 12, &tot),
          "a size that is not above 0");
    CHECK(pairs_between_from_matrix(D.data(), nq, n, n, 1.0f, ex_ok, rp, col, val, 12, &tot) == 0 && tot == 10 && rp[1] == 4 && rp[2] == 7 && rp[3] == 10, "the good call");
    CHECK(col[4] == 1 && col[9] == 2 && col[10] == 77, "the excluded columns are missing and nothing lies beyond total");
    CHECK(pairs_between_from_matrix(nullptr, 0, n, n, 1.0f, nullptr, rp, nullptr, nullptr, 0, &tot) == 0 && tot == 0 && rp[0] == 0 && rp[1] == 4, "no queries");
    CHECK(pairs_between_from_matrix(nullptr, nq, 0, 0, 1.0f, nullptr, rp, nullptr, nullptr, 0, &tot) == 0 && tot == 0 && rp[3] == 0, "no library");
    free(rp);
    free(col);
    free(val);
    printf("bad arguments: ok\n");
}

// ---- icl_pairs_within's half ----------------------------------------------------------------------------------------------------
// its rule, written out: strictly below the diagonal, a number, and not above the threshold
static bool within_listed_slowly(int64_t i, int64_t j, float v, float thr)
{
    if (j >= i) return false;
    if (std::isnan(v)) return false;
    return !(v > thr);
}

static void within_rule()
{
    const float nan = std::nanf("");
    CHECK(ps_listed(3, 2, 0.0f, -0.0f) && ps_listed(3, 2, -0.0f, 0.0f), "a threshold of -0 admits zero values");
    CHECK(!ps_listed(3, 3, 0.0f, 1.0f) && !ps_listed(2, 3, 0.0f, 1.0f) && ps_listed(3, 0, 0.0f, 1.0f), "the strict lower triangle");
    CHECK(!ps_listed(1, 0, nan, INF) && ps_listed(1, 0, INF, INF) && ps_listed(1, 0, -INF, -INF), "NaN and Inf");
    CHECK(!ps_listed(1, 0, 1.0f, 0.5f) && !ps_listed(1, 0, 0.0f, -1.0f), "above the threshold");
    for (int q = 0; q < 20000; ++q) {
        const int64_t i = (int64_t)(rnd() % 5), j = (int64_t)(rnd() % 5);
        const float v = some_value(), t = some_value();
        if (std::isnan(t)) continue;
        CHECK(ps_listed(i, j, v, t) == within_listed_slowly(i, j, v, t), "i=%lld j=%lld v=%g t=%g", (long long)i, (long long)j, v, t);
    }
    printf("within rule: ok\n");
}

static void within_from_matrix_sweep()
{
    for (int round = 0; round < 400; ++round) {
        const int64_t n = round < 3 ? round : (int64_t)(rnd() % 11), ld = n + (int64_t)(rnd() % 3); // n of 0, 1 and 2 first
        std::vector<float> D((size_t)(n * ld));
        for (float &v : D) v = some_value();
        float thr = round < 3 ? INF : some_value();
        if (std::isnan(thr)) thr = INF;
        // the slow statement
        std::vector<int64_t> want_ptr((size_t)n + 1, 0);
        std::vector<int32_t> want_col;
        std::vector<float> want_val;
        for (int64_t i = 0; i < n; ++i) {
            for (int64_t j = 0; j < n; ++j)
                if (within_listed_slowly(i, j, D[(size_t)(i * ld + j)], thr)) {
                    want_col.push_back((int32_t)j);
                    want_val.push_back(D[(size_t)(i * ld + j)]);
                }
            want_ptr[(size_t)i + 1] = (int64_t)want_col.size();
        }
        const int64_t total = (int64_t)want_col.size();
        // the size query, a buffer one short, a buffer of exactly total: each output in a block of exactly its size
        for (int mode = 0; mode < 3; ++mode) {
            const int64_t cap = mode == 0 ? 0 : mode == 1 ? total - 1 : total;
            if (cap < 0) continue;
            int64_t *rp = (int64_t *)malloc((size_t)(n + 1) * 8);
            int32_t *col = mode ? (int32_t *)malloc((size_t)(cap ? cap : 1) * 4) : nullptr; // (a block of no bytes may be no block at all)
            float *val = mode ? (float *)malloc((size_t)(cap ? cap : 1) * 4) : nullptr;
            for (int64_t p = 0; mode && p < cap; ++p) {
                col[p] = 77;
                val[p] = 77.0f;
            }
            int64_t tot = -5;
            const int rc = pairs_within_from_matrix(n > 1 ? D.data() : nullptr, n, ld, thr, rp, col, val, cap, &tot);
            CHECK(tot == total, "round %d mode %d: total %lld, want %lld", round, mode, (long long)tot, (long long)total);
            for (int64_t i = 0; i <= n; ++i) CHECK(rp[i] == want_ptr[(size_t)i], "round %d: row_ptr[%lld]", round, (long long)i);
            CHECK(rc == (mode == 1 ? -1 : 0), "round %d mode %d: code %d", round, mode, rc);
            if (mode == 1) // too small a cap: row_ptr and *total complete (above), col and val untouched
                for (int64_t p = 0; p < cap; ++p) CHECK(col[p] == 77 && val[p] == 77.0f, "round %d: place %lld written though nothing fits", round, (long long)p);
            if (mode == 2)
                for (int64_t p = 0; p < total; ++p)
                    CHECK(col[p] == want_col[(size_t)p] && same_bits(val[p], want_val[(size_t)p]), "round %d: place %lld", round, (long long)p);
            free(rp);
            free(col);
            free(val);
        }
    }
    // what ICL_ERR_ARG covers: nothing is written
    std::vector<float> D(9, 0.0f);
    int64_t rp[4] = {77, 77, 77, 77}, tot = -5;
    int32_t col[3] = {77, 77, 77};
    float val[3] = {77.0f, 77.0f, 77.0f};
    struct bad {
        const char *name;
        int rc;
    } cases[] = {
        {"null D", pairs_within_from_matrix(nullptr, 3, 3, 1.0f, rp, col, val, 3, &tot)},
        {"null row_ptr", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, nullptr, col, val, 3, &tot)},
        {"null total", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, col, val, 3, nullptr)},
        {"null col", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, nullptr, val, 3, &tot)},
        {"null val", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, col, nullptr, 3, &tot)},
        {"null both with a cap", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, nullptr, nullptr, 1, &tot)},
        {"negative n", pairs_within_from_matrix(D.data(), -1, 3, 1.0f, rp, col, val, 3, &tot)},
        {"n of 2^31", pairs_within_from_matrix(D.data(), 1LL << 31, 1LL << 31, 1.0f, rp, col, val, 3, &tot)},
        {"short ld", pairs_within_from_matrix(D.data(), 3, 2, 1.0f, rp, col, val, 3, &tot)},
        {"NaN threshold", pairs_within_from_matrix(D.data(), 3, 3, std::nanf(""), rp, col, val, 3, &tot)},
        {"negative cap", pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, col, val, -1, &tot)},
    };
    for (const bad &b : cases) CHECK(b.rc == -1, "%s", b.name);
    for (int q = 0; q < 3; ++q) CHECK(rp[q] == 77 && rp[3] == 77 && col[q] == 77 && val[q] == 77.0f, "outputs untouched");
    CHECK(tot == -5, "total untouched");
    CHECK(pairs_within_from_matrix(D.data(), 3, 3, 1.0f, rp, col, val, 3, &tot) == 0 && tot == 3 && rp[0] == 0 && rp[1] == 0 && rp[2] == 1 && rp[3] == 3,
          "the good call");
    CHECK(col[0] == 0 && col[1] == 0 && col[2] == 1, "the good call's columns");
    printf("within from_matrix sweep: ok\n");
}

static void within_prefix()
{
    for (int round = 0; round < 300; ++round) {
        const int64_t n = (int64_t)(rnd() % 700);
        int32_t *count = (int32_t *)malloc((size_t)(n ? n : 1) * 4);
        for (int64_t i = 0; i < n; ++i) count[i] = (int32_t)(rnd() % 4 == 0 ? rnd() % (uint64_t)(i + 1) : 0); // (row i has at most i partners)
        int64_t *seg_ptr = (int64_t *)malloc((size_t)(n + 1) * 8), *row_ptr = (int64_t *)malloc((size_t)(n + 1) * 8), total = -1;
        pairs_prefix(n, 1, count, seg_ptr, row_ptr, &total);
        int64_t sum = 0;
        for (int64_t i = 0; i < n; ++i) {
            CHECK(row_ptr[i] == sum && seg_ptr[i] == sum, "round %d: row %lld starts at %lld, not %lld", round, (long long)i, (long long)row_ptr[i], (long long)sum);
            sum += count[i];
        }
        CHECK(row_ptr[n] == sum && seg_ptr[n] == sum && total == sum, "round %d: the ends of the prefix", round);
        free(count);
        free(seg_ptr);
        free(row_ptr);
    }
    int64_t rp[4] = {77, 77, 77, 77}, tot = -5;
    pairs_empty(2, rp, &tot);
    CHECK(rp[0] == 0 && rp[1] == 0 && rp[2] == 0 && rp[3] == 77 && tot == 0, "the empty result is nrows + 1 zeros");
    printf("within prefix: ok\n");
}

int main()
{
    rule();
    from_matrix_sweep();
    prefix_and_placement();
    bad_arguments();
    within_rule();
    within_from_matrix_sweep();
    within_prefix();
    printf("ok\n");
    return 0;
}
