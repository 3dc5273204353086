// apart_bits_main.cpp -- the host rules of imageclust_amd/csrc/apart_bits.h (which keep-apart constraints icl_cluster_many_apart accepts,
// and the bit rows its kernels see): a stand-alone host program (no GPU, no HIP) that tests/test_cluster_apart_cpu.py builds with the
// address and undefined-behaviour sanitizers and runs.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/apart_bits.h"

#include <cstdio>
#include <cstdlib>
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

// the table of (m, cls, pairs) against a naive m x m bool array, bit by bit, the padding of every row's last word included
static int64_t check_table(int64_t m, const std::vector<int32_t> &cls, const std::vector<int32_t> &pairs, bool with_cls)
{
    const int64_t np = (int64_t)pairs.size() / 2, W = ab_words(m);
    CHECK(ab_bad_arg(m, with_cls ? cls.data() : nullptr, np ? pairs.data() : nullptr, np).empty(), "m %lld: refused", (long long)m);
    std::vector<char> naive((size_t)(m * m), 0);
    for (int64_t q = 0; q < np; ++q) naive[(size_t)(pairs[2 * q] * m + pairs[2 * q + 1])] = naive[(size_t)(pairs[2 * q + 1] * m + pairs[2 * q])] = 1;
    for (int64_t i = 0; with_cls && i < m; ++i)
        for (int64_t j = 0; j < m; ++j)
            if (i != j && cls[(size_t)i] != 0 && cls[(size_t)i] == cls[(size_t)j]) naive[(size_t)(i * m + j)] = 1;
    std::vector<uint32_t> rows((size_t)(m * W) + 1, 0xdeadbeefu); // (one word behind the table: it must stay as it is)
    const bool any = ab_expand(m, with_cls ? cls.data() : nullptr, np ? pairs.data() : nullptr, np, rows.data());
    CHECK(ab_table_bytes(m) == (size_t)(m * W) * 4 && rows.back() == 0xdeadbeefu, "m %lld: table size", (long long)m);
    int64_t set = 0;
    for (int64_t i = 0; i < m; ++i)
        for (int64_t j = 0; j < 32 * W; ++j) {
            const bool bit = rows[(size_t)(i * W + (j >> 5))] >> (j & 31) & 1u;
            const bool want = j < m && naive[(size_t)(i * m + j)];
            CHECK(bit == want, "m %lld: bit (%lld, %lld) is %d", (long long)m, (long long)i, (long long)j, (int)bit);
            if (j < m) CHECK(bit == ab_bit(rows.data(), m, i, j) && bit == ab_bit(rows.data(), m, j, i), "m %lld: ab_bit / symmetry at (%lld, %lld)", (long long)m, (long long)i, (long long)j);
            set += bit;
        }
    for (int64_t i = 0; i < m; ++i) CHECK(!ab_bit(rows.data(), m, i, i), "m %lld: diagonal %lld", (long long)m, (long long)i);
    CHECK(any == (set > 0), "m %lld: any", (long long)m);
    return set;
}

int main()
{
    const int64_t sizes[] = {1, 2, 31, 32, 33, 64, 65, 300};
    // 1. random pairs (both orders, duplicates) and classes against the naive array
    int64_t bits = 0;
    for (int64_t m : sizes)
        for (int round = 0; round < 6; ++round) {
            std::vector<int32_t> cls((size_t)m, 0), pairs;
            if (m >= 2) {
                const int64_t np = round == 0 ? 0 : (int64_t)(rnd() % (uint64_t)(3 * m)) + 1;
                for (int64_t q = 0; q < np; ++q) {
                    const int32_t i = (int32_t)(rnd() % (uint64_t)m);
                    int32_t j = (int32_t)(rnd() % (uint64_t)(m - 1));
                    j += j >= i;
                    pairs.push_back(i), pairs.push_back(j);
                    if (q % 5 == 0) pairs.push_back(j), pairs.push_back(i); // the other order: a duplicate
                }
            }
            for (int64_t i = 0; i < m; ++i) cls[(size_t)i] = round % 2 ? (int32_t)(rnd() % 4) * (int32_t)(rnd() % 2) : 0;
            bits += check_table(m, cls, pairs, round != 1);
            if (round == 1) CHECK(check_table(m, cls, pairs, true) >= 0, "classes");
        }
    CHECK(bits > 1000, "only %lld bits set", (long long)bits);
    printf("random tables: %lld bits\n", (long long)bits);
    // 2. the word edges: pairs on seeds 0, 31, 32, 63, 64, m - 1 and one class across every word boundary
    for (int64_t m : sizes) {
        std::vector<int32_t> cls((size_t)m, 0), pairs;
        const int64_t edge[] = {0, 31, 32, 63, 64, m - 1};
        for (int64_t a : edge)
            for (int64_t b : edge)
                if (a < m && b < m && a < b) pairs.push_back((int32_t)b), pairs.push_back((int32_t)a);
        for (int64_t i = 0; i < m; ++i)
            if (i % 32 == 31 || i % 32 == 0) cls[(size_t)i] = 7;
        const int64_t set = check_table(m, cls, pairs, true);
        CHECK(m < 2 || set > 0, "m %lld: nothing set", (long long)m);
    }
    check_table(0, {}, {}, true);
    printf("word edges\n");
    // 3. every refusal
    {
        const int32_t ok_cls[3] = {0, 5, 5}, neg_cls[3] = {0, -1, 0};
        const int32_t ok[4] = {0, 2, 2, 1}, self[2] = {1, 1}, high[2] = {0, 3}, low[2] = {-1, 0}, high_first[2] = {3, 0};
        CHECK(ab_bad_arg(3, ok_cls, ok, 2).empty() && ab_bad_arg(3, nullptr, nullptr, 0).empty() && ab_bad_arg(0, nullptr, nullptr, 0).empty(), "accepted");
        CHECK(!ab_bad_arg(3, neg_cls, ok, 2).empty(), "a negative class");
        CHECK(!ab_bad_arg(3, ok_cls, self, 1).empty(), "i == j");
        CHECK(!ab_bad_arg(3, ok_cls, high, 1).empty() && !ab_bad_arg(3, ok_cls, high_first, 1).empty(), "an index of m");
        CHECK(!ab_bad_arg(3, ok_cls, low, 1).empty(), "a negative index");
        CHECK(!ab_bad_arg(3, ok_cls, nullptr, 1).empty(), "pairs without an array");
        CHECK(!ab_bad_arg(3, ok_cls, ok, -1).empty(), "a negative count");
        CHECK(!ab_bad_arg(1, nullptr, ok, 1).empty() && !ab_bad_arg(0, nullptr, ok, 1).empty(), "a pair in a problem of one seed or none");
    }
    printf("refusals\n");
    printf("ok\n");
    return 0;
}
