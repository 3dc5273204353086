// fit_select_main.cpp -- the host side of icl_cluster_fit: imageclust_amd/csrc/fit_select.h (the leave-out rule, the packed keys, the
// body of icl_cluster_fit_from_matrix) in a stand-alone host program (no GPU, no HIP) that tests/test_cluster_fit_cpu.py builds with the
// address and undefined-behaviour sanitizers and runs.  Every output lives in a heap block of exactly its size, so a write past an
// end is reported.  The results are checked against the rules written out the slow way.  Prints one line per rule and a final "ok".
#include "../imageclust_amd/csrc/fit_select.h"

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
    return x == y || (std::isnan(a) && std::isnan(b));
}

// a value from a small set: ties, both zeros, NaN and the infinities wherever they fall
static float some_value()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float set[] = {0.0f, -0.0f, 1.0f, 2.0f, 2.0f, 3.5f, -1.0f, inf, -inf, std::nanf(""), NS_MAXF, 7.0f};
    return set[rnd() % (sizeof set / sizeof set[0])];
}

// (a, ia) in front of (b, ib), written out: numbers before NaN, smaller first, then the lower index
static bool in_front(float a, int64_t ia, float b, int64_t ib)
{
    if (std::isnan(a) != std::isnan(b)) return std::isnan(b);
    if (!std::isnan(a) && a != b) return a < b;
    return ia < ib;
}

struct problem {
    int64_t nq, K, ld;
    int32_t k_alt, max_size;
    std::vector<float> D;
    std::vector<int32_t> qs, cof, cs;
};

static problem make(int64_t nq, int64_t K, int32_t k_alt, int32_t max_size)
{
    problem p;
    p.nq = nq, p.K = K, p.ld = K + (int64_t)(rnd() % 3), p.k_alt = k_alt, p.max_size = max_size;
    p.D.resize((size_t)(nq * p.ld));
    for (float &v : p.D) v = some_value();
    for (int64_t i = 0; i < nq; ++i) {
        p.qs.push_back(1 + (int32_t)(rnd() % 6));
        p.cof.push_back(K && rnd() % 5 ? (int32_t)(rnd() % (uint64_t)K) : -1);
    }
    for (int64_t j = 0; j < K; ++j) p.cs.push_back((1 + (int32_t)(rnd() % 9)) * (rnd() % 4 ? 1 : -1));
    return p;
}

static void run_and_check(const problem &p, bool with_sizes)
{
    const int64_t nq = p.nq, K = p.K;
    const int k = p.k_alt;
    // exact-size heap blocks (a vector of 0 entries gives a null pointer: legal where nothing is to be written)
    std::vector<float> own((size_t)nq, -5.0f), av((size_t)(nq * k), -5.0f);
    std::vector<int32_t> aj((size_t)(nq * k), -5), listed((size_t)K, -5), rep((size_t)K, -5), worst((size_t)K, -5);
    const int32_t *qs = with_sizes ? p.qs.data() : nullptr, *cs = with_sizes ? p.cs.data() : nullptr;
    const bool ok = fs_fit_from_matrix(p.D.data(), nq, K, p.ld, qs, p.cof.data(), cs, k, p.max_size, own.data(), k ? aj.data() : nullptr,
                                       k ? av.data() : nullptr, listed.data(), rep.data(), worst.data());
    CHECK(ok, "nq=%lld K=%lld k=%d refused", (long long)nq, (long long)K, k);
    for (int64_t i = 0; i < nq; ++i) {
        const int64_t c = p.cof[(size_t)i];
        CHECK(same_bits(own[(size_t)i], c < 0 ? NS_MAXF : p.D[(size_t)(i * p.ld + c)]), "own of row %lld", (long long)i);
        std::vector<int64_t> left; // the columns the row may list, then a selection sort by the order written out
        for (int64_t j = 0; j < K; ++j) {
            const int64_t s = cs ? cs[j] : 1, q = qs ? qs[i] : 1;
            if (j != c && s > 0 && !(p.max_size > 0 && q + s > p.max_size)) left.push_back(j);
        }
        for (int place = 0; place < k; ++place) {
            int64_t best = -1;
            size_t at = 0;
            for (size_t x = 0; x < left.size(); ++x)
                if (best < 0 || in_front(p.D[(size_t)(i * p.ld + left[x])], left[x], p.D[(size_t)(i * p.ld + best)], best)) best = left[x], at = x;
            if (best >= 0) left.erase(left.begin() + (long)at);
            CHECK(aj[(size_t)(i * k + place)] == (int32_t)best, "row %lld place %d: column %d, want %lld", (long long)i, place,
                  aj[(size_t)(i * k + place)], (long long)best);
            CHECK(same_bits(av[(size_t)(i * k + place)], best < 0 ? NS_MAXF : p.D[(size_t)(i * p.ld + best)]), "row %lld place %d: value", (long long)i,
                  place);
        }
    }
    for (int64_t c = 0; c < K; ++c) {
        int64_t n = 0, r = -1, w = -1;
        for (int64_t i = 0; i < nq; ++i) {
            if (p.cof[(size_t)i] != c) continue;
            ++n;
            if (r < 0 || in_front(own[(size_t)i], i, own[(size_t)r], r)) r = i;
            // worst: NaN above every number, larger first, then the lower index
            const float v = own[(size_t)i], u = w < 0 ? 0.0f : own[(size_t)w];
            if (w < 0 || (std::isnan(v) && !std::isnan(u)) || (!std::isnan(v) && !std::isnan(u) && v > u)) w = i;
        }
        CHECK(listed[(size_t)c] == n && rep[(size_t)c] == r && worst[(size_t)c] == w, "cluster %lld: listed %d rep %d worst %d, want %lld %lld %lld",
              (long long)c, listed[(size_t)c], rep[(size_t)c], worst[(size_t)c], (long long)n, (long long)r, (long long)w);
    }
    // the per-cluster outputs are optional
    CHECK(fs_fit_from_matrix(p.D.data(), nq, K, p.ld, qs, p.cof.data(), cs, k, p.max_size, own.data(), k ? aj.data() : nullptr, k ? av.data() : nullptr,
                             nullptr, nullptr, nullptr),
          "null per-cluster outputs refused");
}

static void keys()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float up[] = {-inf, -NS_MAXF, -1.0f, -1e-45f, 0.0f, 1e-45f, 1.0f, NS_MAXF, inf, std::nanf("")};
    const int n = (int)(sizeof up / sizeof up[0]);
    for (int a = 0; a + 1 < n; ++a) CHECK(fs_ordered_bits(up[a]) < fs_ordered_bits(up[a + 1]), "order of %g and %g", up[a], up[a + 1]);
    CHECK(fs_ordered_bits(-0.0f) == fs_ordered_bits(0.0f), "the zeros are one value");
    CHECK(fs_ordered_bits(-std::nanf("")) == fs_ordered_bits(std::nanf("")), "every NaN is one value");
    const int64_t rows[] = {0, 1, 77, 0x7ffffffe, 0x7fffffff};
    for (float v : up)
        for (int64_t r : rows) {
            CHECK(fs_rep_row(fs_key_rep(v, r)) == (int32_t)r && fs_worst_row(fs_key_worst(v, r)) == (int32_t)r, "row %lld round trip", (long long)r);
            CHECK(fs_key_rep(v, r) != FS_REP_EMPTY && fs_key_worst(v, r) != FS_WORST_EMPTY, "a real key equals an empty one");
        }
    CHECK(fs_key_rep(1.0f, 3) < fs_key_rep(1.0f, 9) && fs_key_worst(1.0f, 3) > fs_key_worst(1.0f, 9), "ties go to the lower row");
    CHECK(fs_rep_row(FS_REP_EMPTY) == -1 && fs_worst_row(FS_WORST_EMPTY) == -1, "empty keys");
    CHECK(fs_left_out(3, 3, 1, 1, 0) && fs_left_out(2, 3, 1, -1, 0) && fs_left_out(2, 3, 5, 6, 10) && !fs_left_out(2, 3, 5, 5, 10) &&
              !fs_left_out(2, -1, 5, 6, 0),
          "leave-out rule");
    CHECK(fs_items(-2147483647 - 1) == 2147483648LL && fs_items(7) == 7, "item counts");
}

static void bad_arguments()
{
    problem p = make(4, 5, 3, 0);
    std::vector<float> own(4, -5.0f), av(12, -5.0f);
    std::vector<int32_t> aj(12, -5), listed(5, -5), rep(5, -5), worst(5, -5);
    auto call = [&](const problem &q, const float *D, const int32_t *cof, float *o, int32_t *j, float *v) {
        return fs_fit_from_matrix(D, q.nq, q.K, q.ld, q.qs.data(), cof, q.cs.data(), q.k_alt, q.max_size, o, j, v, listed.data(), rep.data(), worst.data());
    };
    auto untouched = [&]() {
        for (float x : own) CHECK(x == -5.0f, "own written");
        for (float x : av) CHECK(x == -5.0f, "alt_val written");
        for (int32_t x : aj) CHECK(x == -5, "alt_idx written");
        for (size_t c = 0; c < 5; ++c) CHECK(listed[c] == -5 && rep[c] == -5 && worst[c] == -5, "a per-cluster output written");
    };
    int branches = 0;
    auto refuse = [&](const problem &q, bool d = true, bool c = true, bool o = true, bool j = true, bool v = true) {
        CHECK(!call(q, d ? q.D.data() : nullptr, c ? q.cof.data() : nullptr, o ? own.data() : nullptr, j ? aj.data() : nullptr, v ? av.data() : nullptr),
              "bad argument %d accepted", branches);
        untouched();
        ++branches;
    };
    problem q = p;
    refuse(q, false);
    refuse(q, true, false);
    refuse(q, true, true, false);
    refuse(q, true, true, true, false);
    refuse(q, true, true, true, true, false);
    q.k_alt = -1, refuse(q), q.k_alt = 65, refuse(q), q = p;
    q.nq = -1, refuse(q), q = p;
    q.K = -1, refuse(q), q = p;
    q.K = 1LL << 31, q.ld = 1LL << 31, refuse(q), q = p;
    q.ld = q.K - 1, refuse(q), q = p;
    q.qs[2] = 0, refuse(q), q = p;
    q.cs[4] = 0, refuse(q), q = p;
    q.cof[1] = 5, refuse(q), q.cof[1] = -2, refuse(q), q = p;
    q.K = 0, q.ld = 0, q.cof.assign(4, -1), q.cof[3] = 0, refuse(q); // K == 0 takes rows of no cluster only
    q.cof[3] = -1;
    CHECK(call(q, nullptr, q.cof.data(), own.data(), aj.data(), av.data()), "K == 0 with every row in no cluster refused");
    for (float x : own) CHECK(x == NS_MAXF, "own without clusters");
    for (int32_t x : aj) CHECK(x == -1, "alternatives without clusters");
    printf("bad arguments: %d refused, nothing written\n", branches);
}

int main()
{
    keys();
    printf("keys and leave-out rule\n");
    // the shapes (nq, K) of the test suite's case list, the empty sides, then a sweep
    const int64_t shapes[][2] = {{1, 1}, {2, 2}, {5, 1}, {130, 3}, {300, 129}, {257, 260}, {64, 700}, {0, 6}, {6, 0}, {0, 0}};
    const int ks[] = {0, 1, 10, 64};
    int64_t runs = 0;
    for (auto &s : shapes)
        for (int k : ks)
            for (int32_t mx : {0, 8}) {
                problem p = make(s[0], s[1], k, mx);
                run_and_check(p, true);
                run_and_check(p, false);
                runs += 2;
            }
    printf("case list: %lld runs\n", (long long)runs);
    runs = 0;
    for (int t = 0; t < 300; ++t) {
        problem p = make((int64_t)(rnd() % 12), (int64_t)(rnd() % 12), (int32_t)(rnd() % 5), (int32_t)(rnd() % 3 ? 6 + rnd() % 8 : 0));
        run_and_check(p, (rnd() & 1) != 0);
        ++runs;
    }
    printf("sweep: %lld runs\n", (long long)runs);
    bad_arguments();
    printf("ok\n");
    return 0;
}
