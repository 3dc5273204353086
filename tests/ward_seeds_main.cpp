// ward_seeds_main.cpp -- the host rules of imageclust_amd/csrc/ward_seeds.h that every clustering call shares (the final cluster list
// from a merge log, the admission of a seeded problem, CalculateOptimalClusters): a stand-alone host program (no GPU, no HIP) that
// tests/test_ward_seeds_cpu.py builds with the address and undefined-behaviour sanitizers and runs.  Prints one line per rule and a
// final "ok".
#include "../imageclust_amd/csrc/ward_seeds.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// a valid log of T merges over m rows: each step joins two different live clusters, in either order
static std::vector<int32_t> random_log(int64_t m, int64_t T)
{
    std::vector<int32_t> live, log;
    for (int64_t i = 0; i < m; ++i) live.push_back((int32_t)i);
    for (int64_t t = 0; t < T; ++t) {
        const size_t x = (size_t)(rnd() % live.size());
        const int32_t a = live[x];
        live.erase(live.begin() + (long)x);
        const size_t y = (size_t)(rnd() % live.size());
        const int32_t b = live[y];
        live.erase(live.begin() + (long)y);
        log.push_back(a);
        log.push_back(b);
        live.push_back((int32_t)(m + t));
    }
    return log;
}

struct listing {
    std::vector<int32_t> id, rank, finals;
    int32_t n = -7;
    ward_list_result r;
};
static const int32_t SENTINEL = -77;
static listing run_list(int64_t m, const int32_t *sizes, int32_t min_size, const std::vector<int32_t> &log)
{
    listing L;
    L.id.assign((size_t)m + 1, SENTINEL); // (one entry behind the rows: the walk must not touch it)
    L.rank.assign((size_t)m + 1, SENTINEL);
    L.finals.assign(3, SENTINEL);
    L.r = ward_final_list(m, sizes, min_size, log.data(), (int64_t)log.size() / 2, L.id.data(), L.rank.data(), &L.n, &L.finals);
    return L;
}

// The rule written out the slow way: a cluster's member list is a's then b's; the final list is the live clusters in creation order.
static void check_against_member_lists(int64_t m, const std::vector<int32_t> &sizes, int32_t min_size, const std::vector<int32_t> &log, const listing &L)
{
    const int64_t T = (int64_t)log.size() / 2;
    std::vector<std::vector<int32_t>> mem((size_t)(m + T));
    std::vector<int64_t> items((size_t)(m + T), 0);
    std::vector<char> live((size_t)(m + T), 1);
    for (int64_t i = 0; i < m; ++i) mem[(size_t)i] = {(int32_t)i}, items[(size_t)i] = std::llabs((long long)sizes[(size_t)i]);
    for (int64_t t = 0; t < T; ++t) {
        const int32_t a = log[(size_t)(2 * t)], b = log[(size_t)(2 * t + 1)];
        mem[(size_t)(m + t)] = mem[(size_t)a];
        mem[(size_t)(m + t)].insert(mem[(size_t)(m + t)].end(), mem[(size_t)b].begin(), mem[(size_t)b].end());
        items[(size_t)(m + t)] = items[(size_t)a] + items[(size_t)b];
        live[(size_t)a] = live[(size_t)b] = 0;
    }
    std::vector<int32_t> id((size_t)m, -1), rank((size_t)m, -1), finals;
    int32_t next = 0;
    int64_t largest = 0;
    for (int64_t c = 0; c < m + T; ++c) {
        if (!live[(size_t)c]) continue;
        finals.push_back((int32_t)c);
        finals.push_back(mem[(size_t)c][0]);
        largest = std::max(largest, items[(size_t)c]);
        if (items[(size_t)c] < min_size) continue;
        for (size_t q = 0; q < mem[(size_t)c].size(); ++q) id[(size_t)mem[(size_t)c][q]] = next, rank[(size_t)mem[(size_t)c][q]] = (int32_t)q;
        ++next;
    }
    CHECK(L.r.kind == ward_list_result::OK && L.n == next && L.r.largest == largest && L.finals == finals, "m %lld: count %d (%d), largest %lld (%lld)",
          (long long)m, L.n, next, (long long)L.r.largest, (long long)largest);
    CHECK(std::equal(id.begin(), id.end(), L.id.begin()) && std::equal(rank.begin(), rank.end(), L.rank.begin()), "m %lld: ids or ranks", (long long)m);
    CHECK(L.id[(size_t)m] == SENTINEL && L.rank[(size_t)m] == SENTINEL, "m %lld: an entry behind the rows was written", (long long)m);
}

static int64_t check_null_sizes_are_ones()
{
    int64_t logs = 0;
    const int64_t ms[] = {0, 1, 2, 3, 17, 64};
    const int32_t mins[] = {1, 3};
    for (int64_t m : ms)
        for (int32_t min_size : mins)
            for (int rep = 0; rep < 8; ++rep) {
                rng_state = (uint64_t)(1000 * m + 10 * min_size + rep);
                const int64_t T = m < 2 ? 0 : rep == 0 ? 0 : rep == 1 ? m - 1 : (int64_t)(rnd() % (uint64_t)m);
                const std::vector<int32_t> log = random_log(m, T), ones((size_t)m, 1);
                const listing A = run_list(m, nullptr, min_size, log), B = run_list(m, ones.data(), min_size, log);
                CHECK(A.r.kind == ward_list_result::OK && B.r.kind == ward_list_result::OK, "m %lld: a valid log was refused", (long long)m);
                CHECK(A.id == B.id && A.rank == B.rank && A.n == B.n && A.finals == B.finals && A.r.largest == B.r.largest,
                      "m %lld, min_size %d, %lld merges: null sizes differ from ones", (long long)m, min_size, (long long)T);
                check_against_member_lists(m, ones, min_size, log, A);
                // ... and the same walk at seed granularity: sizes of 1 to 4 items, every third seed frozen
                std::vector<int32_t> sz((size_t)m);
                for (int64_t i = 0; i < m; ++i) sz[(size_t)i] = (int32_t)(1 + rnd() % 4) * (i % 3 == 2 ? -1 : 1);
                check_against_member_lists(m, sz, min_size, log, run_list(m, sz.data(), min_size, log));
                logs += 1;
            }
    return logs;
}

static void expect_refused(int64_t m, const int32_t *sizes, const std::vector<int32_t> &log, int kind, int64_t at, const char *text)
{
    const listing L = run_list(m, sizes, 1, log);
    CHECK((int)L.r.kind == kind && L.r.at == at, "%s: kind %d at %lld", text, (int)L.r.kind, (long long)L.r.at);
    CHECK(ward_list_text(L.r) == text, "%s: the text is '%s'", text, ward_list_text(L.r).c_str());
    CHECK(L.n == -7 && L.finals == std::vector<int32_t>(3, SENTINEL), "%s: n_clusters or finals written", text);
    for (size_t i = 0; i < L.id.size(); ++i) CHECK(L.id[i] == SENTINEL && L.rank[i] == SENTINEL, "%s: row %zu written", text, i);
}

static int check_bad_logs()
{
    const int C = ward_list_result::CORRUPT, Z = ward_list_result::ZERO_SIZE;
    const int32_t one2[] = {1, 1}, one4[] = {1, 2, -3, 1}, zero[] = {1, 0}, zero3[] = {2, -1, 0};
    // the logs tests/test_cluster_seeded_cpu.py gives icl_seeded_assign_ids, m = 2
    expect_refused(2, one2, {1, 1}, C, 0, "corrupt merge log at step 0 (1,1)");        // a == b
    expect_refused(2, one2, {2, 0}, C, 0, "corrupt merge log at step 0 (2,0)");        // id >= m + t
    expect_refused(2, one2, {1, 0, 1, 2}, C, 1, "corrupt merge log at step 1 (1,2)");  // a dead id
    expect_refused(2, one2, {-1, 0}, C, 0, "corrupt merge log at step 0 (-1,0)");      // id < 0
    // the same with null sizes, and deeper into a log
    expect_refused(2, nullptr, {1, 1}, C, 0, "corrupt merge log at step 0 (1,1)");
    expect_refused(2, nullptr, {0, -1}, C, 0, "corrupt merge log at step 0 (0,-1)");
    expect_refused(4, nullptr, {0, 1, 2, 3, 4, 6}, C, 2, "corrupt merge log at step 2 (4,6)"); // the step's own id
    expect_refused(4, one4, {0, 1, 4, 2, 5, 4}, C, 2, "corrupt merge log at step 2 (5,4)");    // dead merged cluster
    expect_refused(4, one4, {0, 1, 3, 3}, C, 1, "corrupt merge log at step 1 (3,3)");
    expect_refused(4, one4, {0, 1, 2, 1000000}, C, 1, "corrupt merge log at step 1 (2,1000000)");
    expect_refused(4, one4, {-2147483647 - 1, 1}, C, 0, "corrupt merge log at step 0 (-2147483648,1)");
    // a size of 0 is found before the log is read
    expect_refused(2, zero, {}, Z, 1, "seed 1 has size 0");
    expect_refused(3, zero3, {5, 5}, Z, 2, "seed 2 has size 0");
    return 13;
}

// ward_seed_admit against the rule written out: refusals first (items, then the first unfrozen seed above max_size), k, the clamp, the sizes
static void expect_admit(const std::vector<int32_t> &sz, int32_t min_size, int32_t max_size, int32_t k_target, int status, const char *why, int64_t k)
{
    const int64_t m = (int64_t)sz.size();
    std::vector<int32_t> eff((size_t)m + 1, SENTINEL);
    const ward_admission a = ward_seed_admit(m, sz.data(), min_size, max_size, k_target, eff.data());
    int64_t N = 0;
    for (int32_t s : sz) N += s < 0 ? -(int64_t)s : s;
    CHECK(a.status == status && a.N == N && a.why == why, "admit: status %d (%d), N %lld (%lld), why '%s' ('%s')", a.status, status, (long long)a.N, (long long)N,
          a.why.c_str(), why);
    CHECK(eff[(size_t)m] == SENTINEL, "admit: an entry behind the seeds was written");
    if (status != ICL_OK) {
        for (int64_t i = 0; i < m; ++i) CHECK(eff[(size_t)i] == SENTINEL, "admit: a refused problem's sizes were written");
        return;
    }
    const int64_t kmax = std::min<int64_t>(std::max<int64_t>(max_size, 1), std::max<int64_t>(N, 1));
    CHECK(a.k == k && a.kmax == kmax, "admit: k %lld (%lld), kmax %d (%lld)", (long long)a.k, (long long)k, a.kmax, (long long)kmax);
    for (int64_t i = 0; i < m; ++i) CHECK(eff[(size_t)i] == (sz[(size_t)i] < 0 ? kmax : sz[(size_t)i]), "admit: eff[%lld] = %d", (long long)i, eff[(size_t)i]);
}

static int check_admission()
{
    const int32_t P29 = 1 << 29, P30 = 1 << 30;
    expect_admit({P29, P29}, 1, P30, 0, ICL_ERR_UNSUPPORTED, "1073741824 items in all", 0);
    expect_admit({P29, -P29}, 1, P30, 1, ICL_ERR_UNSUPPORTED, "1073741824 items in all", 0); // (a frozen seed's items count, and k_target does not help)
    expect_admit({P29, P29 - 1}, 1, P30, 2, ICL_OK, "", 2);                                   // one item fewer is accepted
    // a frozen seed above max_size at index 1 is no refusal; the unfrozen ones at 3 and 4 are, and the first is named
    expect_admit({2, -9, 3, 7, 8}, 1, 6, 0, ICL_ERR_UNSUPPORTED, "seed 3 holds 7 items, above maxSize (6), and is not frozen", 0);
    expect_admit({2, -9, 3, 6, 6}, 1, 6, 0, ICL_OK, "", 15); // 26 items: lo = ceil(26 / 6) = 5, hi = 26 -> k = 15
    expect_admit({2, -9, 3, 6, 6}, 1, 6, 4, ICL_OK, "", 4);  // k_target > 0 is taken as it is
    expect_admit({2, -9, 3, 6, 6}, 1, 6, -1, ICL_OK, "", 15);
    int64_t k = -1;
    CHECK(ward_optimal_k(26, 1, 6, &k) == ICL_OK && k == 15, "ward_optimal_k(26, 1, 6) = %lld", (long long)k);
    CHECK(ward_optimal_k(10, 3, 6, &k) == ICL_OK && k == 2, "ward_optimal_k(10, 3, 6) = %lld", (long long)k); // lo 2, hi 3 -> 2
    CHECK(ward_optimal_k(7, 5, 6, &k) == ICL_ERR_CONSTRAINT && ward_optimal_k(3, 4, 6, &k) == ICL_ERR_CONSTRAINT, "lo > hi, total < min_size");
    CHECK(ward_optimal_k(5, 0, 6, &k) == ICL_ERR_CONSTRAINT && ward_optimal_k(5, 1, 0, &k) == ICL_ERR_CONSTRAINT && ward_optimal_k(5, 1, 6, nullptr) == ICL_ERR_ARG,
          "sizes below 1, null k");
    expect_admit({3, 4}, 5, 6, 0, ICL_ERR_CONSTRAINT, "cannot satisfy cluster size constraints with total items (7), minSize (5), and maxSize (6)", 0);
    expect_admit({3, 4}, 5, 6, 1, ICL_OK, "", 1);  // (k_target in front of the constraints)
    expect_admit({-1, -1, -1}, 1, 0, 2, ICL_OK, "", 2); // max_size below 1 (no unfrozen seed fits under it): kmax = 1
    expect_admit({-1, 1, -1}, 1, 0, 2, ICL_ERR_UNSUPPORTED, "seed 1 holds 1 items, above maxSize (0), and is not frozen", 0);
    expect_admit({1, -2}, 1, 100, 0, ICL_OK, "", 2); // max_size above N: kmax = N = 3, and the frozen seed gets it
    // m = 0: no items are fewer than any min_size; with a k_target the problem is accepted, kmax = 1
    expect_admit({}, 1, 6, 0, ICL_ERR_CONSTRAINT, "cannot satisfy cluster size constraints with total items (0), minSize (1), and maxSize (6)", 0);
    expect_admit({}, 2, 6, 3, ICL_OK, "", 3);
    return 14;
}

int main()
{
    const int64_t logs = check_null_sizes_are_ones();
    printf("null sizes are ones: %lld logs over m = 0, 1, 2, 3, 17, 64 and min_size = 1, 3; the member lists written out agree\n", (long long)logs);
    printf("bad logs: %d refused, each with its step and pair, nothing written\n", check_bad_logs());
    printf("admission: %d problems against the rule written out\n", check_admission());
    printf("ok\n");
    return 0;
}
