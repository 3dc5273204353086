// Stand-alone checks of ingest_feed.h (imageclust_amd/csrc), built and run by tests/test_ingest_feed_cpu.py under AddressSanitizer +
// UBSan and under ThreadSanitizer.  Exit status 0: every check held (the sanitizers end the program themselves on a finding).
#include "ingest_feed.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static std::atomic<int64_t> live_items{0};

struct item {
    int64_t index;
    std::vector<uint8_t> bytes;
    item(int64_t i, size_t nbytes) : index(i), bytes(nbytes, (uint8_t)i) { ++live_items; }
    ~item() { --live_items; }
};
using feed = ingest_feed<item>;

static int64_t bytes_of(const item &r) { return (int64_t)r.bytes.size(); }

// a pseudo-random 0 - 200 us of "decoding"
static void nap(int64_t i)
{
    uint64_t x = (uint64_t)i * 0x9E3779B97F4A7C15ull;
    x ^= x >> 29;
    std::this_thread::sleep_for(std::chrono::microseconds((x * 0xBF58476D1CE4E5B9ull >> 33) % 201));
}

// (a) n items arrive in index order, each exactly once
static void order(int threads)
{
    const int64_t n = 1000;
    std::vector<std::atomic<int>> produced((size_t)n);
    for (auto &p : produced) p = 0;
    {
        feed f(n, threads, 64, 1 << 20, [&](int64_t i) {
            nap(i);
            ++produced[(size_t)i];
            return std::unique_ptr<item>(new item(i, 100));
        }, bytes_of);
        for (int64_t k = 0; k < n; ++k) {
            CHECK(f.taken() == k);
            const item *p = f.peek();
            CHECK(p && p->index == k);
            std::unique_ptr<item> r = f.take();
            CHECK(r.get() == p && r->index == k && r->bytes.size() == 100 && r->bytes[0] == (uint8_t)k);
        }
        CHECK(f.taken() == n);
    }
    for (auto &p : produced) CHECK(p == 1);
    CHECK(live_items == 0);
}

// (b) no worker runs `window` or more items ahead of the consumer; an item larger than the whole byte budget still gets through
static void admission(int threads)
{
    const int64_t n = 1000, window = 8, budget = 1000, big = 50;
    std::atomic<int64_t> taken{0}; // raised before each take(): never below the feed's own count
    std::mutex m;
    int64_t max_ahead = -1;
    {
        feed f(n, threads, window, budget, [&](int64_t i) {
            {
                std::lock_guard<std::mutex> lk(m);
                max_ahead = std::max(max_ahead, i - taken.load());
            }
            nap(i);
            return std::unique_ptr<item>(new item(i, i == big ? 5 * (size_t)budget : 100));
        }, bytes_of);
        for (int64_t k = 0; k < n; ++k) {
            const item *p = f.peek();
            CHECK(p && p->index == k && (int64_t)p->bytes.size() == (k == big ? 5 * budget : 100));
            ++taken;
            f.take();
        }
    }
    CHECK(max_ahead >= 0 && max_ahead < window);
    CHECK(live_items == 0);
}

// (c) the consumer leaves after 10 of 1000 items while workers are inside produce
static void abandon(int threads)
{
    const int64_t n = 1000, window = 256;
    std::atomic<int64_t> inside{0}, started{0};
    {
        feed f(n, threads, window, 1 << 20, [&](int64_t i) {
            ++started;
            ++inside;
            nap(i);
            std::unique_ptr<item> r(new item(i, 100));
            --inside;
            return r;
        }, bytes_of);
        for (int64_t k = 0; k < 10; ++k) {
            CHECK(f.peek() != nullptr);
            CHECK(f.take()->index == k);
        }
        while (inside == 0 && started < 10 + window) std::this_thread::yield(); // (every admitted item produced already: nothing to wait for)
    }
    CHECK(inside == 0 && started < n);
    CHECK(live_items == 0);
}

// (d) produce has no memory for item 37: peek() says so, the consumer leaves, the feed joins
static void out_of_memory(int threads)
{
    const int64_t n = 1000, bad = 37;
    bool told = false;
    {
        feed f(n, threads, 64, 1 << 20, [&](int64_t i) {
            nap(i);
            return std::unique_ptr<item>(i == bad ? nullptr : new item(i, 100));
        }, bytes_of);
        while (f.taken() < n) {
            const item *p = f.peek();
            if (!p) {
                told = true;
                break;
            }
            CHECK(p->index == f.taken() && p->index < bad);
            f.take();
        }
        CHECK(f.taken() <= bad);
    }
    CHECK(told);
    CHECK(live_items == 0);
}

// (e) fewer items than threads, and none
static void small_n(int threads)
{
    {
        feed f(1, threads, 64, 1 << 20, [&](int64_t i) { return std::unique_ptr<item>(new item(i, 100)); }, bytes_of);
        const item *p = f.peek();
        CHECK(p && p->index == 0);
        CHECK(f.take()->index == 0 && f.taken() == 1);
    }
    {
        feed f(0, threads, 64, 1 << 20, [&](int64_t i) { return std::unique_ptr<item>(new item(i, 100)); }, bytes_of);
        CHECK(f.taken() == 0);
    }
    CHECK(live_items == 0);
}

int main()
{
    for (int threads : {1, 4, 16}) {
        order(threads);
        admission(threads);
        abandon(threads);
        out_of_memory(threads);
        small_n(threads);
        printf("threads %d: ok\n", threads);
    }
    return 0;
}
