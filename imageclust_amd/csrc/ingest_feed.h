// ingest_feed.h -- an ordered, bounded feed: worker threads produce the results of items 0 .. n-1, one consumer receives them in index
// order.  Host-only and self-contained (no HIP header, nothing of icl_common.h), so that a plain host compiler and its sanitizers can
// build and run it (tests/ingest_feed_main.cpp).  jpeg_gpu.hip feeds its slab builder through it: the items are files.
//
// Admission: a worker claims the next index only while it is less than `window` items ahead of the consumer and the results waiting
// for the consumer hold less than `budget` bytes -- except for the item the consumer waits for, which is always admitted (progress:
// a single result may be larger than the whole budget).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

template <class R> class ingest_feed {
public:
    using produce_fn = std::function<std::unique_ptr<R>(int64_t)>; // runs on a worker thread; nullptr: no memory even for the result
    using bytes_fn = std::function<int64_t(const R &)>;            // what a result counts against the budget while it waits

    ingest_feed(int64_t n, int threads, int64_t window, int64_t budget, produce_fn produce, bytes_fn bytes_of)
        : n_(n), window_(window), budget_(budget), produce_(std::move(produce)), bytes_of_(std::move(bytes_of)), res_((size_t)n)
    {
        try {
            for (int t = 0; t < threads; ++t) pool_.emplace_back([this] { work(); });
        } catch (...) { // (a thread could not be started: no destructor runs for a half-built feed)
            shut();
            throw;
        }
    }
    ~ingest_feed() { shut(); } // stops the workers and joins them, whatever the consumer has taken
    ingest_feed(const ingest_feed &) = delete;
    ingest_feed &operator=(const ingest_feed &) = delete;

    int64_t taken() const { return next_pack_; } // (consumer thread only) items handed over so far; peek / take while taken() < n

    // The next item in index order, once it is there; nullptr when a worker ran out of memory (the feed has stopped: the call fails).
    const R *peek()
    {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return res_[(size_t)next_pack_] != nullptr || oom_; });
        return oom_ ? nullptr : res_[(size_t)next_pack_].get();
    }

    // Hands over the item peek() returned, releases its bytes from the budget and wakes the workers.
    std::unique_ptr<R> take()
    {
        std::lock_guard<std::mutex> lk(m_);
        std::unique_ptr<R> r = std::move(res_[(size_t)next_pack_]);
        pending_bytes_ -= bytes_of_(*r);
        ++next_pack_;
        cv_.notify_all();
        return r;
    }

private:
    void work()
    {
        for (;;) {
            int64_t i;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] {
                    return stop_ || next_claim_ >= n_ || next_claim_ == next_pack_ || (next_claim_ < next_pack_ + window_ && pending_bytes_ < budget_);
                });
                if (stop_ || next_claim_ >= n_) return;
                i = next_claim_++;
            }
            std::unique_ptr<R> r;
            try {
                r = produce_(i);
            } catch (...) { // (produce reports through its result; whatever escapes it ends the call like a failed allocation)
            }
            std::lock_guard<std::mutex> lk(m_);
            if (!r) { // the consumer waits for this item: it must learn that it will not come
                oom_ = true;
                stop_ = true;
            } else {
                pending_bytes_ += bytes_of_(*r);
                res_[(size_t)i] = std::move(r);
            }
            cv_.notify_all();
        }
    }

    void shut()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : pool_)
            if (t.joinable()) t.join();
    }

    const int64_t n_, window_, budget_;
    const produce_fn produce_;
    const bytes_fn bytes_of_;
    std::mutex m_;
    std::condition_variable cv_;
    std::vector<std::unique_ptr<R>> res_; // produced, not yet taken
    int64_t next_claim_ = 0, next_pack_ = 0, pending_bytes_ = 0;
    bool stop_ = false, oom_ = false;
    std::vector<std::thread> pool_;
};
