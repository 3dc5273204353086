// embed_file.hip -- icl_embed_file: GetImageEmbedding(path) from N goroutines (workflow.go:156-175), coalesced into batched forward passes.
//
// The reference serialises its batch-1 forward passes behind NetMutex (embeddings.go:133).  Here concurrent callers are
// COALESCED: every caller decodes and resizes its own file in parallel, then joins a per-context queue; the first one
// to arrive becomes the leader, waits a short window (or until a full batch has gathered), runs ONE forward pass over
// everything queued and hands each caller its row.  fp32 rows do not depend on what else is in the batch (every output
// pixel is its own in-order sum), so results equal the one-at-a-time path bit for bit.
#include "icl_common.h"
#include "jpeg_stage.h"
#include "resnet_model.h"

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <new>
#include <vector>

struct icl_file_req {
    const uint8_t *img;
    float *out;
    int head;
    int rc = ICL_OK;
    bool done = false;
    std::string err;
};
struct icl_file_batcher {
    std::mutex m;
    std::condition_variable cv;
    std::vector<icl_file_req *> pending;
    bool leader = false;
    int inflight = 0; // callers inside icl_embed_file (decoding, queued or being served): a leader stops waiting once all of them are queued
    int prec = ICL_PREC_FP32;
    int window_us = 2000;
    int max_batch = 256;
    bool fail_next = false; // ICL_FILE_FAIL_NEXT_LEADER: the next batch leader gives up right after taking its requests
    int64_t batches = 0, images = 0; // statistics (icl_file_batch_stats)
};
static icl_file_batcher *file_batcher(icl_ctx *ctx)
{
    static std::mutex gm;
    std::lock_guard<std::mutex> lk(gm);
    if (!ctx->file_batcher) ctx->file_batcher = new icl_file_batcher();
    return (icl_file_batcher *)ctx->file_batcher;
}
void icl_file_batcher_free(icl_ctx *ctx)
{
    delete (icl_file_batcher *)ctx->file_batcher;
    ctx->file_batcher = nullptr;
}

extern "C" int icl_set_file_options(icl_ctx *ctx, int prec, int window_us, int max_batch)
{
    const bool fail_next = (prec & ICL_FILE_FAIL_NEXT_LEADER) != 0;
    prec &= ~ICL_FILE_FAIL_NEXT_LEADER;
    if (!ctx || !prec_ok(prec) || window_us < 0 || max_batch < 1 || max_batch > 4096)
        return icl_fail(ctx, ICL_ERR_ARG, "icl_set_file_options: bad argument");
    icl_file_batcher *b = file_batcher(ctx);
    std::lock_guard<std::mutex> lk(b->m);
    b->fail_next = fail_next;
    b->prec = prec;
    b->window_us = window_us;
    b->max_batch = max_batch;
    return ICL_OK;
}

extern "C" int icl_file_batch_stats(icl_ctx *ctx, int64_t *batches, int64_t *images)
{
    if (!ctx) return ICL_ERR_ARG;
    icl_file_batcher *b = file_batcher(ctx);
    std::lock_guard<std::mutex> lk(b->m);
    if (batches) *batches = b->batches;
    if (images) *images = b->images;
    return ICL_OK;
}

// One caller of the queue, with its image as a file or as a memory source (icl_embed_file / icl_embed_image_mem: a batch may mix them).
static int embed_one(icl_ctx *ctx, const ingest_src &src, int head, float *out, const char *what)
{
    if (!head_ok(head)) return icl_fail(ctx, ICL_ERR_ARG, "head must be 2048 or 1000");
    return no_throw(ctx, what, [&]() -> int {
        icl_file_batcher *b = file_batcher(ctx);
        struct inflight_guard { // counts this caller in from before it queues until it leaves, whatever the exit
            icl_file_batcher *b;
            explicit inflight_guard(icl_file_batcher *bb) : b(bb)
            {
                std::lock_guard<std::mutex> g(b->m);
                ++b->inflight;
            }
            ~inflight_guard()
            {
                std::lock_guard<std::mutex> g(b->m);
                --b->inflight;
                b->cv.notify_all();
            }
        };
        inflight_guard ig(b);
        std::vector<uint8_t> img((size_t)ICL_IMG_BYTES);
        ICL_TRY(icl_read_image_224(ctx, src, img.data())); // decode + resize run on the caller's thread, in parallel with other callers
        icl_file_req me;
        me.img = img.data();
        me.out = out;
        me.head = head;
        std::unique_lock<std::mutex> lk(b->m);
        b->pending.push_back(&me);
        b->cv.notify_all(); // a waiting leader re-checks whether its batch is full / everybody who entered is queued
        while (!me.done) {
            if (b->leader) { // someone else is collecting or running a batch: wait for my row (or for the leadership)
                b->cv.wait(lk);
                continue;
            }
            b->leader = true;
            // From here on this thread owes every request it takes a result: whatever goes wrong (bad_alloc in the slab copies,
            // an exception out of the forward pass) each taken request is completed with an error, the leadership is given up and
            // everybody is woken -- a leader that left with `leader` still set would block every later caller for good.
            std::vector<icl_file_req *> take;
            auto finish = [&](int rc, const char *why) { // lock held
                for (icl_file_req *r : take)
                    if (!r->done) {
                        if (rc != ICL_OK) {
                            r->rc = rc;
                            try {
                                r->err = why;
                            } catch (...) {
                            }
                        }
                        r->done = true;
                    }
                b->leader = false;
                b->cv.notify_all(); // followers pick up their rows; one of the still-pending callers becomes the next leader
            };
            try {
                // the window only matters while other callers are still decoding: a lone caller (or the last of a burst) runs at once
                if (b->window_us > 0)
                    b->cv.wait_for(lk, std::chrono::microseconds(b->window_us),
                                   [&] { return (int)b->pending.size() >= b->max_batch || (int)b->pending.size() >= b->inflight; });
                take.swap(b->pending);
                if ((int)take.size() > b->max_batch) {
                    b->pending.assign(take.begin() + b->max_batch, take.end());
                    take.resize((size_t)b->max_batch);
                }
                const int prec = b->prec;
                const bool give_up = b->fail_next; // icl_set_file_options(ICL_FILE_FAIL_NEXT_LEADER): one leader fails as if out of memory
                b->fail_next = false;
                lk.unlock();
                if (give_up) throw std::bad_alloc();
                for (int hd : {ICL_HEAD_POOLED, ICL_HEAD_DENSE0}) { // one forward pass per requested head
                    std::vector<icl_file_req *> grp;
                    for (icl_file_req *r : take)
                        if (r->head == hd) grp.push_back(r);
                    if (grp.empty()) continue;
                    std::vector<uint8_t> slab(grp.size() * (size_t)ICL_IMG_BYTES);
                    std::vector<float> res(grp.size() * (size_t)hd);
                    for (size_t i = 0; i < grp.size(); ++i) memcpy(&slab[i * (size_t)ICL_IMG_BYTES], grp[i]->img, (size_t)ICL_IMG_BYTES);
                    const int rc = icl_embed_u8(ctx, slab.data(), (int64_t)grp.size(), hd, prec, res.data());
                    const std::string err = rc ? ctx->err : std::string();
                    for (size_t i = 0; i < grp.size(); ++i) {
                        grp[i]->rc = rc;
                        grp[i]->err = err;
                        if (rc == ICL_OK) memcpy(grp[i]->out, &res[i * (size_t)hd], (size_t)hd * 4);
                    }
                }
                lk.lock();
                b->batches += 1;
                b->images += (int64_t)take.size();
                finish(ICL_OK, "");
            } catch (...) {
                if (!lk.owns_lock()) lk.lock();
                if (take.empty()) take.swap(b->pending); // failed before the batch was cut: nobody may be left waiting for this leader
                finish(ICL_ERR_NOMEM, "icl_embed_file: the batch leader ran out of memory");
            }
        }
        if (me.rc != ICL_OK) return icl_fail(ctx, me.rc, "%s", me.err.c_str());
        return ICL_OK;
    });
}

extern "C" int icl_embed_file(icl_ctx *ctx, const char *path, int head, float *out)
{
    if (!ctx || !path || !out) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_file: bad argument");
    return embed_one(ctx, ingest_src{path, nullptr, 0, 0}, head, out, "icl_embed_file");
}

extern "C" int icl_embed_image_mem(icl_ctx *ctx, const uint8_t *data, int64_t bytes, int head, float *out)
{
    if (!ctx || !out) return icl_fail(ctx, ICL_ERR_ARG, "icl_embed_image_mem: bad argument");
    return embed_one(ctx, ingest_src{nullptr, data, bytes, 0}, head, out, "icl_embed_image_mem");
}
