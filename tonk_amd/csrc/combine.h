// combine.h -- concurrent synchronous calls combined into shared launches (compress.cpp,
// decompress.cpp).
//
// Tonk compresses and decompresses each message on the connection's own thread and waits for the
// result (PacketCompression.cpp:70-118, 178-208).  One GPU round trip per message is slow next to
// zstd on the calling thread, so calls from different connections are combined: a caller queues
// its request; the first caller becomes the leader and runs every queued request as ONE batch
// (one upload, one launch, one download), then completes them and serves the requests that queued
// meanwhile.  A batch costs about one round trip however many connections it serves.
//
// Request: a struct derived from CombineRequest<Owner>; Owner (a compressor or decompressor) has
// `bool queued` and `int device`.  A batch holds at most one request per owner (an owner's
// messages are processed in call order) and one device.
#pragma once
#include <condition_variable>
#include <mutex>
#include <vector>

namespace tamd {

template <class Owner>
struct CombineRequest {
    Owner* c = nullptr;
    int rc = 0;
    bool done = false;
    std::condition_variable cv;  // its caller waits here: a batch wakes only its own callers
};

template <class Req>
class Combiner {
public:
    // Queues `req` and returns its rc once a batch has served it; `run(batch)` is called by the
    // leader with no lock held.
    template <class Run>
    int submit(Req& req, Run run) {
        std::unique_lock<std::mutex> lk(mu_);
        pending_.push_back(&req);
        // Wait while another caller leads; take over when it steps down with this request unserved.
        req.cv.wait(lk, [&req, this] { return req.done || !leader_; });
        if (req.done) return req.rc;
        leader_ = true;
        std::vector<Req*> batch, later;
        // The leader serves batches only until its own request is done, then hands leadership to a
        // waiting caller: its own path is never held by other connections' traffic.
        while (!req.done) {
            batch.clear();
            later.clear();
            for (Req* r : pending_) {
                if (r->c->queued || r->c->device != pending_[0]->c->device) later.push_back(r);
                else {
                    r->c->queued = true;
                    batch.push_back(r);
                }
            }
            pending_.swap(later);
            lk.unlock();
            run(batch);
            lk.lock();
            for (Req* r : batch) {
                r->c->queued = false;
                r->done = true;
                if (r != &req) r->cv.notify_one();
            }
            idle_cv_.notify_all();
        }
        leader_ = false;
        if (!pending_.empty()) pending_.front()->cv.notify_one();  // the next queued caller leads
        return req.rc;
    }

    // Returns once no call of `c` is queued or in flight (its owner is not calling it).
    template <class Owner>
    void wait_idle(Owner* c) {
        std::unique_lock<std::mutex> g(mu_);
        idle_cv_.wait(g, [c] { return !c->queued; });
    }

private:
    std::mutex mu_;
    std::condition_variable idle_cv_;  // wait_idle waits here for an owner's last call
    std::vector<Req*> pending_;
    bool leader_ = false;
};

}  // namespace tamd
