// decompress.cpp -- host side of the decompression step (include/tonk_compress.h
// tamd_decompress*): the streams' device memory, the job and message descriptors, and the
// launches of tamd_lz_decompress (unlz.hip).  The block reader itself is unlz.h.
#include "../../include/tonk_compress.h"
#include "combine.h"
#include "lz_host.h"
#include "unlz.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <mutex>
#include <string.h>
#include <vector>

extern "C" __global__ void tamd_lz_decompress(const tamd_unlz_job*, uint32_t, const tamd_unlz_msg*, const uint8_t*,
                                              uint8_t*, uint8_t*, uint32_t*, int32_t*);

namespace tamd {
namespace {

void launch(hipStream_t st, hipEvent_t e0, hipEvent_t e1, const tamd_unlz_job* jobs, uint32_t n_jobs,
            const tamd_unlz_msg* msgs, const uint8_t* in, uint8_t* out, uint8_t* scratch, uint32_t* restored,
            int32_t* status) {
    const dim3 grid((n_jobs + TAMD_UNLZ_WAVES - 1) / TAMD_UNLZ_WAVES), block(64 * TAMD_UNLZ_WAVES);
    if (e0)
        hipExtLaunchKernelGGL(tamd_lz_decompress, grid, block, 0, st, e0, e1, 0, jobs, n_jobs, msgs, in, out, scratch,
                              restored, status);
    else
        hipLaunchKernelGGL(tamd_lz_decompress, grid, block, 0, st, jobs, n_jobs, msgs, in, out, scratch, restored, status);
}

const uint32_t kGuard = 64;           // bytes kept around the batch's stream memory, checked after every launch
const uint8_t kGuardByte = 0xC7;
const size_t kQueuedMax = 4 * (size_t)TAMD_UNLZ_RING;  // uncompressed bytes a decompressor queues before it flushes

}  // namespace

struct Decompressor {
    uint32_t max = 0;
    int device = 0;
    uint8_t* stream = nullptr;  // device: TAMD_UNLZ_STREAM_BYTES (state + ring), from the first launch on
    bool started = false;       // a launch has initialised `stream`
    bool failed = false;
    bool queued = false;        // a call of this decompressor is in the current batch
    std::vector<uint8_t> q_bytes;   // InsertUncompressed messages waiting for the next launch
    std::vector<uint32_t> q_lens;
};

}  // namespace tamd

using namespace tamd;

// ---- the per-message interface: concurrent calls combined into one launch (combine.h) ----
namespace {
struct UnlzRequest : CombineRequest<Decompressor> {
    const uint8_t* block = nullptr;  // null: only the queued uncompressed messages (a flush)
    uint32_t bytes = 0;
    uint8_t* dest = nullptr;
    uint32_t dest_cap = 0;
    unsigned* restored = nullptr;
};
Combiner<UnlzRequest> g_combiner;

// leader-only launch state
struct UnlzBatchState : LeaderStream {
    Buffer in, out, scratch;  // in: jobs | msgs | bytes; out: restored[] | status[] | block outputs
} g_batch;

// Stream memory of destroyed decompressors, kept for the next ones (lz_host.h).
DevicePool<TAMD_UNLZ_STREAM_BYTES> g_streams;

// Runs one batch (leader, no lock held): per request one job = the decompressor's queued
// uncompressed messages in order, then its block.
void run_batch(const std::vector<UnlzRequest*>& b) {
    UnlzBatchState& S = g_batch;
    const int dev = b[0]->c->device;
    bool ok = S.use(dev);
    size_t n_msgs = 0, in_bytes = 0, out_bytes = 0, scratch_bytes = 0;
    for (UnlzRequest* r : b) {
        Decompressor* c = r->c;
        if (ok && !c->stream && !c->failed) {
            c->stream = g_streams.take(dev);
            if (!c->stream) c->failed = true;
        }
        n_msgs += c->q_lens.size() + (r->block ? 1 : 0);
        in_bytes += align16(c->q_bytes.size()) + align16(r->bytes);
        out_bytes += align16(c->max);
        if (c->max > TAMD_LZ_MAX_MESSAGE) scratch_bytes += align16(c->max);
    }
    const size_t n = b.size();
    const size_t o_msgs = align16(n * sizeof(tamd_unlz_job));
    const size_t o_data = o_msgs + align16(n_msgs * sizeof(tamd_unlz_msg));
    const size_t o_status = align16(n_msgs * 4), o_blocks = o_status + align16(n_msgs * 4);
    ok = ok && S.in.grow(o_data + in_bytes + 32, true) && S.out.grow(o_blocks + out_bytes, true) &&
         S.scratch.grow(scratch_bytes + 16, false);
    std::vector<size_t> last(n, 0);  // index of each request's block among the messages
    uint32_t n_jobs = 0;
    if (ok) {
        tamd_unlz_job* jb = (tamd_unlz_job*)S.in.h;
        tamd_unlz_msg* ms = (tamd_unlz_msg*)(S.in.h + o_msgs);
        size_t mi = 0, din = 0, dout = 0, scr = 0;
        for (size_t i = 0; i < n; ++i) {
            UnlzRequest* r = b[i];
            Decompressor* c = r->c;
            if (c->failed || !c->stream) continue;  // (left out of the launch: nothing touches a null stream)
            tamd_unlz_job& j = jb[n_jobs++];
            memset(&j, 0, sizeof(j));
            j.stream = c->stream;
            j.first = (uint32_t)mi;
            j.cap = c->max;
            j.flags = TAMD_UNLZ_KEEP | (c->started ? 0u : TAMD_UNLZ_FRESH);
            j.scratch = TAMD_UNLZ_NO_SCRATCH;
            if (c->max > TAMD_LZ_MAX_MESSAGE) {
                j.scratch = scr;
                scr += align16(c->max);
            }
            if (!c->q_bytes.empty()) memcpy(S.in.h + o_data + din, c->q_bytes.data(), c->q_bytes.size());
            size_t at = din;
            for (uint32_t len : c->q_lens) {
                tamd_unlz_msg& m = ms[mi++];
                memset(&m, 0, sizeof(m));
                m.in = at;
                m.bytes = len;
                m.flags = TAMD_UNLZ_MSG_QUIET;
                at += len;
            }
            din += align16(c->q_bytes.size());
            if (r->block) {
                memcpy(S.in.h + o_data + din, r->block, r->bytes);
                tamd_unlz_msg& m = ms[mi];
                memset(&m, 0, sizeof(m));
                m.in = din;
                m.out = dout;
                m.bytes = r->bytes;
                m.flags = TAMD_UNLZ_MSG_BLOCK;
                last[i] = mi++;
                din += align16(r->bytes);
            }
            dout += align16(c->max);
            j.count = (uint32_t)mi - j.first;
        }
        if (n_jobs) {
            ok = hipMemcpyAsync(S.in.d, S.in.h, o_data + in_bytes, hipMemcpyHostToDevice, S.st) == hipSuccess;
            if (ok) {
                launch(S.st, nullptr, nullptr, (const tamd_unlz_job*)S.in.d, n_jobs, (const tamd_unlz_msg*)(S.in.d + o_msgs),
                       S.in.d + o_data, S.out.d + o_blocks, S.scratch.d, (uint32_t*)S.out.d, (int32_t*)(S.out.d + o_status));
                ok = hipGetLastError() == hipSuccess;
            }
            ok = ok && hipMemcpyAsync(S.out.h, S.out.d, o_blocks + out_bytes, hipMemcpyDeviceToHost, S.st) == hipSuccess;
            ok = ok && hipStreamSynchronize(S.st) == hipSuccess;
        }
    }
    size_t dout = 0;
    for (size_t i = 0; i < n; ++i) {
        UnlzRequest* r = b[i];
        Decompressor* c = r->c;
        if (c->failed || !c->stream) {
            c->failed = true;
            r->rc = -2;
            continue;
        }
        c->started = true;
        c->q_bytes.clear();
        c->q_lens.clear();
        r->rc = 0;
        if (!ok) {
            c->failed = true;
            r->rc = -2;
        } else if (r->block) {
            const int32_t st = ((const int32_t*)(S.out.h + o_status))[last[i]];
            const uint32_t got = ((const uint32_t*)S.out.h)[last[i]];
            if (st != 0) {
                c->failed = true;  // the reference's "Decompress fails, connection closes"
                r->rc = -16 + st;  // (-17 .. -30: the block reader's reason, unlz.h)
            } else if (got > r->dest_cap) {
                c->failed = true;  // never a partial write
                r->rc = -4;
            } else {
                memcpy(r->dest, S.out.h + o_blocks + dout, got);
                *r->restored = got;
            }
        }
        dout += align16(c->max);
    }
}
}  // namespace

extern "C" void* tamd_decompressor_create(unsigned max_bytes) {
    if (max_bytes == 0 || max_bytes > TAMD_UNLZ_RING) return nullptr;
    if (!device_ok()) return nullptr;
    Decompressor* c = new Decompressor();
    c->max = max_bytes;
    hipGetDevice(&c->device);
    return c;
}

extern "C" void tamd_decompressor_destroy(void* dp) {
    Decompressor* c = (Decompressor*)dp;
    if (!c) return;
    g_combiner.wait_idle(c);
    if (c->stream) g_streams.put(c->device, c->stream);
    delete c;
}

extern "C" void tamd_decompressor_insert_uncompressed(void* dp, const uint8_t* data, unsigned bytes) {
    Decompressor* c = (Decompressor*)dp;
    // (a message outside 1..max is ignored, as MessageDecompressor::InsertUncompressed does)
    if (!c || !data || bytes == 0 || bytes > c->max || c->failed) return;
    c->q_bytes.insert(c->q_bytes.end(), data, data + bytes);
    c->q_lens.push_back(bytes);
    if (c->q_bytes.size() > kQueuedMax) {  // bounded: flush without a block
        UnlzRequest req;
        req.c = c;
        g_combiner.submit(req, run_batch);
    }
}

extern "C" int tamd_decompressor_decompress(void* dp, const uint8_t* block, unsigned bytes, uint8_t* dest,
                                            unsigned dest_cap, unsigned* restored) {
    Decompressor* c = (Decompressor*)dp;
    if (restored) *restored = 0;
    if (!c || !block || !dest || !restored || bytes == 0) return -1;
    if (c->failed) return -2;
    if (bytes > c->max) {  // (no such block from a compressor of the same maximum)
        c->failed = true;
        return -1;
    }
    UnlzRequest req;
    req.c = c;
    req.block = block;
    req.bytes = bytes;
    req.dest = dest;
    req.dest_cap = dest_cap;
    req.restored = restored;
    return g_combiner.submit(req, run_batch);
}

extern "C" int tamd_decompress_batch(const void* dev_in, uint32_t n_streams, uint32_t n_msgs, const uint32_t* in_bytes,
                                     const uint8_t* is_block, uint32_t max_bytes, void* dev_out, uint32_t* restored_host,
                                     int32_t* status_host, float* kernel_ms) {
    if (!dev_in || !in_bytes || !is_block || !dev_out || !restored_host || !status_host || !n_streams || !n_msgs ||
        !max_bytes || max_bytes > TAMD_UNLZ_RING)
        return -1;
    if (!device_ok()) return -3;
    const uint64_t total = (uint64_t)n_streams * n_msgs;
    if (total > 0x7fffffffull) return -1;
    std::vector<tamd_unlz_job> jobs(n_streams);
    std::vector<tamd_unlz_msg> msgs(total);
    const bool big = max_bytes > TAMD_LZ_MAX_MESSAGE;
    const size_t scratch_each = align16(max_bytes);
    // persistent launch state (grown on demand)
    static std::mutex mu;
    static hipStream_t st = nullptr;
    static hipEvent_t e0 = nullptr, e1 = nullptr;
    static Buffer streams, desc, result, scratch;
    std::lock_guard<std::mutex> g(mu);
    bool ok = true;
    if (!st) ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&e0) == hipSuccess &&
                  hipEventCreate(&e1) == hipSuccess;
    const size_t stream_bytes = (size_t)n_streams * TAMD_UNLZ_STREAM_BYTES;
    const size_t o_msgs = align16(jobs.size() * sizeof(tamd_unlz_job));
    const size_t desc_bytes = o_msgs + total * sizeof(tamd_unlz_msg);
    const size_t o_status = align16(total * 4), o_guard = o_status + align16(total * 4);
    ok = ok && streams.grow(stream_bytes + 2 * kGuard, false) && desc.grow(desc_bytes, false) &&
         result.grow(o_guard + 2 * kGuard, false) && scratch.grow(big ? scratch_each * n_streams : 16, false);
    if (!ok) return -2;
    uint8_t* const base = streams.d + kGuard;
    for (uint32_t s = 0; s < n_streams; ++s) {
        tamd_unlz_job& j = jobs[s];
        memset(&j, 0, sizeof(j));
        j.stream = base + (size_t)s * TAMD_UNLZ_STREAM_BYTES;
        j.first = (uint32_t)((uint64_t)s * n_msgs);
        j.count = n_msgs;
        j.cap = max_bytes;
        j.flags = TAMD_UNLZ_FRESH;
        j.scratch = big ? (uint64_t)s * scratch_each : TAMD_UNLZ_NO_SCRATCH;
    }
    for (uint64_t i = 0; i < total; ++i) {
        tamd_unlz_msg& m = msgs[i];
        memset(&m, 0, sizeof(m));
        m.in = m.out = i * max_bytes;
        m.bytes = in_bytes[i];
        m.flags = is_block[i] ? TAMD_UNLZ_MSG_BLOCK : 0u;
    }
    // guard bytes before and after the streams' memory: set before, read back after the launch
    ok = hipMemsetAsync(streams.d, kGuardByte, kGuard, st) == hipSuccess &&
         hipMemsetAsync(base + stream_bytes, kGuardByte, kGuard, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(desc.d, jobs.data(), jobs.size() * sizeof(tamd_unlz_job), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(desc.d + o_msgs, msgs.data(), total * sizeof(tamd_unlz_msg), hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        launch(st, e0, e1, (const tamd_unlz_job*)desc.d, n_streams, (const tamd_unlz_msg*)(desc.d + o_msgs),
               (const uint8_t*)dev_in, (uint8_t*)dev_out, scratch.d, (uint32_t*)result.d, (int32_t*)(result.d + o_status));
        ok = hipGetLastError() == hipSuccess;
    }
    uint8_t guard[2 * kGuard];
    ok = ok && hipMemcpyAsync(restored_host, result.d, total * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(status_host, result.d + o_status, total * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(guard, streams.d, kGuard, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(guard + kGuard, base + stream_bytes, kGuard, hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) return -2;
    for (uint32_t i = 0; i < 2 * kGuard; ++i)
        if (guard[i] != kGuardByte) return -5;  // a write left the streams' memory
    if (kernel_ms) {
        float ms = 0;
        hipEventElapsedTime(&ms, e0, e1);
        *kernel_ms = ms;
    }
    return 0;
}

extern "C" int tamd_decompress_batch_host(const void* host_in, uint32_t n_streams, uint32_t n_msgs,
                                          const uint32_t* in_bytes, const uint8_t* is_block, uint32_t max_bytes,
                                          void* host_out, uint32_t* restored_host, int32_t* status_host, float* kernel_ms) {
    if (!host_in || !host_out || !n_streams || !n_msgs || !max_bytes) return -1;
    if (!device_ok()) return -3;
    const size_t bytes = (size_t)n_streams * n_msgs * max_bytes;
    void *d_in = nullptr, *d_out = nullptr;
    int rc = -2;
    // (32 readable bytes after the last input slot; output slots a message does not fill keep
    // what host_out held)
    if (hipMalloc(&d_in, bytes + 32) == hipSuccess && hipMalloc(&d_out, bytes) == hipSuccess &&
        hipMemcpy(d_in, host_in, bytes, hipMemcpyHostToDevice) == hipSuccess &&
        hipMemset((uint8_t*)d_in + bytes, 0, 32) == hipSuccess &&
        hipMemcpy(d_out, host_out, bytes, hipMemcpyHostToDevice) == hipSuccess) {
        rc = tamd_decompress_batch(d_in, n_streams, n_msgs, in_bytes, is_block, max_bytes, d_out, restored_host, status_host,
                                   kernel_ms);
        if (rc == 0 && hipMemcpy(host_out, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = -2;
    }
    if (d_in) hipFree(d_in);
    if (d_out) hipFree(d_out);
    return rc;
}
