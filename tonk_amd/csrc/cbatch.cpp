// cbatch.cpp -- include/tonk_compress_batch.h: batched, stateful compression and decompression of
// messages in the caller's device memory.  A handle is the shared core (handle.h: lock, stream,
// pinned descriptor and result staging) and, per stream, what the per-message interface keeps per
// compressor and decompressor (compress.cpp, decompress.cpp): the ring rule's bookkeeping on the
// host (lz.h RingTrack), the 64 KB ring and the decoder's state and ring on the device, one
// allocation per side between guard bytes.  A call is one descriptor copy, its launches back to
// back on the handle's stream, one result copy and one wait:
//
//   compress   : per pass (lz_pass.h) tamd_lz_place_ring (lz_place.hip) moves the pass's messages
//                into their rings, then tamd_lz_compress (lz.hip, unchanged) runs a job per message
//                over the ring and writes the block to the caller's slot.
//   decompress : tamd_lz_decompress (unlz.hip, unchanged), a job per stream that has items, its
//                items in order, inputs and outputs at absolute addresses.
#include "../../include/tonk_compress_batch.h"

#include "handle.h"
#include "kernel_abi.h"
#include "lz.h"
#include "lz_pass.h"
#include "unlz.h"

#include <memory>

extern "C" __global__ void tamd_lz_compress(const tamd_lz_job*, uint32_t, const tamd_lz_msg*, const uint8_t*,
                                            uint8_t*, uint32_t*, uint8_t*, unsigned long long*);
extern "C" __global__ void tamd_lz_decompress(const tamd_unlz_job*, uint32_t, const tamd_unlz_msg*, const uint8_t*,
                                              uint8_t*, uint8_t*, uint32_t*, int32_t*);

#include <stdlib.h>

using namespace tamd;

namespace {

enum { kPlace = 0, kCompress = 1, kDecompress = 2, kSpare = 3, kKinds = 4 };

const uint32_t kGuard = 64;  // bytes kept in front of and behind each side's memory, checked after every call
const uint8_t kGuardByte = 0xC7;
const size_t kRingPitch = TAMD_LZ_RING + TAMD_LZ_MIRROR;
const size_t kScratchBudget = (size_t)64 << 20;  // scratch of one launch's large messages; more: another launch

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// The FSE table blob on the current device, as compress.cpp's device_fse makes it (this library
// is linked without compress.cpp: libtonk_amd.so stays the same objects in the same order); null
// when it cannot be uploaded.  The handle owns it.
uint8_t* upload_fse() {
    std::vector<uint8_t> blob(TAMD_FSE_BYTES, 0);
    tamd_fse_blob(blob.data());
    // (TONK_AMD_LZ_FIT=0: the predefined sequence tables only, as the per-message interface reads it)
    if (getenv("TONK_AMD_LZ_FIT") && atoi(getenv("TONK_AMD_LZ_FIT")) == 0) blob[TAMD_FSE_FLAGS] |= TAMD_FSE_PREDEFINED_ONLY;
    uint8_t* d = nullptr;
    if (hipMalloc((void**)&d, TAMD_FSE_BYTES) != hipSuccess) return nullptr;
    if (hipMemcpy(d, blob.data(), TAMD_FSE_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
        hipFree(d);
        return nullptr;
    }
    return d;
}

struct Cbatch {
    HandleCore core;
    tamd_cbatch_params prm;
    uint8_t* rings = nullptr;    // kGuard | n_streams x kRingPitch | kGuard
    uint8_t* streams = nullptr;  // kGuard | n_streams x TAMD_UNLZ_STREAM_BYTES | kGuard
    uint8_t* fse = nullptr;      // the FSE table blob (lz.h)
    uint8_t* scratch = nullptr;  // messages above TAMD_LZ_MAX_MESSAGE, grown on demand up to the budget
    size_t scratch_cap = 0;
    std::vector<RingTrack> tracks;   // compressor side, by stream
    std::vector<uint8_t> started;    // decompressor side: a launch has initialised the stream's state
    LzPassPlan plan;
    std::vector<LzPlaced> placed;
    std::vector<uint32_t> order, at, cuts;        // a call's items in launch order, the passes' and launches' starts
    std::vector<uint32_t> count, first, touched;  // decompress: per-stream counters, the streams of a call

    uint8_t* ring(uint32_t s) const { return rings + kGuard + (size_t)s * kRingPitch; }
    uint8_t* stream(uint32_t s) const { return streams + kGuard + (size_t)s * TAMD_UNLZ_STREAM_BYTES; }
    size_t side_bytes(bool comp) const { return (size_t)prm.n_streams * (comp ? kRingPitch : (size_t)TAMD_UNLZ_STREAM_BYTES); }

    // One side's memory: zeros between guard bytes.
    bool allocate(uint8_t** p, size_t bytes) {
        if (!core.hip(hipMalloc((void**)p, bytes + 2 * kGuard), "hipMalloc")) return false;
        return core.hip(hipMemsetAsync(*p, 0, bytes + 2 * kGuard, core.stream), "hipMemsetAsync") &&
               core.hip(hipMemsetAsync(*p, kGuardByte, kGuard, core.stream), "hipMemsetAsync") &&
               core.hip(hipMemsetAsync(*p + kGuard + bytes, kGuardByte, kGuard, core.stream), "hipMemsetAsync");
    }
    bool need_scratch(size_t bytes) {  // (between calls: the device is idle)
        if (bytes <= scratch_cap) return true;
        if (scratch) hipFree(scratch);
        scratch = nullptr;
        scratch_cap = 0;
        if (!core.hip(hipMalloc((void**)&scratch, bytes), "hipMalloc")) return false;
        scratch_cap = bytes;
        return true;
    }
    // A side's guard bytes into the pinned result buffer at `at` (enqueued behind the call's launches).
    void fetch_guards(const uint8_t* side, size_t bytes, size_t at) {
        core.hip(hipMemcpyAsync(core.out.host + at, side, kGuard, hipMemcpyDeviceToHost, core.stream), "guard copy");
        core.hip(hipMemcpyAsync(core.out.host + at + kGuard, side + kGuard + bytes, kGuard, hipMemcpyDeviceToHost, core.stream), "guard copy");
    }
    bool guards_intact(size_t at) {
        for (uint32_t i = 0; i < 2 * kGuard; ++i)
            if (core.out.host[at + i] != kGuardByte) {
                if (!core.failed) core.error = "tonk_amd: a write left the handle's stream memory";
                core.failed = true;
                return false;
            }
        return true;
    }

    ~Cbatch() {  // (the core, destroyed after this, waits again and frees the rest)
        if (core.device < 0) return;
        hipSetDevice(core.device);
        if (core.stream) hipStreamSynchronize(core.stream);
        if (rings) hipFree(rings);
        if (streams) hipFree(streams);
        if (scratch) hipFree(scratch);
        if (fse) hipFree(fse);
    }
};

// Entry checks of a call that names streams; returns 0 with the handle locked and its device current.
int enter(Cbatch* s, std::unique_lock<std::mutex>& lk, uint32_t n, const uint32_t* stream, uint32_t side) {
    if (const int e = tamd::enter(s, lk)) return e;
    if (!(s->prm.sides & side)) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (stream[i] >= s->prm.n_streams) return -2;
    return 0;
}

}  // namespace

extern "C" {

void* tamd_cbatch_create(const tamd_cbatch_params* p, char* err, size_t err_len) {
    const uint32_t sides = TAMD_CBATCH_COMPRESS | TAMD_CBATCH_DECOMPRESS;
    // (the maximum's bounds are tamd_compressor_create's)
    if (!p || !p->n_streams || !p->max_message_bytes || p->max_message_bytes + p->max_message_bytes > TAMD_LZ_RING ||
        p->max_message_bytes > TAMD_LZ_DICT || !(p->sides & sides) || (p->sides & ~sides) || p->abut > 1)
        return fail(err, err_len, "bad parameters");
    std::string why = device_check(p->device, "messages are compressed and restored");
    if (!why.empty()) return fail(err, err_len, why);
    std::unique_ptr<Cbatch> s(new Cbatch());
    s->prm = *p;
    why = s->core.open(p->device);
    if (!why.empty()) return fail(err, err_len, why);
    HandleCore& c = s->core;
    const uint32_t ns = p->n_streams;
    if (p->sides & TAMD_CBATCH_COMPRESS) {
        s->fse = upload_fse();
        if (!s->fse) return fail(err, err_len, "tonk_amd: the FSE tables could not be uploaded");
        if (!s->allocate(&s->rings, s->side_bytes(true))) return fail(err, err_len, c.error);
        RingTrack t;
        t.max = p->max_message_bytes;
        s->tracks.assign(ns, t);
        s->plan.open.resize(ns);
    }
    if (p->sides & TAMD_CBATCH_DECOMPRESS) {
        if (!s->allocate(&s->streams, s->side_bytes(false))) return fail(err, err_len, c.error);
        s->started.assign(ns, 0);
        s->count.assign(ns, 0);
        s->first.assign(ns, 0);
    }
    if (!c.hip(hipStreamSynchronize(c.stream), "hipStreamSynchronize")) return fail(err, err_len, c.error);
    return s.release();
}

void tamd_cbatch_destroy(void* h) { destroy<Cbatch>(h); }
const char* tamd_cbatch_error(void* h) { return error_text<Cbatch>(h); }
void tamd_cbatch_set_timing(void* h, int on) { set_timing<Cbatch>(h, on); }
void tamd_cbatch_kernel_ms(void* h, double* out, unsigned n) { kernel_ms<Cbatch>(h, out, n, kKinds); }

int tamd_cbatch_compress(void* h, uint32_t n, const uint32_t* stream, const uint64_t* src, const uint32_t* bytes,
                         void* dev_out, uint64_t out_pitch, uint32_t* written) {
    Cbatch* s = (Cbatch*)h;
    if (!s || (n && (!stream || !src || !bytes || !dev_out || !written))) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream, TAMD_CBATCH_COMPRESS)) return e;
    HandleCore& c = s->core;
    const uint32_t maxb = s->prm.max_message_bytes;
    if (out_pitch < maxb) return -3;
    for (uint32_t i = 0; i < n; ++i)
        if (bytes[i] == 0 || bytes[i] > maxb || !src[i]) return -1;
    if (!n) return 0;
    if (out_pitch > 0x100000000ull / n) return -1;  // tamd_lz_msg.out is a 32-bit offset from dev_out

    // msgs (by item: the kernel's written[] comes back in item order) | jobs | placements, the last
    // two in launch order: by pass, a pass cut where its large messages' scratch passes the budget
    const size_t o_jobs = (size_t)n * sizeof(tamd_lz_msg), o_place = o_jobs + (size_t)n * sizeof(tamd_lz_job);
    const size_t up = o_place + (size_t)n * sizeof(LzPlaceDesc), o_guard = align16((size_t)n * 4);
    if (!c.room(up, o_guard + 2 * kGuard)) return -4;
    s->placed.resize(n);
    const uint32_t passes = s->plan.plan(n, stream, bytes, s->tracks.data(), s->prm.abut ? 0u : 1u, s->placed.data());
    s->at.assign(passes + 1, 0);
    for (uint32_t i = 0; i < n; ++i) ++s->at[s->placed[i].pass + 1];
    for (uint32_t p = 0; p < passes; ++p) s->at[p + 1] += s->at[p];
    s->order.resize(n);
    for (uint32_t i = 0; i < n; ++i) s->order[s->at[s->placed[i].pass]++] = i;  // (at[p] ends as pass p's end)
    tamd_lz_msg* ms = (tamd_lz_msg*)c.desc.host;
    tamd_lz_job* jb = (tamd_lz_job*)(c.desc.host + o_jobs);
    LzPlaceDesc* pl = (LzPlaceDesc*)(c.desc.host + o_place);
    std::vector<uint32_t>& cuts = s->cuts;  // launch k takes order[cuts[k], cuts[k + 1])
    cuts.clear();
    size_t scr = 0, scr_most = 0;
    uint32_t pass = ~0u;
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t i = s->order[k];
        const LzPlaced& p = s->placed[i];
        const size_t big = bytes[i] > TAMD_LZ_MAX_MESSAGE ? tamd_lz_scratch_bytes(bytes[i]) : 0;
        if (p.pass != pass || (big && scr + big > kScratchBudget)) {
            cuts.push_back(k);
            pass = p.pass;
            scr = 0;
        }
        uint8_t* const ring = s->ring(stream[i]);
        // positions are rebased to a multiple of the ring size below the window (same ring slots,
        // small numbers), as the per-message interface does
        const uint64_t base = p.win & ~(uint64_t)(TAMD_LZ_RING - 1);
        tamd_lz_msg& m = ms[i];
        memset(&m, 0, sizeof(m));
        m.pos = (uint32_t)(p.pos - base);
        m.len = bytes[i];
        m.win = (uint32_t)(p.win - base);
        m.out = (uint32_t)((uint64_t)i * out_pitch);
        m.cap = maxb;
        m.scratch = big ? (uint32_t)scr : TAMD_LZ_NO_SCRATCH;
        scr += big;
        if (scr > scr_most) scr_most = scr;
        tamd_lz_job& j = jb[k];
        memset(&j, 0, sizeof(j));
        j.buf = ring;
        j.mask = TAMD_LZ_RING - 1;
        j.first = i;
        j.count = 1;
        pl[k] = LzPlaceDesc{(uint64_t)(uintptr_t)ring, src[i], (uint32_t)(p.pos & (TAMD_LZ_RING - 1)), bytes[i]};
    }
    cuts.push_back(n);
    if (!s->need_scratch(scr_most)) return -4;
    const bool ok = c.run_all(up, o_guard, [&] {
        for (size_t k = 0; k + 1 < cuts.size(); ++k) {
            const uint32_t a = cuts[k], cnt = cuts[k + 1] - a;
            c.launch_timed(kPlace, [&] {
                hipLaunchKernelGGL(tamd_lz_place_ring, dim3((cnt + 15u) / 16u), dim3(256), 0, c.stream,
                                   (const LzPlaceDesc*)(c.desc.dev + o_place) + a, cnt);
            });
            c.launch_timed(kCompress, [&] {
                hipLaunchKernelGGL(tamd_lz_compress, dim3((cnt + TAMD_LZ_WAVES - 1) / TAMD_LZ_WAVES), dim3(64 * TAMD_LZ_WAVES), 0,
                                   c.stream, (const tamd_lz_job*)(c.desc.dev + o_jobs) + a, cnt, (const tamd_lz_msg*)c.desc.dev,
                                   s->fse, (uint8_t*)dev_out, (uint32_t*)c.out.dev, s->scratch, (unsigned long long*)nullptr);
            });
        }
        s->fetch_guards(s->rings, s->side_bytes(true), o_guard);
    });
    if (!ok || !s->guards_intact(o_guard)) return -4;
    const uint32_t* w = (const uint32_t*)c.out.host;
    for (uint32_t i = 0; i < n; ++i) {
        if (w[i] > maxb) {  // (never: the kernel's limit is below the message's size)
            c.error = "tonk_amd: the compression kernel returned a block above the maximum";
            c.failed = true;
            return -4;
        }
        written[i] = w[i];
    }
    return 0;
}

int tamd_cbatch_decompress(void* h, uint32_t n, const uint32_t* stream, const uint64_t* src, const uint32_t* bytes,
                           const uint8_t* is_block, void* dev_out, uint64_t out_pitch, uint32_t* restored, int32_t* status) {
    Cbatch* s = (Cbatch*)h;
    if (!s || (n && (!stream || !src || !bytes || !is_block || !dev_out || !restored || !status))) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream, TAMD_CBATCH_DECOMPRESS)) return e;
    HandleCore& c = s->core;
    const uint32_t maxb = s->prm.max_message_bytes;
    if (out_pitch < maxb) return -3;
    for (uint32_t i = 0; i < n; ++i)
        if (bytes[i] && bytes[i] <= maxb && !src[i]) return -1;  // (an entry the kernel refuses is never read)
    if (!n) return 0;

    // a job per stream with items, in the order the streams first appear; its messages in item order
    s->touched.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (s->count[stream[i]]++ == 0) s->touched.push_back(stream[i]);
    const uint32_t n_jobs = (uint32_t)s->touched.size();
    const size_t o_msgs = (size_t)n_jobs * sizeof(tamd_unlz_job), up = o_msgs + (size_t)n * sizeof(tamd_unlz_msg);
    const size_t o_status = align16((size_t)n * 4), o_guard = o_status + align16((size_t)n * 4);
    const bool big = maxb > TAMD_LZ_MAX_MESSAGE;
    const size_t scratch_each = align16(maxb);
    const uint32_t per_launch = big && kScratchBudget / scratch_each < n_jobs ? (uint32_t)(kScratchBudget / scratch_each) : n_jobs;
    bool ok = c.room(up, o_guard + 2 * kGuard) && (!big || s->need_scratch((size_t)per_launch * scratch_each));
    if (ok) {
        tamd_unlz_job* jb = (tamd_unlz_job*)c.desc.host;
        tamd_unlz_msg* ms = (tamd_unlz_msg*)(c.desc.host + o_msgs);
        uint32_t acc = 0;
        for (uint32_t k = 0; k < n_jobs; ++k) {
            const uint32_t st = s->touched[k];
            tamd_unlz_job& j = jb[k];
            memset(&j, 0, sizeof(j));
            j.stream = s->stream(st);
            j.first = acc;
            j.count = s->count[st];
            j.cap = maxb;
            j.flags = TAMD_UNLZ_KEEP | (s->started[st] ? 0u : TAMD_UNLZ_FRESH);
            j.scratch = big ? (uint64_t)(k % per_launch) * scratch_each : TAMD_UNLZ_NO_SCRATCH;
            s->first[st] = acc;
            acc += s->count[st];
            s->count[st] = 0;  // (from here on: the stream's next message slot)
        }
        s->order.resize(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t mi = s->first[stream[i]] + s->count[stream[i]]++;
            s->order[mi] = i;
            tamd_unlz_msg& m = ms[mi];
            memset(&m, 0, sizeof(m));
            m.in = src[i];  // (absolute: the kernel's bases are null)
            m.out = (uint64_t)(uintptr_t)dev_out + (uint64_t)i * out_pitch;
            m.bytes = bytes[i];
            m.flags = is_block[i] ? TAMD_UNLZ_MSG_BLOCK : TAMD_UNLZ_MSG_QUIET;
        }
    }
    for (uint32_t st : s->touched) s->count[st] = 0;
    if (!ok) return -4;
    ok = c.run_all(up, o_guard, [&] {
        for (uint32_t a = 0; a < n_jobs; a += per_launch) {
            const uint32_t cnt = n_jobs - a < per_launch ? n_jobs - a : per_launch;
            c.launch_timed(kDecompress, [&] {
                hipLaunchKernelGGL(tamd_lz_decompress, dim3((cnt + TAMD_UNLZ_WAVES - 1) / TAMD_UNLZ_WAVES), dim3(64 * TAMD_UNLZ_WAVES),
                                   0, c.stream, (const tamd_unlz_job*)c.desc.dev + a, cnt, (const tamd_unlz_msg*)(c.desc.dev + o_msgs),
                                   (const uint8_t*)nullptr, (uint8_t*)nullptr, s->scratch, (uint32_t*)c.out.dev,
                                   (int32_t*)(c.out.dev + o_status));
            });
        }
        s->fetch_guards(s->streams, s->side_bytes(false), o_guard);
    });
    if (!ok || !s->guards_intact(o_guard)) return -4;
    for (uint32_t st : s->touched) s->started[st] = 1;
    const uint32_t* r = (const uint32_t*)c.out.host;
    const int32_t* rc = (const int32_t*)(c.out.host + o_status);
    for (uint32_t mi = 0; mi < n; ++mi) {
        restored[s->order[mi]] = r[mi];
        status[s->order[mi]] = rc[mi];
    }
    return 0;
}

int tamd_cbatch_reset(void* h, uint32_t n, const uint32_t* stream, uint32_t sides) {
    Cbatch* s = (Cbatch*)h;
    if (!s || (n && !stream) || !sides || (sides & ~(TAMD_CBATCH_COMPRESS | TAMD_CBATCH_DECOMPRESS))) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream, sides)) return e;
    if ((sides & s->prm.sides) != sides) return -1;
    HandleCore& c = s->core;
    for (uint32_t i = 0; i < n; ++i) {
        if (sides & TAMD_CBATCH_COMPRESS) {
            // (the ring is zeroed as at creation: the bytes behind a fresh stream's messages are
            // the same for every connection that takes the slot)
            RingTrack t;
            t.max = s->prm.max_message_bytes;
            s->tracks[stream[i]] = t;
            c.hip(hipMemsetAsync(s->ring(stream[i]), 0, kRingPitch, c.stream), "hipMemsetAsync");
        }
        if (sides & TAMD_CBATCH_DECOMPRESS) s->started[stream[i]] = 0;  // (its next job starts TAMD_UNLZ_FRESH)
    }
    if (sides & TAMD_CBATCH_COMPRESS) c.hip(hipStreamSynchronize(c.stream), "hipStreamSynchronize");
    return c.failed ? -4 : 0;
}

}  // extern "C"
