// batch.cpp -- include/tonk_batch.h: batched encoders and decoders over the caller's own device
// packets.  One handle is n_streams connections, each a Context with an Encoder and a Decoder
// (as resident_backend.h pairs them), on one Device.  A call runs the control planes of the
// streams it names on the calling thread, moves the packets between the caller's layout and arena
// rows with the kernels of frame.hip, merges the streams' pending programs into one
// (Device::begin / fill / launch, the session's non-pipelined pass) and waits: every call is
// synchronous, so between calls nothing is in flight and every program launched has completed.
//
// Row ownership.  Added originals are copied into rows the codec owns (not borrowed): the codec
// releases them by its own rule (a packet leaves the encoder's window when it is acknowledged
// and the running sums no longer need it; the decoder's when its window moves on).  A ring of
// borrowed slots would be overwritten while a sum range still reads a packet.  A call's rows of
// one stream are allocated back to back and equal-length stretches are added as runs
// (Encoder::add_run, Decoder::add_run_inorder), so windows become segments and the programs read
// them as ACCR runs.  Freed rows are reused only after release_up_to(completed epoch).
#include "../../include/tonk_batch.h"

#include "decoder.h"
#include "device.h"
#include "frame.h"
#include "handle.h"

#include <memory>

using namespace tamd;

namespace {

enum { kFrame = 0, kUnframe = 1, kTails = 2, kKinds = 3 };

struct Batch {
    tamd_batch_params prm;
    Device dev;
    HandleCore core;  // (on dev's stream, which it does not own; destroyed before dev)
    struct Stream {
        std::unique_ptr<Context> ctx;  // (destroyed after its codecs)
        std::unique_ptr<Encoder> enc;
        std::unique_ptr<Decoder> dec;
        uint64_t call = 0;    // the call that last released its rows
        bool touched = false; // may have a pending program
    };
    std::vector<Stream> st;
    std::vector<uint32_t> touched;
    uint64_t call = 0;
    // index lists of a call by stream (a stable counting sort of the caller's list)
    std::vector<uint32_t> order, start;
    std::vector<RowId> rows;
    // measurement (tamd_batch_kernel_ms) beside the core's timer: bytes moved, the programs' share
    uint64_t moved[2] = {0, 0};
    double prog_ms0 = 0;
    uint64_t prog_n0 = 0;

    hipStream_t stream() const { return core.stream; }
    uint32_t max_recovery() const { return prm.max_packet_bytes + TAMD_BATCH_RECOVERY_OVERHEAD; }

    bool ok() {
        if (!core.failed && dev.failed()) {
            core.failed = true;
            core.error = dev.error();
        }
        return !core.failed;
    }
    // The first use of a stream in a call: everything launched has completed, so rows freed up to
    // the stream's last closed epoch are reusable.
    Stream& use(uint32_t s) {
        Stream& x = st[s];
        if (x.call != call) {
            x.call = call;
            x.ctx->rows.release_up_to(x.ctx->epoch - 1);
        }
        return x;
    }
    void touch(uint32_t s) {
        if (!st[s].touched) {
            st[s].touched = true;
            touched.push_back(s);
        }
    }

    // Wait for everything enqueued; read the timed launches' durations.
    bool sync() {
        dev.synchronize();
        core.timer.collect();
        return ok();
    }

    // (frame.h: the launch shape, shared with the host walk of the tests)
    static uint32_t waves_per_packet(uint32_t bytes) { return tamd_frame_waves(bytes); }
    static uint32_t grid(size_t n, uint32_t wpp) { return tamd_frame_grid(n, wpp); }

    // tamd_frame_rows over `d` (already in desc.host); enqueued only.
    void frame(size_t n, uint32_t largest) {
        if (!n || !ok()) return;
        Staging& desc = core.desc;
        const FrameDesc* h = (const FrameDesc*)desc.host;
        for (size_t i = 0; i < n; ++i) moved[0] += h[i].len;
        if (!core.hip(hipMemcpyAsync(desc.dev, desc.host, n * sizeof(FrameDesc), hipMemcpyHostToDevice, stream()), "descriptor copy"))
            return;
        const uint32_t wpp = waves_per_packet(largest);
        core.launch_timed(kFrame, [&] {
            hipLaunchKernelGGL(tamd_frame_rows, dim3(grid(n, wpp)), dim3(256), 0, stream(), (const FrameDesc*)desc.dev,
                               (uint32_t)n, dev.arena(), wpp);
        });
    }
    // tamd_unframe_rows over the records in desc.host, results into out.host; waits.  Without
    // `write` only the lengths and statuses are produced.
    bool unframe(size_t n, uint64_t pitch, uint32_t largest, bool write) {
        if (!n) return sync();
        Staging &desc = core.desc, &out = core.out;
        if (!ok() || !out.ensure(n * sizeof(UnframeOut))) return core.hip(hipErrorOutOfMemory, "staging allocation");
        if (!core.hip(hipMemcpyAsync(desc.dev, desc.host, n * sizeof(UnframeDesc), hipMemcpyHostToDevice, stream()), "descriptor copy"))
            return false;
        const uint32_t wpp = write ? waves_per_packet(largest) : 1u;
        core.launch_timed(kUnframe, [&] {
            hipLaunchKernelGGL(tamd_unframe_rows, dim3(grid(n, wpp)), dim3(256), 0, stream(), (const UnframeDesc*)desc.dev,
                               (uint32_t)n, (const uint8_t*)dev.arena(), pitch, (UnframeOut*)out.dev, write ? 1u : 0u, wpp);
        });
        core.hip(hipMemcpyAsync(out.host, out.dev, n * sizeof(UnframeOut), hipMemcpyDeviceToHost, stream()), "result copy");
        if (!sync()) return false;
        const UnframeOut* o = (const UnframeOut*)out.host;
        for (size_t i = 0; i < n && write; ++i) moved[1] += o[i].len;
        return true;
    }

    // Merge the pending programs of the streams touched in this call into one and enqueue it
    // (session.cpp's non-pipelined pass: scans, layout, fill, close the epochs, launch).
    void flush() {
        if (touched.empty() || !ok()) return;
        std::vector<Context*> cs;
        for (uint32_t s : touched) {
            st[s].touched = false;
            cs.push_back(st[s].ctx.get());
            st[s].ctx->prepare_flush();
        }
        touched.clear();
        dev.begin(cs.data(), cs.size());
        for (size_t i = 0; i < cs.size(); ++i) {
            dev.fill(i);
            cs[i]->finish_flush();
        }
        dev.launch();
    }

    // The caller's list sorted by stream, list order kept inside a stream: entries of stream s are
    // order[start[s] .. start[s + 1]).
    void sort_by_stream(uint32_t n, const uint32_t* stream) {
        start.assign(prm.n_streams + 1, 0);
        for (uint32_t i = 0; i < n; ++i) ++start[stream[i] + 1];
        for (uint32_t s = 0; s < prm.n_streams; ++s) start[s + 1] += start[s];
        order.resize(n);
        std::vector<uint32_t> at(start.begin(), start.end() - 1);
        for (uint32_t i = 0; i < n; ++i) order[at[stream[i]]++] = i;
    }
    // k rows of `bytes` each, back to back; false (none kept) when the stream's arena range is full.
    bool alloc_rows(Context& c, uint32_t k, uint32_t bytes) {
        rows.assign(k, kNoRow);
        for (uint32_t j = 0; j < k; ++j)
            if ((rows[j] = c.alloc(bytes)) == kNoRow) {
                for (uint32_t x = 0; x < j; ++x) c.rows.free_deferred(rows[x]);
                return false;
            }
        return true;
    }
    // The rows of a stretch of k packets of one stream; without them the codec is disabled (an
    // arena range that is full disables it, as in the C ABI).
    template <class Codec>
    bool stretch_rows(Codec& codec, Context& c, uint32_t k, uint32_t bytes) {
        if (!codec.disabled() && alloc_rows(c, k, bytes)) return true;
        codec.set_disabled();
        return false;
    }
    bool staging_failed() { return core.hip(hipErrorOutOfMemory, "staging allocation"); }
};

// Common entry checks; returns 0 with the handle locked by `lk`.
int enter(Batch* b, std::unique_lock<std::mutex>& lk, uint32_t n, const uint32_t* stream) {
    if (!b) return -1;
    lk = std::unique_lock<std::mutex>(b->core.mu);
    if (!b->ok()) return -4;
    for (uint32_t i = 0; i < n; ++i)
        if (stream[i] >= b->prm.n_streams) return -2;
    b->dev.bind_thread();
    ++b->call;
    return 0;
}

// What the two add calls share: packet i of the list is len[i] bytes at dev_payloads + i * pitch +
// offset[i] (a null offset: 0).  The list is walked stream by stream in list order; `stretch(s, x,
// idx, m, took)` is given what is left of stream s's entries (idx[0 .. m)), adds a stretch of them
// from the first, sets their result codes, calls took(i, row) for every packet i that a row took,
// and returns how many entries they were.  The packets taken are framed into their rows by one
// launch.
template <class F>
int add_packets(Batch* b, uint32_t n, const uint32_t* stream, const uint32_t* len, const uint32_t* offset, const void* dev_payloads,
                uint64_t pitch, F&& stretch) {
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, n, stream)) return e;
    const uint32_t maxb = b->prm.max_packet_bytes;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (len[i] > maxb) continue;
        if (len[i] > largest) largest = len[i];
        if (len[i] && (uint64_t)(offset ? offset[i] : 0u) + len[i] > pitch) return -3;
    }
    if (!b->core.desc.ensure((size_t)n * sizeof(FrameDesc))) return b->staging_failed(), -4;
    FrameDesc* d = (FrameDesc*)b->core.desc.host;
    size_t nd = 0;
    b->sort_by_stream(n, stream);
    for (uint32_t s = 0; s < b->prm.n_streams; ++s) {
        const uint32_t* idx = b->order.data() + b->start[s];
        const uint32_t m = b->start[s + 1] - b->start[s];
        if (!m) continue;
        Batch::Stream& x = b->use(s);
        const RowTable& pool = x.ctx->rows;
        const auto took = [&](uint32_t i, RowId r) {
            d[nd++] = FrameDesc{(uint64_t)(uintptr_t)dev_payloads + (uint64_t)i * pitch + (offset ? offset[i] : 0u), pool.offset(r),
                                len[i], pool.cap_bytes(r), 0};
        };
        for (uint32_t a = 0; a < m;) a += stretch(s, x, idx + a, m - a, took);
    }
    b->frame(nd, largest + 3);
    return b->sync() ? 0 : -4;
}

}  // namespace

extern "C" {

void* tamd_batch_create(const tamd_batch_params* p, char* err, size_t err_len) {
    if (!p || p->n_streams == 0 || p->max_packet_bytes == 0 || p->max_packet_bytes > 65535 || p->arena_bytes == 0)
        return fail(err, err_len, "bad parameters");
    const uint64_t range = (p->arena_bytes / p->n_streams) & ~(uint64_t)(TAMD_ROW_UNIT - 1);
    if (range < 64u * (p->max_packet_bytes + 64u)) return fail(err, err_len, "bad parameters: arena too small for the streams");
    if (!gf_init()) return fail(err, err_len, "gf self test failed");
    std::unique_ptr<Batch> b(new Batch());
    b->prm = *p;
    b->dev.set_small_uploads(p->n_streams <= 4);
    b->dev.set_program_slots(2, 4u << 20);
    if (!b->dev.init((int)p->device, p->arena_bytes)) return fail(err, err_len, b->dev.error());
    b->core.device = b->dev.device();
    b->core.stream = (hipStream_t)b->dev.stream();
    if (!b->dev.gf_selftest()) return fail(err, err_len, "device GF(256) self test failed");
    const uint32_t row_cap = (p->max_packet_bytes + TAMD_BATCH_RECOVERY_OVERHEAD + 63u) / 64u * 64u;
    b->st.resize(p->n_streams);
    for (uint32_t i = 0; i < p->n_streams; ++i) {
        Batch::Stream& s = b->st[i];
        s.ctx.reset(new Context());
        s.ctx->rows.init(range, (range / TAMD_ROW_UNIT) * i);
        // (the session's choices for flat programs, session.cpp tamd_session_create)
        s.ctx->backsub_rows = p->n_streams <= 4 ? 2u : ~0u;
        s.ctx->dense_split = p->n_streams <= 4 ? 0u : Encoder::kDenseSplit;
        s.ctx->short_scans = p->n_streams <= 4;
        s.enc.reset(new Encoder(s.ctx.get(), row_cap));
        s.dec.reset(new Decoder(s.ctx.get(), row_cap));
    }
    return b.release();
}

void tamd_batch_destroy(void* h) {
    Batch* b = (Batch*)h;
    if (!b) return;
    {
        std::lock_guard<std::mutex> lk(b->core.mu);
        b->dev.bind_thread();
        b->dev.synchronize();
    }
    delete b;
}

const char* tamd_batch_error(void* h) { return error_text<Batch>(h); }

int tamd_batch_encoder_add(void* h, uint32_t n, const uint32_t* stream, const uint32_t* len, const void* dev_payloads,
                           uint64_t pitch, uint32_t* packet_num, int32_t* rc) {
    return tamd_batch_encoder_add_at(h, n, stream, len, nullptr, dev_payloads, pitch, packet_num, rc);
}

// Packet i at dev_payloads + i * pitch + offset[i] (a null offset: 0).
int tamd_batch_encoder_add_at(void* h, uint32_t n, const uint32_t* stream, const uint32_t* len, const uint32_t* offset,
                              const void* dev_payloads, uint64_t pitch, uint32_t* packet_num, int32_t* rc) {
    Batch* b = (Batch*)h;
    if (!b || !stream || !len || !dev_payloads || !packet_num || !rc) return -1;
    return add_packets(b, n, stream, len, offset, dev_payloads, pitch,
                       [&](uint32_t, Batch::Stream& x, const uint32_t* idx, uint32_t m, const auto& took) {
        const uint32_t l = len[idx[0]];
        packet_num[idx[0]] = 0;
        if (l == 0 || l > b->prm.max_packet_bytes) return rc[idx[0]] = kInvalidInput, 1u;
        uint32_t k = 1;  // the stretch of equally long packets from here
        while (k < m && len[idx[k]] == l) ++k;
        const uint32_t hb = length_header_bytes(l), framed = hb + l;
        if (!b->stretch_rows(*x.enc, *x.ctx, k, framed)) {
            for (uint32_t j = 0; j < k; ++j) { rc[idx[j]] = kDisabled; packet_num[idx[j]] = 0; }
            return k;
        }
        uint32_t col0 = 0;
        const bool run = k >= 2 && x.enc->add_run(b->rows.data(), k, framed, hb, l, false, &col0);
        for (uint32_t j = 0; j < k; ++j) {
            const RowId r = b->rows[j];
            uint32_t pn = col_add(col0, j);
            const Result res = run ? kSuccess : x.enc->add(r, framed, hb, l, nullptr, &pn, false);
            rc[idx[j]] = res;
            packet_num[idx[j]] = res == kSuccess ? pn : 0;
            if (res == kSuccess) took(idx[j], r);
            else x.ctx->rows.free_deferred(r);
        }
        return k;
    });
}

int tamd_batch_encode(void* h, uint32_t n, const uint32_t* stream, void* dev_out, uint64_t pitch, uint32_t* bytes,
                      int32_t* rc) {
    Batch* b = (Batch*)h;
    if (!b || !stream || !dev_out || !bytes || !rc) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, n, stream)) return e;
    if (pitch < b->max_recovery()) return -3;
    if (!b->core.desc.ensure((size_t)n * sizeof(UnframeDesc))) return b->staging_failed(), -4;
    UnframeDesc* d = (UnframeDesc*)b->core.desc.host;
    size_t nd = 0;
    std::vector<std::pair<uint32_t, RowId>> made;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = stream[i];
        Batch::Stream& x = b->use(s);
        RecoveryOut o;
        const Result res = x.enc->encode(o);
        b->touch(s);
        rc[i] = res;
        bytes[i] = res == kSuccess ? o.total() : 0;
        if (res != kSuccess) continue;
        made.push_back(std::make_pair(s, o.row));
        if (o.total() > largest) largest = o.total();
        d[nd++] = UnframeDesc{(uint64_t)(uintptr_t)dev_out + (uint64_t)i * pitch, x.ctx->rows.offset(o.row), o.total(), 1, 0};
    }
    b->flush();
    const bool done = b->unframe(nd, pitch, largest, true);
    // (released once the stream's next program has completed)
    for (const auto& m : made) b->st[m.first].ctx->rows.free_deferred(m.second);
    return done ? 0 : -4;
}

int tamd_batch_encoder_ack(void* h, uint32_t stream, const uint8_t* data, uint32_t bytes, uint32_t* next_expected) {
    Batch* b = (Batch*)h;
    if (!b || !data || !next_expected) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, 1, &stream)) return e;
    if (bytes < 1) return kInvalidInput;
    Batch::Stream& x = b->use(stream);
    uint32_t next = 0;
    const Result res = x.enc->acknowledge(data, bytes, &next);
    b->touch(stream);
    if (res == kSuccess) *next_expected = next;
    return res;
}

int tamd_batch_decoder_add_original(void* h, uint32_t n, const uint32_t* stream, const uint32_t* packet_num,
                                    const uint32_t* len, const void* dev_payloads, uint64_t pitch, int32_t* rc) {
    return tamd_batch_decoder_add_original_at(h, n, stream, packet_num, len, nullptr, dev_payloads, pitch, rc);
}

int tamd_batch_decoder_add_original_at(void* h, uint32_t n, const uint32_t* stream, const uint32_t* packet_num,
                                       const uint32_t* len, const uint32_t* offset, const void* dev_payloads, uint64_t pitch,
                                       int32_t* rc) {
    Batch* b = (Batch*)h;
    if (!b || !stream || !packet_num || !len || !dev_payloads || !rc) return -1;
    return add_packets(b, n, stream, len, offset, dev_payloads, pitch,
                       [&](uint32_t s, Batch::Stream& x, const uint32_t* idx, uint32_t m, const auto& took) {
        const uint32_t l = len[idx[0]], pn0 = packet_num[idx[0]];
        b->touch(s);  // (an original that completes a region may recover packets: ops pending)
        if (l == 0 || l > b->prm.max_packet_bytes || pn0 >= kColumnPeriod) return rc[idx[0]] = kInvalidInput, 1u;
        uint32_t k = 1;  // the stretch of equally long packets with consecutive numbers from here
        while (k < m && len[idx[k]] == l && packet_num[idx[k]] == pn0 + k && pn0 + k < kColumnPeriod) ++k;
        const uint32_t hb = length_header_bytes(l), framed = hb + l;
        if (!b->stretch_rows(*x.dec, *x.ctx, k, framed)) {
            for (uint32_t j = 0; j < k; ++j) rc[idx[j]] = kDisabled;
            return k;
        }
        const bool run = k >= 2 && x.dec->add_run_inorder(pn0, b->rows.data(), k, framed, hb, l, false);
        for (uint32_t j = 0; j < k; ++j) {
            const RowId r = b->rows[j];
            bool kept = run;
            rc[idx[j]] = run ? kSuccess : x.dec->add_original(pn0 + j, r, framed, hb, l, nullptr, &kept, false);
            if (kept) took(idx[j], r);
            else x.ctx->rows.free_deferred(r);
        }
        return k;
    });
}

int tamd_batch_decoder_add_recovery(void* h, uint32_t n, const uint32_t* stream, const uint32_t* bytes,
                                    const void* dev_packets, uint64_t pitch, int32_t* rc) {
    Batch* b = (Batch*)h;
    if (!b || !stream || !bytes || !dev_packets || !rc) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, n, stream)) return e;
    const uint32_t maxb = b->max_recovery(), largest = largest_within(bytes, n, maxb);
    if (pitch < largest) return -3;
    if (!n) return 0;
    // the packets' last bytes (their footers): one gather, one copy
    HandleCore& c = b->core;
    const size_t desc_bytes = (size_t)n * (sizeof(FrameDesc) > sizeof(TailDesc) ? sizeof(FrameDesc) : sizeof(TailDesc));
    if (!c.room(desc_bytes, (size_t)n * 8)) return -4;
    TailDesc* t = (TailDesc*)c.desc.host;
    for (uint32_t i = 0; i < n; ++i) {
        const bool valid = bytes[i] >= 1 && bytes[i] <= maxb;
        t[i] = TailDesc{(uint64_t)(uintptr_t)dev_packets + (uint64_t)i * pitch, valid ? bytes[i] : 0u, 0};
    }
    c.hip(hipMemcpyAsync(c.desc.dev, c.desc.host, (size_t)n * sizeof(TailDesc), hipMemcpyHostToDevice, c.stream), "descriptor copy");
    if (b->ok())
        c.launch_timed(kTails, [&] {
            hipLaunchKernelGGL(tamd_gather_tails, dim3((n + 255) / 256), dim3(256), 0, c.stream, (const TailDesc*)c.desc.dev, n, c.out.dev);
        });
    c.hip(hipMemcpyAsync(c.out.host, c.out.dev, (size_t)n * 8, hipMemcpyDeviceToHost, c.stream), "tail copy");
    if (!b->sync()) return -4;
    const uint8_t* tails = c.out.host;
    FrameDesc* d = (FrameDesc*)c.desc.host;  // (the tail records are done with)
    size_t nd = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = stream[i], total = bytes[i];
        if (total < 1 || total > maxb) { rc[i] = kInvalidInput; continue; }
        Batch::Stream& x = b->use(s);
        Context& cx = *x.ctx;
        if (x.dec->disabled()) { rc[i] = kDisabled; continue; }
        const RowId r = cx.alloc(total);
        if (r == kNoRow) { x.dec->set_disabled(); rc[i] = kDisabled; continue; }
        bool took = false;
        b->touch(s);
        rc[i] = x.dec->add_recovery(r, total, tails + (size_t)i * 8, nullptr, &took);
        if (!took) { cx.rows.free_deferred(r); continue; }
        d[nd++] = FrameDesc{(uint64_t)(uintptr_t)dev_packets + (uint64_t)i * pitch, cx.rows.offset(r), total, cx.rows.cap_bytes(r), 1};
    }
    b->frame(nd, largest);
    return b->sync() ? 0 : -4;
}

int tamd_batch_decode(void* h, uint32_t n, const uint32_t* stream, void* dev_out, uint64_t pitch, uint32_t cap,
                      uint32_t* out_stream, uint32_t* out_packet_num, uint32_t* out_bytes, uint32_t* n_out,
                      int32_t* stream_rc) {
    Batch* b = (Batch*)h;
    if (!b || !stream || !dev_out || !out_stream || !out_packet_num || !out_bytes || !n_out || !stream_rc) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, n, stream)) return e;
    if (pitch < b->prm.max_packet_bytes) return -3;
    *n_out = 0;
    // what each listed stream recovered: (list entry, packet number, row, upper bound) in output order
    struct Got { uint32_t k, num, row_units, upper; };
    std::vector<Got> got;
    std::vector<RecoveredPacket*> rp;
    for (uint32_t k = 0; k < n; ++k) {
        Batch::Stream& x = b->use(stream[k]);
        stream_rc[k] = kNeedMoreData;
        if (x.dec->is_ready() != kSuccess) continue;
        if (x.dec->ready_count() > cap - got.size()) continue;  // (decoded by a later call)
        rp.clear();
        const Result res = x.dec->decode(rp);
        b->touch(stream[k]);
        stream_rc[k] = res;
        if (res != kSuccess) continue;
        for (const RecoveredPacket* p : rp) got.push_back(Got{k, p->packet_num, x.ctx->rows.offset(p->row), p->framed_upper});
    }
    b->flush();
    // Two launches: the first reads every row's length header (one copy brings the lengths and
    // statuses to the host), the second writes the payloads.  In between, a stream with a row
    // whose header is malformed, announces 0 bytes or more than the row or a slot holds is
    // disabled and its packets leave the list (capi.cpp read_back's rule): none of its bytes are
    // written, and the other streams' packets land at their final slots.
    for (int pass = 0; pass < 2 && !got.empty(); ++pass) {
        if (!b->core.desc.ensure(got.size() * sizeof(UnframeDesc))) return b->staging_failed(), -4;
        UnframeDesc* d = (UnframeDesc*)b->core.desc.host;
        uint32_t largest = 0;
        for (size_t j = 0; j < got.size(); ++j) {
            d[j] = UnframeDesc{(uint64_t)(uintptr_t)dev_out + (uint64_t)j * pitch, got[j].row_units, got[j].upper, 0, 0};
            if (got[j].upper > largest) largest = got[j].upper;
        }
        if (!b->unframe(got.size(), pitch, largest, pass == 1)) return -4;
        const UnframeOut* o = (const UnframeOut*)b->core.out.host;
        if (pass == 1) {  // (the rows the first launch accepted, unchanged since)
            for (size_t j = 0; j < got.size(); ++j)
                if (o[j].status != TAMD_FRAME_OK || o[j].len != out_bytes[j]) return b->core.hip(hipErrorUnknown, "recovered row changed"), -4;
            break;
        }
        for (size_t j = 0; j < got.size(); ++j)
            if (o[j].status != TAMD_FRAME_OK) {
                b->st[stream[got[j].k]].dec->set_disabled();
                stream_rc[got[j].k] = kDisabled;
            }
        size_t keep = 0;
        for (size_t j = 0; j < got.size(); ++j) {
            if (stream_rc[got[j].k] != kSuccess) continue;
            out_stream[keep] = stream[got[j].k];
            out_packet_num[keep] = got[j].num;
            out_bytes[keep] = o[j].len;
            got[keep++] = got[j];
        }
        got.resize(keep);
    }
    for (size_t j = 0; j < got.size(); ++j) {
        const uint32_t hb = length_header_bytes(out_bytes[j]);
        b->st[stream[got[j].k]].dec->set_recovered_length(got[j].num, hb + out_bytes[j], hb, nullptr);
    }
    *n_out = (uint32_t)got.size();
    return b->sync() ? 0 : -4;
}

int tamd_batch_decoder_ack(void* h, uint32_t stream, uint8_t* buffer, uint32_t limit, uint32_t* used) {
    Batch* b = (Batch*)h;
    if (!b || !buffer || !used) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(b, lk, 1, &stream)) return e;
    if (limit < 16) return kInvalidInput;  // SIAMESE_ACK_MIN_BYTES
    uint32_t u = 0;
    const Result res = b->use(stream).dec->ack(buffer, limit, &u);
    *used = u;
    return res;
}

void tamd_batch_set_timing(void* h, int on) {
    Batch* b = (Batch*)h;
    if (!b) return;
    std::lock_guard<std::mutex> lk(b->core.mu);
    b->dev.bind_thread();
    b->core.timer.on = on != 0;
    b->dev.set_timing(on != 0);
}

void tamd_batch_kernel_ms(void* h, double* out, unsigned n) {
    Batch* b = (Batch*)h;
    if (!b || !out) return;
    std::lock_guard<std::mutex> lk(b->core.mu);
    b->dev.bind_thread();
    b->dev.collect_timing();
    DeviceStats& ds = b->dev.stats();
    LaunchTimer& t = b->core.timer;
    const double v[10] = {t.ms[kFrame], t.ms[kUnframe], t.ms[kTails], ds.kernel_ms - b->prog_ms0,
                          (double)t.launches[kFrame], (double)t.launches[kUnframe], (double)t.launches[kTails],
                          (double)(ds.timed_launches - b->prog_n0), (double)b->moved[0], (double)b->moved[1]};
    for (unsigned i = 0; i < n && i < 10; ++i) out[i] = v[i];
    t.reset();
    b->moved[0] = b->moved[1] = 0;
    b->prog_ms0 = ds.kernel_ms;
    b->prog_n0 = ds.timed_launches;
}

}  // extern "C"
