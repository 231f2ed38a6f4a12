// recv.cpp -- include/tonk_receive.h: the front of the receive path for a call's datagrams in the
// caller's device memory.  A handle is the shared core (handle.h: lock, stream, pinned descriptor
// and result staging) and one device allocation: the expanded keys of its streams (the sealer's
// table and set_key: a pinned host copy, the changed range goes up ahead of the next call's
// descriptors) and their anti-replay states (recv.h: 67 words each), guard bytes in front of,
// between and behind the two.  A call is one descriptor copy, the five launches of recv.hip back to
// back on the handle's stream, one result copy and one wait.  The only per-item host work besides
// the refusal checks is grouping the item indices by stream (a CSR list in the pinned staging).
#include "../../include/tonk_receive.h"

#include "handle.h"
#include "kernel_abi.h"
#include "recv.h"

#include <memory>

using namespace tamd;

static_assert(sizeof(tamd_recv_result) == sizeof(RecvResult), "the kernels write the interface's record");

namespace {

enum { kPredict = 0, kTag = 1, kResolve = 2, kDecipher = 3, kKinds = 4 };

const uint32_t kGuard = 64;  // bytes of a guard block (recv.hip TAMD_RECV_GUARD), checked after every call
const uint8_t kGuardByte = 0xC7;
const size_t kStateBytes = TAMD_RECV_STATE_WORDS * sizeof(uint64_t);

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

struct Receiver {
    HandleCore core;
    tamd_recv_params prm;
    uint8_t* mem = nullptr;  // kGuard | n_streams keys | kGuard | n_streams states | kGuard
    tamd_seal_key* keys_host = nullptr;  // pinned
    uint32_t dirty_lo = ~0u, dirty_hi = 0;  // streams [lo, hi) whose key changed since the last upload
    std::vector<uint64_t> largest;  // the host mirror of LargestSequence, kept from the results
    std::vector<uint32_t> count, listed;  // a call's items per stream, the streams in order of appearance
    uint64_t repaired = 0;  // datagrams whose tag was computed again in the resolve step

    size_t key_bytes() const { return (size_t)prm.n_streams * sizeof(tamd_seal_key); }
    uint8_t* keys_dev() const { return mem + kGuard; }
    uint8_t* states_dev() const { return mem + 2 * kGuard + key_bytes(); }
    uint8_t* guard(int k) const { return k == 0 ? mem : k == 1 ? mem + kGuard + key_bytes() : states_dev() + (size_t)prm.n_streams * kStateBytes; }

    void upload_keys() {
        if (dirty_lo >= dirty_hi) return;
        core.hip(hipMemcpyAsync(keys_dev() + (size_t)dirty_lo * sizeof(tamd_seal_key), keys_host + dirty_lo,
                                (size_t)(dirty_hi - dirty_lo) * sizeof(tamd_seal_key), hipMemcpyHostToDevice, core.stream), "key copy");
        dirty_lo = ~0u;
        dirty_hi = 0;
    }

    ~Receiver() {  // (the core, destroyed after this, waits again and frees the rest)
        if (core.device < 0) return;
        hipSetDevice(core.device);
        if (core.stream) hipStreamSynchronize(core.stream);
        if (keys_host) hipHostFree(keys_host);
        if (mem) hipFree(mem);
    }
};

// Entry checks of a call that names streams; returns 0 with the handle locked and its device current.
int enter(Receiver* s, std::unique_lock<std::mutex>& lk, uint32_t n, const uint32_t* stream) {
    if (const int e = tamd::enter(s, lk)) return e;
    for (uint32_t i = 0; i < n; ++i)
        if (stream[i] >= s->prm.n_streams) return -2;
    return 0;
}

}  // namespace

extern "C" {

void* tamd_recv_create(const tamd_recv_params* p, char* err, size_t err_len) {
    if (!p || p->n_streams == 0 || p->max_datagram_bytes == 0 || p->max_datagram_bytes > 65535) return fail(err, err_len, "bad parameters");
    std::string why = device_check(p->device, "datagrams are received");
    if (!why.empty()) return fail(err, err_len, why);
    std::unique_ptr<Receiver> s(new Receiver());
    s->prm = *p;
    why = s->core.open(p->device);
    if (!why.empty()) return fail(err, err_len, why);
    HandleCore& c = s->core;
    const size_t kb = s->key_bytes(), total = 3 * (size_t)kGuard + kb + (size_t)p->n_streams * kStateBytes;
    if (hipHostMalloc((void**)&s->keys_host, kb, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s->mem, total) != hipSuccess)
        return fail(err, err_len, "tonk_amd: the key and state tables could not be allocated");
    memset(s->keys_host, 0, kb);  // (a fresh stream's key is 0; all of its expansion is 0 too)
    // zeros (key 0, Reset(0)) between guard bytes
    bool ok = c.hip(hipMemsetAsync(s->mem, 0, total, c.stream), "hipMemsetAsync");
    for (int k = 0; k < 3; ++k) ok = ok && c.hip(hipMemsetAsync(s->guard(k), kGuardByte, kGuard, c.stream), "hipMemsetAsync");
    if (!ok || !c.hip(hipStreamSynchronize(c.stream), "hipStreamSynchronize")) return fail(err, err_len, c.error);
    s->largest.assign(p->n_streams, 0);
    s->count.assign(p->n_streams, 0);
    return s.release();
}

void tamd_recv_destroy(void* h) { destroy<Receiver>(h); }
const char* tamd_recv_error(void* h) { return error_text<Receiver>(h); }
void tamd_recv_set_timing(void* h, int on) { set_timing<Receiver>(h, on); }

void tamd_recv_kernel_ms(void* h, double* out, unsigned n) {
    if (!h || !out) return;
    kernel_ms<Receiver>(h, out, n, kKinds);
    Receiver* s = (Receiver*)h;
    std::lock_guard<std::mutex> lk(s->core.mu);
    if (n > 2 * kKinds) out[2 * kKinds] = (double)s->repaired;
    s->repaired = 0;
}

int tamd_recv_set_key(void* h, uint32_t stream, uint64_t key) {
    Receiver* s = (Receiver*)h;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, 1, &stream)) return e;
    s->keys_host[stream] = tamd_seal_expand(key);
    if (stream < s->dirty_lo) s->dirty_lo = stream;
    if (stream + 1 > s->dirty_hi) s->dirty_hi = stream + 1;
    return 0;
}

int tamd_recv_reset(void* h, uint32_t stream, uint64_t base) {
    Receiver* s = (Receiver*)h;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, 1, &stream)) return e;
    HandleCore& c = s->core;
    if (!c.room(kStateBytes, 0)) return -4;
    tamd_recv_reset_state((uint64_t*)c.desc.host, base);
    c.hip(hipMemcpyAsync(s->states_dev() + (size_t)stream * kStateBytes, c.desc.host, kStateBytes, hipMemcpyHostToDevice, c.stream), "state copy");
    if (!c.hip(hipStreamSynchronize(c.stream), "hipStreamSynchronize")) return -4;
    s->largest[stream] = base;
    return 0;
}

int tamd_recv_next_expected(void* h, uint32_t n, const uint32_t* stream, uint64_t* out) {
    Receiver* s = (Receiver*)h;
    if (!s || (n && (!stream || !out))) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream)) return e;
    for (uint32_t i = 0; i < n; ++i) out[i] = s->largest[stream[i]] + 1u;
    return 0;
}

int tamd_recv_state(void* h, uint32_t stream, uint64_t* out) {
    Receiver* s = (Receiver*)h;
    if (!s || !out) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, 1, &stream)) return e;
    HandleCore& c = s->core;
    if (!c.room(0, kStateBytes)) return -4;
    c.hip(hipMemcpyAsync(c.out.host, s->states_dev() + (size_t)stream * kStateBytes, kStateBytes, hipMemcpyDeviceToHost, c.stream), "state copy");
    if (!c.hip(hipStreamSynchronize(c.stream), "hipStreamSynchronize")) return -4;
    memcpy(out, c.out.host, kStateBytes);
    return 0;
}

int tamd_recv_receive(void* h, uint32_t n, const uint32_t* stream, const uint32_t* bytes, void* dev, uint64_t pitch, int32_t* rc,
                      tamd_recv_result* result) {
    Receiver* s = (Receiver*)h;
    if (!s || (n && (!stream || !bytes || !dev || !rc || !result))) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream)) return e;
    HandleCore& c = s->core;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    if (pitch < largest_within(bytes, n, maxb)) return -3;
    if (!n) return 0;

    // the streams of the call in the order they first appear, their item counts
    s->listed.clear();
    for (uint32_t i = 0; i < n; ++i)
        if (s->count[stream[i]]++ == 0) s->listed.push_back(stream[i]);
    const uint32_t nl = (uint32_t)s->listed.size();
    // up:   RecvDesc[n] | listed[nl] | start[nl + 1] | idx[n]
    // down: rc[n] | RecvResult[n] | the three guard blocks; behind them, on the device only, what
    //       the steps hand on: RecvFields[n] | pred[n] | tag_ok[n] | clen[n]
    const size_t u_listed = (size_t)n * sizeof(RecvDesc), u_start = u_listed + (size_t)nl * 4, u_idx = u_start + ((size_t)nl + 1) * 4;
    const size_t up = u_idx + (size_t)n * 4;
    const size_t o_res = align16((size_t)n * 4), o_guard = o_res + (size_t)n * sizeof(RecvResult), down = o_guard + 3 * kGuard;
    const size_t o_f = align16(down), o_pred = o_f + (size_t)n * sizeof(RecvFields), o_tag = o_pred + (size_t)n * 8;
    const size_t o_clen = o_tag + (size_t)n * 4, total = o_clen + (size_t)n * 4;
    if (!c.room(up, total)) {
        for (uint32_t st : s->listed) s->count[st] = 0;
        return -4;
    }
    RecvDesc* d = (RecvDesc*)c.desc.host;
    uint32_t* listed = (uint32_t*)(c.desc.host + u_listed);
    uint32_t* start = (uint32_t*)(c.desc.host + u_start);
    uint32_t* idx = (uint32_t*)(c.desc.host + u_idx);
    uint32_t acc = 0;
    for (uint32_t j = 0; j < nl; ++j) {
        const uint32_t st = s->listed[j];
        listed[j] = st;
        start[j] = acc;
        acc += s->count[st];
        s->count[st] = start[j];  // (from here on: where the stream's next item goes)
    }
    start[nl] = acc;
    for (uint32_t i = 0; i < n; ++i) {
        d[i] = RecvDesc{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch, stream[i], bytes[i]};
        idx[s->count[stream[i]]++] = i;
    }
    for (uint32_t st : s->listed) s->count[st] = 0;

    RecvCall a;
    memset(&a, 0, sizeof(a));
    a.d = (const RecvDesc*)c.desc.dev;
    a.listed = (const uint32_t*)(c.desc.dev + u_listed);
    a.start = (const uint32_t*)(c.desc.dev + u_start);
    a.idx = (const uint32_t*)(c.desc.dev + u_idx);
    a.rc = (uint32_t*)c.out.dev;
    a.res = (RecvResult*)(c.out.dev + o_res);
    a.guards_out = c.out.dev + o_guard;
    a.f = (RecvFields*)(c.out.dev + o_f);
    a.pred = (uint64_t*)(c.out.dev + o_pred);
    a.tag_ok = (uint32_t*)(c.out.dev + o_tag);
    a.clen = (uint32_t*)(c.out.dev + o_clen);
    a.state = (uint64_t*)s->states_dev();
    a.keys = (const uint32_t*)s->keys_dev();
    for (int k = 0; k < 3; ++k) a.guard[k] = s->guard(k);
    a.n = n;
    a.n_listed = nl;
    a.max_bytes = maxb;

    s->upload_keys();
    const dim3 per_item((n + 255u) / 256u), per_stream((nl + 63u) / 64u), per_group((n + 63u) / 64u);
    const bool ok = c.run_all(up, down, [&] {
        c.launch_timed(kPredict, [&] { hipLaunchKernelGGL(tamd_rx_parse, per_item, dim3(256), 0, c.stream, a); });
        c.launch_timed(kPredict, [&] { hipLaunchKernelGGL(tamd_rx_predict, per_stream, dim3(64), 0, c.stream, a); });
        c.launch_timed(kTag, [&] { hipLaunchKernelGGL(tamd_rx_tag, per_group, dim3(512), 0, c.stream, a); });
        c.launch_timed(kResolve, [&] { hipLaunchKernelGGL(tamd_rx_resolve, per_stream, dim3(64), 0, c.stream, a); });
        c.launch_timed(kDecipher, [&] { hipLaunchKernelGGL(tamd_rx_decipher, per_group, dim3(512), 0, c.stream, a); });
    });
    if (!ok) return -4;
    for (uint32_t k = 0; k < 3 * kGuard; ++k)
        if (c.out.host[o_guard + k] != kGuardByte) {
            c.error = "tonk_amd: a write left the handle's key and state tables";
            c.failed = true;
            return -4;
        }
    const uint32_t* o = (const uint32_t*)c.out.host;
    const tamd_recv_result* r = (const tamd_recv_result*)(c.out.host + o_res);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t code = o[i] & 0xffu;
        rc[i] = (int32_t)code;
        if (o[i] & TAMD_RECV_REPAIRED) ++s->repaired;
        if (code == TAMD_RECV_INVALID) {
            memset(&result[i], 0, sizeof(result[i]));
            continue;
        }
        result[i] = r[i];
        uint64_t& top = s->largest[stream[i]];
        if ((code == TAMD_RECV_OK || code == TAMD_RECV_REORDERED) && tamd_recv_less(top, r[i].nonce)) top = r[i].nonce;
    }
    return 0;
}

}  // extern "C"
