// seal.cpp -- include/tonk_seal.h: batched seal and open of datagrams in the caller's device
// memory.  A handle is the shared core (handle.h: lock, stream, pinned descriptor and result
// staging) and the expanded keys of its streams in a device table (a pinned host copy beside it:
// set_key writes there, and the changed range goes up ahead of the next call's descriptors).
// Every call is one descriptor copy, one launch of a kernel of seal.hip, one result copy and one
// wait.
#include "../../include/tonk_seal.h"

#include "handle.h"
#include "kernel_abi.h"
#include "seal.h"

#include <memory>

using namespace tamd;

namespace {

enum { kPackets = 0, kFooters = 1, kKinds = 2 };

struct Sealer {
    HandleCore core;
    tamd_seal_params prm;
    tamd_seal_key* keys_host = nullptr;  // pinned
    uint32_t* keys_dev = nullptr;
    uint32_t dirty_lo = ~0u, dirty_hi = 0;  // streams [lo, hi) changed since the last upload

    // The changed keys go up on the stream ahead of the call's descriptors.
    void upload_keys() {
        if (dirty_lo >= dirty_hi) return;
        core.hip(hipMemcpyAsync(keys_dev + 4 * (size_t)dirty_lo, keys_host + dirty_lo, (size_t)(dirty_hi - dirty_lo) * sizeof(tamd_seal_key),
                                hipMemcpyHostToDevice, core.stream), "key copy");
        dirty_lo = ~0u;
        dirty_hi = 0;
    }

    ~Sealer() {  // (the core, destroyed after this, waits again and frees the rest)
        if (core.device < 0) return;
        hipSetDevice(core.device);
        if (core.stream) hipStreamSynchronize(core.stream);
        if (keys_host) hipHostFree(keys_host);
        if (keys_dev) hipFree(keys_dev);
    }
};

// Entry checks of a call that names streams; returns 0 with the handle locked and its device current.
int enter(Sealer* s, std::unique_lock<std::mutex>& lk, uint32_t n, const uint32_t* stream) {
    if (const int e = tamd::enter(s, lk)) return e;
    for (uint32_t i = 0; i < n; ++i)
        if (stream[i] >= s->prm.n_streams) return -2;
    return 0;
}

// seal, open, cipher and tag: one launch of tamd_seal_packets in `mode`.  message_bytes is null
// for the primitives; the results go to rc or tag, whichever is given.
int packets(Sealer* s, uint32_t mode, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
            const uint32_t* message_bytes, const void* dev, uint64_t pitch, int32_t* rc, uint16_t* tag) {
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream)) return e;
    HandleCore& c = s->core;
    const bool datagram = mode & TAMD_SEAL_M_DATAGRAM;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    if (pitch < largest_within(bytes, n, maxb)) return -3;
    if (!n) return 0;
    if (!c.room(n * sizeof(SealDesc), n * sizeof(uint32_t))) return -4;
    SealDesc* d = (SealDesc*)c.desc.host;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t msg = message_bytes ? message_bytes[i] : 0u;
        const bool valid = datagram ? tamd_seal_valid(bytes[i], msg, maxb) : bytes[i] <= maxb;
        d[i] = SealDesc{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch, nonce[i], stream[i], bytes[i], msg, valid ? 0u : 1u};
    }
    s->upload_keys();
    const bool ok = c.run(kPackets, n * sizeof(SealDesc), n * sizeof(uint32_t), [&] {
        hipLaunchKernelGGL(tamd_seal_packets, dim3((n + 63u) / 64u), dim3(512), 0, c.stream, (const SealDesc*)c.desc.dev, n,
                           (const uint32_t*)s->keys_dev, mode, (uint32_t*)c.out.dev);
    });
    if (!ok) return -4;
    const uint32_t* o = (const uint32_t*)c.out.host;
    for (uint32_t i = 0; rc && i < n; ++i) rc[i] = (int32_t)o[i];
    for (uint32_t i = 0; tag && i < n; ++i)  // (an entry longer than the handle allows is skipped: tag 0)
        tag[i] = bytes[i] <= maxb ? (uint16_t)o[i] : (uint16_t)0;
    return 0;
}

}  // namespace

extern "C" {

void* tamd_seal_create(const tamd_seal_params* p, char* err, size_t err_len) {
    if (!p || p->n_streams == 0 || p->max_datagram_bytes == 0 || p->max_datagram_bytes > 65535) return fail(err, err_len, "bad parameters");
    std::string why = device_check(p->device, "datagrams are sealed");
    if (!why.empty()) return fail(err, err_len, why);
    std::unique_ptr<Sealer> s(new Sealer());
    s->prm = *p;
    why = s->core.open(p->device);
    if (!why.empty()) return fail(err, err_len, why);
    const size_t kb = (size_t)p->n_streams * sizeof(tamd_seal_key);
    if (hipHostMalloc((void**)&s->keys_host, kb, hipHostMallocDefault) != hipSuccess || hipMalloc((void**)&s->keys_dev, kb) != hipSuccess ||
        hipMemset(s->keys_dev, 0, kb) != hipSuccess)
        return fail(err, err_len, "tonk_amd: the key table could not be allocated");
    memset(s->keys_host, 0, kb);  // (a fresh stream's key is 0; all of its expansion is 0 too)
    return s.release();
}

void tamd_seal_destroy(void* h) { destroy<Sealer>(h); }
const char* tamd_seal_error(void* h) { return error_text<Sealer>(h); }
void tamd_seal_set_timing(void* h, int on) { set_timing<Sealer>(h, on); }
void tamd_seal_kernel_ms(void* h, double* out, unsigned n) { kernel_ms<Sealer>(h, out, n, kKinds); }

int tamd_seal_set_key(void* h, uint32_t stream, uint64_t key) {
    Sealer* s = (Sealer*)h;
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, 1, &stream)) return e;
    s->keys_host[stream] = tamd_seal_expand(key);
    if (stream < s->dirty_lo) s->dirty_lo = stream;
    if (stream + 1 > s->dirty_hi) s->dirty_hi = stream + 1;
    return 0;
}

int tamd_seal_seal(void* h, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                   const uint32_t* message_bytes, void* dev, uint64_t pitch, int32_t* rc) {
    Sealer* s = (Sealer*)h;
    if (!s || !stream || !nonce || !bytes || !message_bytes || !dev || !rc) return -1;
    return packets(s, TAMD_SEAL_M_CIPHER | TAMD_SEAL_M_TAG | TAMD_SEAL_M_DATAGRAM, n, stream, nonce, bytes, message_bytes, dev, pitch,
                   rc, nullptr);
}

int tamd_seal_open(void* h, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
                   const uint32_t* message_bytes, void* dev, uint64_t pitch, int32_t* rc) {
    Sealer* s = (Sealer*)h;
    if (!s || !stream || !nonce || !bytes || !message_bytes || !dev || !rc) return -1;
    return packets(s, TAMD_SEAL_M_CIPHER | TAMD_SEAL_M_TAG | TAMD_SEAL_M_DATAGRAM | TAMD_SEAL_M_CHECK, n, stream, nonce, bytes,
                   message_bytes, dev, pitch, rc, nullptr);
}

int tamd_seal_cipher(void* h, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes, void* dev,
                     uint64_t pitch) {
    Sealer* s = (Sealer*)h;
    if (!s || !stream || !nonce || !bytes || !dev) return -1;
    return packets(s, TAMD_SEAL_M_CIPHER, n, stream, nonce, bytes, nullptr, dev, pitch, nullptr, nullptr);
}

int tamd_seal_tag(void* h, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes, const void* dev,
                  uint64_t pitch, uint16_t* tag) {
    Sealer* s = (Sealer*)h;
    if (!s || !stream || !nonce || !bytes || !dev || !tag) return -1;
    return packets(s, TAMD_SEAL_M_TAG, n, stream, nonce, bytes, nullptr, dev, pitch, nullptr, tag);
}

int tamd_seal_footers(void* h, uint32_t n, const uint32_t* bytes, const void* dev, uint64_t pitch, uint8_t* footers) {
    Sealer* s = (Sealer*)h;
    if (!s || !bytes || !dev || !footers) return -1;
    std::unique_lock<std::mutex> lk;
    if (const int e = tamd::enter(s, lk)) return e;
    HandleCore& c = s->core;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    if (pitch < largest_within(bytes, n, maxb)) return -3;
    if (!n) return 0;
    if (!c.room(n * sizeof(TailDesc), (size_t)n * TAMD_SEAL_FOOTER)) return -4;
    TailDesc* t = (TailDesc*)c.desc.host;
    for (uint32_t i = 0; i < n; ++i)  // (a datagram longer than the handle allows: all zeros)
        t[i] = TailDesc{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch, bytes[i] <= maxb ? bytes[i] : 0u, 0};
    s->upload_keys();
    const bool ok = c.run(kFooters, n * sizeof(TailDesc), (size_t)n * TAMD_SEAL_FOOTER, [&] {
        hipLaunchKernelGGL(tamd_gather_footers, dim3((n + 255u) / 256u), dim3(256), 0, c.stream, (const TailDesc*)c.desc.dev, n, c.out.dev);
    });
    if (!ok) return -4;
    memcpy(footers, c.out.host, (size_t)n * TAMD_SEAL_FOOTER);
    return 0;
}

}  // extern "C"
