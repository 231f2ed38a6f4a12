// seal.cpp -- include/tonk_seal.h: batched seal and open of datagrams in the caller's device
// memory.  A handle holds the expanded keys of its streams in a device table (a pinned host copy
// beside it: set_key writes there, and the changed range goes up with the next call's
// descriptors), pinned descriptor and result staging, and one stream.  Every call is one
// descriptor copy, one launch of a kernel of seal.hip, one result copy and one wait.
#include "../../include/tonk_seal.h"

#include "kernel_abi.h"
#include "seal.h"
#include "staging.h"

#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>
#include <stdio.h>
#include <string.h>

using namespace tamd;

namespace {

enum { kPackets = 0, kFooters = 1, kKinds = 2 };

struct Sealer {
    std::mutex mu;
    tamd_seal_params prm;
    int device = -1;
    hipStream_t st = nullptr;
    std::string error;
    bool failed = false;
    tamd_seal_key* keys_host = nullptr;  // pinned
    uint32_t* keys_dev = nullptr;
    uint32_t dirty_lo = ~0u, dirty_hi = 0;  // streams [lo, hi) changed since the last upload
    Staging desc, out;
    bool timing = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    double ms[kKinds] = {0, 0};
    uint64_t launches[kKinds] = {0, 0};

    bool hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        if (!failed) error = std::string(what) + ": " + hipGetErrorString(e);
        failed = true;
        return false;
    }

    // Stage room for n records of `rec` bytes in and `res` bytes out.
    bool room(size_t n, size_t rec, size_t res) {
        if (desc.ensure(n * rec) && out.ensure(n * res)) return true;
        return hip(hipErrorOutOfMemory, "staging allocation");
    }

    // Upload the changed keys and n descriptors, run `launch`, bring `res` bytes per record back
    // and wait.
    template <class F>
    bool run(int kind, size_t n, size_t rec, size_t res, F&& launch) {
        if (dirty_lo < dirty_hi) {
            hip(hipMemcpyAsync(keys_dev + 4 * (size_t)dirty_lo, keys_host + dirty_lo, (size_t)(dirty_hi - dirty_lo) * sizeof(tamd_seal_key),
                               hipMemcpyHostToDevice, st), "key copy");
            dirty_lo = ~0u;
            dirty_hi = 0;
        }
        if (!hip(hipMemcpyAsync(desc.dev, desc.host, n * rec, hipMemcpyHostToDevice, st), "descriptor copy")) return false;
        const bool timed = timing && ev[0] && ev[1];
        if (timed) hip(hipEventRecord(ev[0], st), "hipEventRecord");
        launch();
        hip(hipGetLastError(), "kernel launch");
        if (timed) hip(hipEventRecord(ev[1], st), "hipEventRecord");
        ++launches[kind];
        hip(hipMemcpyAsync(out.host, out.dev, n * res, hipMemcpyDeviceToHost, st), "result copy");
        hip(hipStreamSynchronize(st), "hipStreamSynchronize");
        float v = 0;
        if (timed && !failed && hipEventElapsedTime(&v, ev[0], ev[1]) == hipSuccess) ms[kind] += v;
        return !failed;
    }

    ~Sealer() {
        if (device < 0) return;
        hipSetDevice(device);
        if (st) hipStreamSynchronize(st);
        for (hipEvent_t e : ev)
            if (e) hipEventDestroy(e);
        if (keys_host) hipHostFree(keys_host);
        if (keys_dev) hipFree(keys_dev);
        desc.release();
        out.release();
        if (st) hipStreamDestroy(st);
    }
};

// Common entry checks; returns 0 with the handle locked by `lk` and its device current.
int enter(Sealer* s, std::unique_lock<std::mutex>& lk, uint32_t n, const uint32_t* stream) {
    if (!s) return -1;
    lk = std::unique_lock<std::mutex>(s->mu);
    if (s->failed) return -4;
    for (uint32_t i = 0; stream && i < n; ++i)
        if (stream[i] >= s->prm.n_streams) return -2;
    hipSetDevice(s->device);
    return 0;
}

// seal, open, cipher and tag: one launch of tamd_seal_packets in `mode`.  message_bytes is null
// for the primitives; the results go to rc or tag, whichever is given.
int packets(Sealer* s, uint32_t mode, uint32_t n, const uint32_t* stream, const uint64_t* nonce, const uint32_t* bytes,
            const uint32_t* message_bytes, const void* dev, uint64_t pitch, int32_t* rc, uint16_t* tag) {
    std::unique_lock<std::mutex> lk;
    if (const int e = enter(s, lk, n, stream)) return e;
    const bool datagram = mode & TAMD_SEAL_M_DATAGRAM;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (bytes[i] <= maxb && bytes[i] > largest) largest = bytes[i];
    if (pitch < largest) return -3;
    if (!n) return 0;
    if (!s->room(n, sizeof(SealDesc), sizeof(uint32_t))) return -4;
    SealDesc* d = (SealDesc*)s->desc.host;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t msg = message_bytes ? message_bytes[i] : 0u;
        const bool valid = datagram ? tamd_seal_valid(bytes[i], msg, maxb) : bytes[i] <= maxb;
        d[i] = SealDesc{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch, nonce[i], stream[i], bytes[i], msg, valid ? 0u : 1u};
    }
    const bool ok = s->run(kPackets, n, sizeof(SealDesc), sizeof(uint32_t), [&] {
        hipLaunchKernelGGL(tamd_seal_packets, dim3((n + 63u) / 64u), dim3(512), 0, s->st, (const SealDesc*)s->desc.dev, n,
                           (const uint32_t*)s->keys_dev, mode, (uint32_t*)s->out.dev);
    });
    if (!ok) return -4;
    const uint32_t* o = (const uint32_t*)s->out.host;
    for (uint32_t i = 0; rc && i < n; ++i) rc[i] = (int32_t)o[i];
    for (uint32_t i = 0; tag && i < n; ++i)  // (an entry longer than the handle allows is skipped: tag 0)
        tag[i] = bytes[i] <= maxb ? (uint16_t)o[i] : (uint16_t)0;
    return 0;
}

}  // namespace

extern "C" {

void* tamd_seal_create(const tamd_seal_params* p, char* err, size_t err_len) {
    auto fail = [&](const std::string& m) -> void* {
        if (err && err_len) snprintf(err, err_len, "%s", m.c_str());
        return nullptr;
    };
    if (!p || p->n_streams == 0 || p->max_datagram_bytes == 0 || p->max_datagram_bytes > 65535) return fail("bad parameters");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 0 || (uint32_t)n <= p->device)
        return fail("tonk_amd: no HIP device available (datagrams are sealed only on MI355X/gfx950)");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, (int)p->device) != hipSuccess) return fail("hipGetDeviceProperties failed");
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(std::string("tonk_amd: device is ") + prop.gcnArchName + ", kernels are built for gfx950");
    std::unique_ptr<Sealer> s(new Sealer());
    s->prm = *p;
    if (hipSetDevice((int)p->device) != hipSuccess) return fail("hipSetDevice failed");
    s->device = (int)p->device;
    const size_t kb = (size_t)p->n_streams * sizeof(tamd_seal_key);
    if (hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void**)&s->keys_host, kb, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void**)&s->keys_dev, kb) != hipSuccess || hipMemset(s->keys_dev, 0, kb) != hipSuccess)
        return fail("tonk_amd: the key table could not be allocated");
    memset(s->keys_host, 0, kb);  // (a fresh stream's key is 0; all of its expansion is 0 too)
    return s.release();
}

void tamd_seal_destroy(void* h) {
    Sealer* s = (Sealer*)h;
    if (!s) return;
    { std::lock_guard<std::mutex> lk(s->mu); }
    delete s;
}

const char* tamd_seal_error(void* h) {
    Sealer* s = (Sealer*)h;
    return s ? s->error.c_str() : "bad handle";
}

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
    if (const int e = enter(s, lk, 0, nullptr)) return e;
    const uint32_t maxb = s->prm.max_datagram_bytes;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (bytes[i] <= maxb && bytes[i] > largest) largest = bytes[i];
    if (pitch < largest) return -3;
    if (!n) return 0;
    if (!s->room(n, sizeof(TailDesc), TAMD_SEAL_FOOTER)) return -4;
    TailDesc* t = (TailDesc*)s->desc.host;
    for (uint32_t i = 0; i < n; ++i)  // (a datagram longer than the handle allows: all zeros)
        t[i] = TailDesc{(uint64_t)(uintptr_t)dev + (uint64_t)i * pitch, bytes[i] <= maxb ? bytes[i] : 0u, 0};
    const bool ok = s->run(kFooters, n, sizeof(TailDesc), TAMD_SEAL_FOOTER, [&] {
        hipLaunchKernelGGL(tamd_gather_footers, dim3((n + 255u) / 256u), dim3(256), 0, s->st, (const TailDesc*)s->desc.dev, n, s->out.dev);
    });
    if (!ok) return -4;
    memcpy(footers, s->out.host, (size_t)n * TAMD_SEAL_FOOTER);
    return 0;
}

void tamd_seal_set_timing(void* h, int on) {
    Sealer* s = (Sealer*)h;
    if (!s) return;
    std::lock_guard<std::mutex> lk(s->mu);
    hipSetDevice(s->device);
    s->timing = on != 0;
    for (hipEvent_t& e : s->ev)
        if (on && !e && hipEventCreate(&e) != hipSuccess) e = nullptr;
}

void tamd_seal_kernel_ms(void* h, double* out, unsigned n) {
    Sealer* s = (Sealer*)h;
    if (!s || !out) return;
    std::lock_guard<std::mutex> lk(s->mu);
    const double v[4] = {s->ms[kPackets], s->ms[kFooters], (double)s->launches[kPackets], (double)s->launches[kFooters]};
    for (unsigned i = 0; i < n && i < 4; ++i) out[i] = v[i];
    for (int k = 0; k < kKinds; ++k) { s->ms[k] = 0; s->launches[k] = 0; }
}

}  // extern "C"
