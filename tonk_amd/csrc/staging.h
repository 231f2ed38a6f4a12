// staging.h -- the pinned staging buffer of the batched interfaces' handles (handle.h: batch.cpp,
// seal.cpp, dgram.cpp).  It is freed with its handle (unlike lz_host.h's Buffer, which has static
// lifetime and is never freed at exit).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

namespace tamd {

// A pinned host buffer and its device twin, grown on demand (the device is idle between calls).
struct Staging {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap) return true;
        release();
        const size_t want = n + n / 2 + 4096;
        if (hipHostMalloc((void**)&host, want, hipHostMallocDefault) != hipSuccess) { host = nullptr; return false; }
        if (hipMalloc((void**)&dev, want) != hipSuccess) { dev = nullptr; release(); return false; }
        cap = want;
        return true;
    }
    void release() {
        if (host) hipHostFree(host);
        if (dev) hipFree(dev);
        host = dev = nullptr;
        cap = 0;
    }
    ~Staging() { release(); }
};

}  // namespace tamd
