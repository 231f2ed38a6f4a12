// lz_host.h -- host plumbing shared by the two sides of the compression step (compress.cpp,
// decompress.cpp): the device check, grow-on-demand buffers, recycled device memory of closed
// connections, and the leader's stream.  Internal to the two files (each has its own copies of
// the functions and no state lives here).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string.h>
#include <utility>
#include <vector>

namespace tamd {
namespace {

bool device_ok() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return false;
    int dev = 0;
    hipGetDevice(&dev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// A device buffer (and, when asked, a pinned host twin) grown on demand; contents are not kept.
// `need` and `cap` count entries of `unit` bytes: buffers given the same counts grow together.
struct Buffer {
    uint8_t* h = nullptr;
    uint8_t* d = nullptr;
    size_t cap = 0;
    bool grow(size_t need, bool host, size_t unit = 1) {
        if (need <= cap) return true;
        if (h) hipHostFree(h);
        if (d) hipFree(d);
        h = d = nullptr;
        cap = need + need / 2;
        if (hipMalloc((void**)&d, cap * unit) != hipSuccess ||
            (host && hipHostMalloc((void**)&h, cap * unit, hipHostMallocDefault) != hipSuccess)) {
            cap = 0;
            return false;
        }
        return true;
    }
};

// Device allocations of `Bytes` (a compressor's ring, a decompressor's stream memory) kept per
// device for the next owner and never freed: hipFree waits for the whole device (every stream of
// the process, the Siamese codecs' too), and Tonk destroys a compressor and a decompressor with
// every connection it closes.  One pool per size: allocations of two sizes are never exchanged.
template <size_t Bytes>
class DevicePool {
public:
    // A recycled allocation of `device` (contents stale) or a new one on the current device;
    // null when there is no memory.
    uint8_t* take(int device) {
        {
            std::lock_guard<std::mutex> g(mu_);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].first == device) {
                    uint8_t* p = free_[i].second;
                    free_[i] = free_.back();
                    free_.pop_back();
                    return p;
                }
        }
        uint8_t* p = nullptr;
        return hipMalloc((void**)&p, Bytes) == hipSuccess ? p : nullptr;
    }
    void put(int device, uint8_t* p) {
        std::lock_guard<std::mutex> g(mu_);
        free_.push_back(std::make_pair(device, p));
    }

private:
    std::mutex mu_;
    std::vector<std::pair<int, uint8_t*>> free_;
};

// The leader's stream: `use` makes the batch's device current; on a device change the stream is
// destroyed and recreated (a process works on one device in practice).
struct LeaderStream {
    int device = -1;
    hipStream_t st = nullptr;
    bool use(int dev) {
        if (hipSetDevice(dev) != hipSuccess) return false;
        if (device == dev) return true;
        if (st) hipStreamDestroy(st);
        st = nullptr;
        const bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess;
        device = ok ? dev : -1;
        return ok;
    }
};

}  // namespace
}  // namespace tamd
