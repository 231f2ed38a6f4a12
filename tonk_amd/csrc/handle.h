// handle.h -- what the batched device interfaces share (batch.cpp, seal.cpp, dgram.cpp, cbatch.cpp): the
// device check, the launch timer, the core of a handle (lock, device, stream, sticky error,
// staging, one call's copy-launch-copy-wait) and the common parts of the C entry points.  A handle
// type is a plain struct with a member `core`.
#pragma once
#include "staging.h"

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>
#include <stdio.h>
#include <string.h>

namespace tamd {

// Why device `index` cannot run the kernels, or "" when it can.  `what`: what runs only there
// ("datagrams are sealed").
inline std::string device_check(uint32_t index, const char* what) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 0 || (uint32_t)n <= index)
        return std::string("tonk_amd: no HIP device available (") + what + " only on MI355X/gfx950)";
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, (int)index) != hipSuccess) return "hipGetDeviceProperties failed";
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return std::string("tonk_amd: device is ") + prop.gcnArchName + ", kernels are built for gfx950";
    return "";
}

// The largest of len[0 .. n) that is at most `limit` (a longer entry is refused by itself, and
// does not decide whether the pitch holds the call's packets).
inline uint32_t largest_within(const uint32_t* len, uint32_t n, uint32_t limit) {
    uint32_t largest = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (len[i] <= limit && len[i] > largest) largest = len[i];
    return largest;
}

// Launches per kind of kernel and, while `on`, their device times from a pool of events.  With
// timing off no event call is made.
struct LaunchTimer {
    enum { kMaxKinds = 4 };
    bool on = false;
    double ms[kMaxKinds] = {0, 0, 0, 0};
    uint64_t launches[kMaxKinds] = {0, 0, 0, 0};
    struct Timed { int kind; hipEvent_t a, b; };
    std::vector<Timed> timed;  // enqueued, not read yet
    std::vector<hipEvent_t> events;

    template <class Core>
    hipEvent_t event(Core& c) {
        hipEvent_t e = nullptr;
        if (events.empty()) return c.hip(hipEventCreate(&e), "hipEventCreate"), e;
        e = events.back();
        events.pop_back();
        return e;
    }
    // Enqueue f's kernel on c.stream, between two events when timing is on.
    template <class Core, class F>
    void launch(Core& c, int kind, F&& f) {
        Timed t{kind, nullptr, nullptr};
        if (on) {
            t.a = event(c);
            t.b = event(c);
            if (t.a) c.hip(hipEventRecord(t.a, c.stream), "hipEventRecord");
        }
        f();
        c.hip(hipGetLastError(), "kernel launch");
        ++launches[kind];
        if (t.a && t.b) {
            c.hip(hipEventRecord(t.b, c.stream), "hipEventRecord");
            timed.push_back(t);
        } else if (t.a) {
            events.push_back(t.a);
        }
    }
    // After the stream's wait: the timed launches' durations (one that cannot be read adds nothing).
    void collect() {
        for (const Timed& t : timed) {
            float v = 0;
            if (hipEventElapsedTime(&v, t.a, t.b) == hipSuccess) ms[t.kind] += v;
            events.push_back(t.a);
            events.push_back(t.b);
        }
        timed.clear();
    }
    void reset() {
        for (int k = 0; k < kMaxKinds; ++k) { ms[k] = 0; launches[k] = 0; }
    }
    void release() {  // (the handle's device current, its stream idle)
        collect();
        for (hipEvent_t e : events) hipEventDestroy(e);
        events.clear();
    }
};

struct HandleCore {
    std::mutex mu;
    int device = -1;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    std::string error;  // of the first call that failed
    bool failed = false;  // sticky
    Staging desc, out;  // a call's descriptors up, its results down
    LaunchTimer timer;

    bool hip(hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        if (!failed) error = std::string(what) + ": " + hipGetErrorString(e);
        failed = true;
        return false;
    }
    // Make `index` current and create the handle's own stream; "" or what failed.
    std::string open(uint32_t index) {
        if (hipSetDevice((int)index) != hipSuccess) return "hipSetDevice failed";
        device = (int)index;
        if (hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return "tonk_amd: the stream could not be created";
        owns_stream = true;
        return "";
    }
    bool room(size_t up_bytes, size_t down_bytes) {
        if (desc.ensure(up_bytes) && out.ensure(down_bytes)) return true;
        return hip(hipErrorOutOfMemory, "staging allocation");
    }
    template <class F>
    void launch_timed(int kind, F&& f) { timer.launch(*this, kind, f); }
    // Upload `up` descriptor bytes, let `enqueue` put the call's launches on the stream (each through
    // launch_timed), bring `down` result bytes back (none: no copy) and wait.
    template <class F>
    bool run_all(size_t up, size_t down, F&& enqueue) {
        if (!hip(hipMemcpyAsync(desc.dev, desc.host, up, hipMemcpyHostToDevice, stream), "descriptor copy")) return false;
        enqueue();
        if (down) hip(hipMemcpyAsync(out.host, out.dev, down, hipMemcpyDeviceToHost, stream), "result copy");
        hip(hipStreamSynchronize(stream), "hipStreamSynchronize");
        timer.collect();
        return !failed;
    }
    // The same for a call that is one launch.
    template <class F>
    bool run(int kind, size_t up, size_t down, F&& launch) {
        return run_all(up, down, [&] { launch_timed(kind, launch); });
    }
    ~HandleCore() {
        if (device < 0) return;
        hipSetDevice(device);
        if (stream) hipStreamSynchronize(stream);
        timer.release();
        desc.release();
        out.release();
        if (owns_stream) hipStreamDestroy(stream);
    }
};

// ---- the common parts of the C entry points; T is a handle type ----

// Creation failed: the text into the caller's buffer.
inline void* fail(char* err, size_t err_len, const std::string& text) {
    if (err && err_len) snprintf(err, err_len, "%s", text.c_str());
    return nullptr;
}

// Entry checks of a call; returns 0 with the handle locked by `lk` and its device current.
template <class T>
int enter(T* h, std::unique_lock<std::mutex>& lk) {
    if (!h) return -1;
    lk = std::unique_lock<std::mutex>(h->core.mu);
    if (h->core.failed) return -4;
    hipSetDevice(h->core.device);
    return 0;
}

template <class T>
void destroy(void* h) {
    T* p = (T*)h;
    if (!p) return;
    { std::lock_guard<std::mutex> lk(p->core.mu); }  // (a call in another thread ends first)
    delete p;
}

template <class T>
const char* error_text(void* h) {
    return h ? ((T*)h)->core.error.c_str() : "bad handle";
}

template <class T>
void set_timing(void* h, int on) {
    if (!h) return;
    std::lock_guard<std::mutex> lk(((T*)h)->core.mu);
    ((T*)h)->core.timer.on = on != 0;
}

// ms[0 .. k) then launches[0 .. k) into out[0 .. n), and both start again from 0.
template <class T>
void kernel_ms(void* h, double* out, unsigned n, unsigned k) {
    if (!h || !out) return;
    HandleCore& c = ((T*)h)->core;
    std::lock_guard<std::mutex> lk(c.mu);
    for (unsigned i = 0; i < n && i < 2 * k; ++i) out[i] = i < k ? c.timer.ms[i] : (double)c.timer.launches[i - k];
    c.timer.reset();
}

}  // namespace tamd
