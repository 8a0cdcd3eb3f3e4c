// device_buffer.hpp -- the HIP error check, the owning device buffer and the event timer of the device solvers
// (sw2d_device.hip, sw2d_curved_device.hip, sw2d_quad_device.hip, poisson2d_device.hip).
#pragma once
#include "../host/capi_internal.hpp"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <vector>

namespace bdg_dev {

inline void hipCheck(hipError_t e, const char* what) {
    if (e != hipSuccess) throw bdg_detail::hip_error(std::string(what) + ": " + hipGetErrorString(e));
}

// `total` counts the bytes of the live allocations: replacing a live buffer stops counting its old size; release()
// on its own leaves the count as it is.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count, size_t& total) {
        if (p) total -= std::min(total, n * sizeof(T));
        release();
        if (count == 0) return;
        hipCheck(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)), "hipMalloc");
        n = count;
        total += count * sizeof(T);
    }
    // ... and zeroed on `zeroOn`
    void alloc(size_t count, size_t& total, hipStream_t zeroOn) {
        alloc(count, total);
        zero(zeroOn);
    }
    // allocated to the size of `host` and filled from it by a blocking copy; `what` names the copy in an error
    void upload(const std::vector<T>& host, size_t& total, const char* what) {
        alloc(host.size(), total);
        if (p) hipCheck(hipMemcpy(p, host.data(), n * sizeof(T), hipMemcpyHostToDevice), what);
    }
    void zero(hipStream_t on) {
        if (p) hipCheck(hipMemsetAsync(p, 0, n * sizeof(T), on), "hipMemset");
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
};

// an owned event: destroyed on every way out, a throwing hipCheck included
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() { hipCheck(hipEventCreate(&e), "hipEventCreate"); }
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    ~DevEvent() { (void)hipEventDestroy(e); }
};

// `body()` run `count` times between two events on `stream`, waited for: device milliseconds per run
template <class Body>
float timePerRun(hipStream_t stream, int count, Body&& body) {
    DevEvent a, b;
    hipCheck(hipEventRecord(a.e, stream), "hipEventRecord");
    for (int i = 0; i < count; ++i) body();
    hipCheck(hipEventRecord(b.e, stream), "hipEventRecord");
    hipCheck(hipEventSynchronize(b.e), "hipEventSynchronize");
    float ms = 0.0f;
    hipCheck(hipEventElapsedTime(&ms, a.e, b.e), "hipEventElapsedTime");
    return ms / count;
}

} // namespace bdg_dev
