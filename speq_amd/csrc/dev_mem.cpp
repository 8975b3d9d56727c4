// dev_mem.hpp's raw_alloc / raw_free for the library: the only hipMalloc / hipFree of the device half, and the
// allocation counters and the one-shot failure the tests drive (tests/test_gpu_alloc_failures.py).
#include "dev_mem.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

namespace {
std::atomic<uint64_t> g_live{0}, g_made{0};
std::atomic<int64_t> g_fail_in{0};  // > 0: that many allocations from now, one fails
}  // namespace

namespace speq_dev::mem {

void* raw_alloc(size_t bytes, const char* who) {
    auto nomem = [&](const char* note) {
        return OutOfDeviceMemory(std::string(who) + ": out of device memory (" + std::to_string(bytes) + " bytes)" + note);
    };
    if (g_fail_in.load(std::memory_order_relaxed) > 0 && g_fail_in.fetch_sub(1, std::memory_order_relaxed) == 1)
        throw nomem(" [injected]");
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 16));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        throw nomem("");
    }
    if (e != hipSuccess) throw speq::DeviceError(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    g_live.fetch_add(1, std::memory_order_relaxed);
    g_made.fetch_add(1, std::memory_order_relaxed);
    return p;
}

void raw_free(void* p) noexcept {
    if (!p) return;
    (void)hipFree(p);
    g_live.fetch_sub(1, std::memory_order_relaxed);
}

}  // namespace speq_dev::mem

extern "C" {

void speq_debug_allocs(uint64_t* live, uint64_t* made) {
    if (live) *live = g_live.load(std::memory_order_relaxed);
    if (made) *made = g_made.load(std::memory_order_relaxed);
}

void speq_debug_fail_alloc(int64_t nth) { g_fail_in.store(nth > 0 ? nth : 0, std::memory_order_relaxed); }

}  // extern "C"
