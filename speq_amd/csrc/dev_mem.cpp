// dev_mem.hpp's raw_alloc / raw_free for the library: the only hipMalloc / hipFree of the device half, and the
// allocation counters and the one-shot failure the tests drive (tests/test_gpu_alloc_failures.py); and the only
// hipMemGetInfo, with the two switches that make the library believe memory is short or a buffer offset narrow
// (tests/test_gpu_fallbacks.py).
#include "dev_mem.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

namespace {
std::atomic<uint64_t> g_live{0}, g_made{0};
std::atomic<int64_t> g_fail_in{0};  // > 0: that many allocations from now, one fails
std::atomic<uint64_t> g_queries{0};
std::atomic<int64_t> g_short_in{0};  // > 0: that many free-memory queries from now, one answers at most g_short_bytes
std::atomic<uint64_t> g_short_bytes{0};
std::atomic<uint64_t> g_offset_limit{1ull << 32};
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

uint64_t free_bytes() {
    size_t free_b = 0, total_b = 0;
    const hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess) throw speq::DeviceError(std::string("hipMemGetInfo: ") + hipGetErrorString(e));
    g_queries.fetch_add(1, std::memory_order_relaxed);
    if (g_short_in.load(std::memory_order_relaxed) > 0 && g_short_in.fetch_sub(1, std::memory_order_relaxed) == 1)
        return std::min<uint64_t>(free_b, g_short_bytes.load(std::memory_order_relaxed));
    return free_b;
}

uint64_t offset_limit() { return g_offset_limit.load(std::memory_order_relaxed); }

}  // namespace speq_dev::mem

extern "C" {

void speq_debug_allocs(uint64_t* live, uint64_t* made) {
    if (live) *live = g_live.load(std::memory_order_relaxed);
    if (made) *made = g_made.load(std::memory_order_relaxed);
}

void speq_debug_fail_alloc(int64_t nth) { g_fail_in.store(nth > 0 ? nth : 0, std::memory_order_relaxed); }

void speq_debug_free_queries(uint64_t* made) {
    if (made) *made = g_queries.load(std::memory_order_relaxed);
}

void speq_debug_free_bytes(int64_t nth, uint64_t bytes) {
    g_short_bytes.store(bytes, std::memory_order_relaxed);
    g_short_in.store(nth > 0 ? nth : 0, std::memory_order_relaxed);
}

void speq_debug_offset_limit(uint64_t limit) {
    const uint64_t span = 1ull << 32;
    const uint64_t v = limit == 0 ? span : std::min(std::max<uint64_t>(limit, 4096), span);
    g_offset_limit.store(v, std::memory_order_relaxed);
}

}  // extern "C"
