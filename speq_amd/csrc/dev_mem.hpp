// The one owner of device memory ("Who owns device memory"). Host-only, no HIP include: written against
// raw_alloc / raw_free, which dev_mem.cpp defines for the library over hipMalloc / hipFree (tests/dev_mem_check.cpp
// defines them over malloc). A buffer has an owner from the line it is allocated on, so no path can leave without
// freeing it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "speq_errors.hpp"

namespace speq_dev {

// a device allocation that does not fit: SPEQ_E_DEVICE through guarded(), SPEQ_E_NOMEM through guarded_nomem()
struct OutOfDeviceMemory : speq::DeviceError {
    using speq::DeviceError::DeviceError;
};

namespace mem {
// `bytes` of device memory on the current device, or throws: OutOfDeviceMemory ("who: out of device memory (N
// bytes)") when it does not fit, speq::DeviceError for any other failure.
void* raw_alloc(size_t bytes, const char* who);
void raw_free(void* p) noexcept;  // null: nothing
// Free bytes of the current device: the library's only question of this kind (build_limits.hpp decides from the
// answer). Throws speq::DeviceError when the device does not answer.
uint64_t free_bytes();
// The span of a 32-bit buffer offset, 2^32, as build_limits.hpp's offset decisions take it (host side only).
uint64_t offset_limit();
}  // namespace mem

// Move-only owner of one device allocation; frees it when it goes. T = void counts in bytes.
template <class T = void>
class DevPtr {
    T* p_ = nullptr;
    template <class U>
    friend class DevPtr;

public:
    DevPtr() = default;
    // `count` elements (never fewer than 16 bytes, so an empty array still has an address)
    static DevPtr alloc(size_t count, const char* who) {
        size_t elem = 1;
        if constexpr (!std::is_void_v<T>) elem = sizeof(T);
        DevPtr r;
        r.p_ = static_cast<T*>(mem::raw_alloc(std::max<size_t>(count * elem, 16), who));
        return r;
    }
    DevPtr(DevPtr&& o) noexcept : p_(o.release()) {}
    template <class U, class = std::enable_if_t<std::is_void_v<T> && !std::is_void_v<U>>>
    DevPtr(DevPtr<U>&& o) noexcept : p_(o.release()) {}  // any owner becomes an untyped one (the replica's list)
    DevPtr& operator=(DevPtr&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.release();
        }
        return *this;
    }
    DevPtr(const DevPtr&) = delete;
    DevPtr& operator=(const DevPtr&) = delete;
    ~DevPtr() { reset(); }

    T* get() const { return p_; }
    T* release() { return std::exchange(p_, nullptr); }  // the caller owns the memory now (mem::raw_free)
    void reset() { mem::raw_free(std::exchange(p_, nullptr)); }
    explicit operator bool() const { return p_ != nullptr; }
};

// Grow-only scratch (rocPRIM's temporary storage): need() returns a buffer of at least `bytes`, the one it has when
// that is large enough.
class DevTemp {
    DevPtr<> buf_;
    size_t cap_ = 0;

public:
    void* need(size_t bytes, const char* who) {
        if (bytes > cap_ || !buf_) {
            buf_.reset();  // first, so that the two are never alive together
            cap_ = 0;
            buf_ = DevPtr<>::alloc(bytes, who);
            cap_ = bytes;
        }
        return buf_.get();
    }
};

}  // namespace speq_dev

extern "C" {
// Test seam (tests bind these with ctypes; not part of include/speq_scan.h). live: allocations made through
// raw_alloc and not yet freed; made: allocations made since the process started.
void speq_debug_allocs(uint64_t* live, uint64_t* made);
// The nth allocation from now throws OutOfDeviceMemory before the device is asked; one-shot, 0 disarms.
void speq_debug_fail_alloc(int64_t nth);
// made: free-memory queries (mem::free_bytes) since the process started.
void speq_debug_free_queries(uint64_t* made);
// The nth free-memory query from now answers min(real, bytes): the library believes memory is short, none is taken.
// One-shot, nth 0 disarms.
void speq_debug_free_bytes(int64_t nth, uint64_t bytes);
// mem::offset_limit() answers `limit` (clamped to [4096, 2^32]) until it is set again; 0 restores 2^32. What was
// decided under a limit (a refused table, an unpublished plane family) stays decided.
void speq_debug_offset_limit(uint64_t limit);
}
