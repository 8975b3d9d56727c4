// CPU check of the device-memory owner (speq_amd/csrc/dev_mem.hpp): includes nothing of the project but that header
// and defines raw_alloc / raw_free itself, over malloc / free, with counters and a fail-the-nth switch. Prints "ok" and
// exits 0, or names the first check that failed. tests/test_dev_mem_cpu.py builds it twice (plain, and with the address
// and undefined-behaviour sanitizers, which see a double free, a leak or a use after free that the counters miss).
#include "dev_mem.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <type_traits>

namespace {
std::set<void*> g_live;
uint64_t g_made = 0, g_freed = 0, g_double = 0;
size_t g_last_bytes = 0;
int64_t g_fail_in = 0;
}  // namespace

namespace speq_dev::mem {
void* raw_alloc(size_t bytes, const char* who) {
    if (g_fail_in > 0 && --g_fail_in == 0) throw OutOfDeviceMemory(std::string(who) + ": out of device memory");
    void* p = std::malloc(bytes);
    if (!p) throw std::bad_alloc();
    std::memset(p, 0xA5, bytes);  // (the sanitizers check the size asked for against the size written)
    g_live.insert(p);
    g_last_bytes = bytes;
    ++g_made;
    return p;
}
void raw_free(void* p) noexcept {
    if (!p) return;
    if (!g_live.erase(p)) {
        ++g_double;  // not live: freed twice, or never allocated here
        return;
    }
    ++g_freed;
    std::free(p);
}
}  // namespace speq_dev::mem

using speq_dev::DevPtr;
using speq_dev::DevTemp;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);               \
            return 1;                                                    \
        }                                                                \
    } while (0)

static_assert(!std::is_copy_constructible_v<DevPtr<int>> && !std::is_copy_assignable_v<DevPtr<int>>, "move-only");
static_assert(std::is_nothrow_move_constructible_v<DevPtr<int>> && std::is_nothrow_move_assignable_v<DevPtr<int>>);
static_assert(sizeof(DevPtr<int>) == sizeof(int*), "an owner is its pointer");

int main() {
    {  // a destructor frees once; an empty owner frees nothing
        DevPtr<uint32_t> e;
        CHECK(!e && e.get() == nullptr);
        {
            DevPtr<uint32_t> a = DevPtr<uint32_t>::alloc(10, "a");
            CHECK(a && a.get() != nullptr && g_made == 1 && g_last_bytes == 40 && g_live.size() == 1);
            a.get()[9] = 7u;
        }
        CHECK(g_freed == 1 && g_live.empty());
    }
    CHECK(g_freed == 1 && g_double == 0);
    {  // a move empties the source
        DevPtr<uint64_t> a = DevPtr<uint64_t>::alloc(3, "a");
        uint64_t* raw = a.get();
        DevPtr<uint64_t> b(std::move(a));
        CHECK(!a && a.get() == nullptr && b.get() == raw && g_live.size() == 1);
        DevPtr<> v(std::move(b));  // ... into an untyped owner too
        CHECK(!b && v.get() == raw && g_live.size() == 1 && g_freed == 1);
    }
    CHECK(g_freed == 2 && g_live.empty() && g_double == 0);
    {  // a move assignment onto a full owner frees what it held, once, and empties the source
        DevPtr<uint8_t> a = DevPtr<uint8_t>::alloc(100, "a"), b = DevPtr<uint8_t>::alloc(200, "b");
        uint8_t *ra = a.get(), *rb = b.get();
        a = std::move(b);
        CHECK(a.get() == rb && !b && g_freed == 3 && !g_live.count(ra) && g_live.count(rb));
        DevPtr<uint8_t>& self = a;
        a = std::move(self);  // onto itself: nothing
        CHECK(a.get() == rb && g_freed == 3);
    }
    CHECK(g_freed == 4 && g_live.empty() && g_double == 0);
    {  // release() hands the pointer over and the owner frees nothing
        void* raw = nullptr;
        {
            DevPtr<> a = DevPtr<>::alloc(64, "a");
            CHECK(g_last_bytes == 64);  // (void counts in bytes)
            raw = a.release();
            CHECK(!a && raw != nullptr);
        }
        CHECK(g_freed == 4 && g_live.count(raw));
        speq_dev::mem::raw_free(raw);
        CHECK(g_freed == 5);
    }
    {  // reset() frees once, and again does nothing
        DevPtr<double> a = DevPtr<double>::alloc(5, "a");
        a.reset();
        CHECK(!a && g_freed == 6);
        a.reset();
    }
    CHECK(g_freed == 6 && g_live.empty() && g_double == 0);
    {  // a zero-size request gets at least 16 bytes, and so does a small one
        DevPtr<uint32_t> z = DevPtr<uint32_t>::alloc(0, "z");
        CHECK(z && g_last_bytes == 16);
        DevPtr<> one = DevPtr<>::alloc(1, "one");
        CHECK(g_last_bytes == 16);
        DevPtr<uint64_t> three = DevPtr<uint64_t>::alloc(3, "three");
        CHECK(g_last_bytes == 24);
    }
    CHECK(g_freed == 9 && g_live.empty());
    // a failing nth allocation in a scope with several owners frees exactly the ones already made
    for (int64_t nth = 1; nth <= 4; ++nth) {
        const uint64_t made0 = g_made, freed0 = g_freed;
        bool threw = false;
        g_fail_in = nth;
        try {
            DevPtr<uint32_t> a = DevPtr<uint32_t>::alloc(8, "a");
            DevPtr<uint64_t> b = DevPtr<uint64_t>::alloc(8, "b"), c = DevPtr<uint64_t>::alloc(8, "c");
            DevPtr<> d = DevPtr<>::alloc(8, "d");
            CHECK(g_live.size() == 4);
        } catch (const speq_dev::OutOfDeviceMemory& e) {
            threw = true;
            CHECK(std::string(e.what()).find("out of device memory") != std::string::npos);
        } catch (const speq::DeviceError&) {
            CHECK(!"OutOfDeviceMemory is caught as itself first");
        }
        CHECK(threw && g_fail_in == 0);
        CHECK(g_made - made0 == (uint64_t)nth - 1 && g_freed - freed0 == (uint64_t)nth - 1 && g_live.empty());
    }
    {  // OutOfDeviceMemory is a DeviceError
        g_fail_in = 1;
        bool as_device_error = false;
        try {
            DevPtr<> a = DevPtr<>::alloc(8, "a");
        } catch (const speq::DeviceError&) {
            as_device_error = true;
        }
        CHECK(as_device_error);
    }
    {  // DevTemp::need grows, keeps its buffer when asked for less, and frees once
        const uint64_t made0 = g_made, freed0 = g_freed;
        {
            DevTemp t;
            CHECK(g_made == made0);  // nothing until asked
            void* p1 = t.need(100, "t");
            CHECK(p1 && g_made == made0 + 1 && g_last_bytes == 100);
            CHECK(t.need(40, "t") == p1 && t.need(100, "t") == p1 && g_made == made0 + 1);
            void* p2 = t.need(1000, "t");
            CHECK(p2 && g_made == made0 + 2 && g_freed == freed0 + 1 && g_last_bytes == 1000 && g_live.size() == 1);
            std::memset(p2, 1, 1000);
            CHECK(t.need(999, "t") == p2);
            g_fail_in = 1;  // a failed growth leaves it empty, and a later need allocates again
            bool threw = false;
            try {
                t.need(5000, "t");
            } catch (const speq_dev::OutOfDeviceMemory&) {
                threw = true;
            }
            CHECK(threw && g_live.empty() && g_freed == freed0 + 2);
            CHECK(t.need(10, "t") != nullptr && g_live.size() == 1);
        }
        CHECK(g_made == made0 + 3 && g_freed == freed0 + 3 && g_live.empty());
        DevTemp zero;
        CHECK(zero.need(0, "t") != nullptr && g_last_bytes == 16);  // rocPRIM takes a null pointer for a size query
    }
    CHECK(g_live.empty() && g_double == 0 && g_made == g_freed);
    std::printf("ok\n");
    return 0;
}
