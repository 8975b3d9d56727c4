// CPU check of a pipeline slot's buffers (speq_amd/csrc/slot_buffers.hpp): includes nothing of the project but that
// header and dev_mem.hpp, and defines the four seam functions itself over malloc / free, with counters, the size and
// the kind of every live allocation, and a fail-the-nth switch that counts device and pinned allocations together.
// Prints "ok" and exits 0, or names the first check that failed. tests/test_slot_buffers_cpu.py builds it twice (plain,
// and with the address and undefined-behaviour sanitizers).
//
// Every operation is run once to count its allocations N; then each of 1..N fails once on a set in the same state as
// before, the invariant of the header is checked field by field (exactly as it was, or empty), and the same call is
// repeated on the same set (an emptied one brought back to the state before first, as a slot's next acquire does) and
// has to succeed with the result of the clean run.
#include "slot_buffers.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <tuple>
#include <type_traits>

using speq_dev::PinnedHow;
using speq_dev::SlotBuffers;

namespace {
struct Live {
    size_t bytes;
    bool pinned;
    PinnedHow how;
};
std::map<void*, Live> g_live;
uint64_t g_made = 0, g_freed = 0, g_bad_free = 0;
int64_t g_fail_in = 0;

void* take(size_t bytes, bool pinned, PinnedHow how, const char* who) {
    if (g_fail_in > 0 && --g_fail_in == 0) throw speq_dev::OutOfDeviceMemory(std::string(who) + ": out of memory");
    void* p = std::malloc(bytes);
    if (!p) throw std::bad_alloc();
    std::memset(p, 0xA5, bytes);  // (the sanitizers check the size asked for against the size written)
    g_live[p] = Live{bytes, pinned, how};
    ++g_made;
    return p;
}
void give(void* p, bool pinned, PinnedHow how) {
    if (!p) return;
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second.pinned != pinned || (pinned && it->second.how != how)) {
        ++g_bad_free;  // freed twice, never allocated here, through the other seam, or released the wrong way
        return;
    }
    g_live.erase(it);
    ++g_freed;
    std::free(p);
}
}  // namespace

namespace speq_dev::mem {
void* raw_alloc(size_t bytes, const char* who) { return take(bytes, false, PinnedHow::registered, who); }
void raw_free(void* p) noexcept { give(p, false, PinnedHow::registered); }
PinnedMem pinned_alloc(size_t bytes, const char* who) {  // (both kinds in turn: the owner has to hand its own back)
    const PinnedHow how = (g_made & 1) ? PinnedHow::host_malloc : PinnedHow::registered;
    return {take(bytes, true, how, who), how};
}
void pinned_free(void* p, PinnedHow how) noexcept { give(p, true, how); }
}  // namespace speq_dev::mem

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("line %d (%s): %s\n", __LINE__, g_what, #cond);       \
            return 1;                                                         \
        }                                                                     \
    } while (0)

namespace {
const char* g_what = "";

static_assert(!std::is_copy_constructible_v<SlotBuffers> && !std::is_copy_assignable_v<SlotBuffers>, "move-only");
static_assert(std::is_nothrow_move_constructible_v<SlotBuffers> && std::is_nothrow_move_assignable_v<SlotBuffers>);
static_assert(!std::is_copy_constructible_v<speq_dev::PinnedPtr<int>>, "move-only");

// every field of a set
auto fields(const SlotBuffers& s) {
    return std::make_tuple((void*)s.h_seq.get(), (void*)s.h_qual.get(), (void*)s.h_off.get(), (void*)s.d_seq.get(),
                           (void*)s.d_qual.get(), (void*)s.d_off.get(), (void*)s.d_pseq.get(), (void*)s.d_pqual.get(),
                           (void*)s.d_poff.get(), s.d_scratch.get(), s.cap_bytes, s.cap_records, s.parse_bytes,
                           s.parse_slots, s.scratch_bytes);
}
bool all_zero(const SlotBuffers& s) { return fields(s) == fields(SlotBuffers()); }

// p is live, of the right kind, and was asked for with exactly `bytes`
bool holds(const void* p, size_t bytes, bool pinned) {
    auto it = g_live.find(const_cast<void*>(p));
    return it != g_live.end() && it->second.pinned == pinned && it->second.bytes == bytes;
}

// Every pointer beside the capacity that describes it, and no host buffer without its device twin. pad: what the
// parse buffers were asked for past parse_bytes.
int consistent(const SlotBuffers& s, uint64_t pad) {
    if (s.cap_bytes == 0) {
        CHECK(!s.h_seq && !s.h_qual && !s.h_off && !s.d_seq && !s.d_qual && !s.d_off && s.cap_records == 0);
    } else {
        CHECK(s.cap_bytes >= 64 && s.cap_records >= 2);
        CHECK(holds(s.h_seq.get(), s.cap_bytes, true) && holds(s.d_seq.get(), s.cap_bytes + 64, false));
        CHECK(holds(s.h_off.get(), (s.cap_records + 1) * 8, true));
        CHECK(holds(s.d_off.get(), (s.cap_records + 1) * 8, false));
        CHECK((bool)s.h_qual == (bool)s.d_qual);
        if (s.h_qual) CHECK(holds(s.h_qual.get(), s.cap_bytes, true) && holds(s.d_qual.get(), s.cap_bytes, false));
    }
    if (s.parse_bytes == 0) {
        CHECK(!s.d_pseq && !s.d_pqual && !s.d_poff && !s.d_scratch && s.parse_slots == 0 && s.scratch_bytes == 0);
    } else {
        CHECK(holds(s.d_pseq.get(), s.parse_bytes + pad, false) && holds(s.d_pqual.get(), s.parse_bytes + pad, false));
        CHECK((bool)s.d_poff == (s.scratch_bytes != 0) && (bool)s.d_scratch == (s.scratch_bytes != 0));
        if (s.scratch_bytes)
            CHECK(holds(s.d_poff.get(), (s.parse_slots + 1) * 8, false) &&
                  holds(s.d_scratch.get(), std::max<size_t>(s.scratch_bytes, 16), false));
    }
    return 0;
}

// how many live allocations a set owns
size_t owned(const SlotBuffers& s) {
    size_t n = 0;
    for (const void* p : {(const void*)s.h_seq.get(), (const void*)s.h_qual.get(), (const void*)s.h_off.get(),
                          (const void*)s.d_seq.get(), (const void*)s.d_qual.get(), (const void*)s.d_off.get(),
                          (const void*)s.d_pseq.get(), (const void*)s.d_pqual.get(), (const void*)s.d_poff.get(),
                          (const void*)s.d_scratch.get()})
        n += p != nullptr;
    return n;
}

// make(): a set in the state before the operation; op(set): the operation; expect(set): the result of a clean run.
// n_expected: the allocations of the clean run. keeps: which failing n leave the set as it was (the others empty it).
template <class Make, class Op, class Expect>
int fails_once_each(const char* what, uint64_t n_expected, uint64_t pad, Make make, Op op, Expect expect,
                    uint64_t keeps_from = ~0ull) {
    g_what = what;
    uint64_t N = 0;
    {
        SlotBuffers s = make();
        const uint64_t made0 = g_made;
        op(s);
        N = g_made - made0;
        CHECK(N == n_expected);
        CHECK(expect(s) && consistent(s, pad) == 0 && g_live.size() == owned(s));
    }
    CHECK(g_live.empty());
    for (uint64_t n = 1; n <= N; ++n) {
        SlotBuffers s = make();
        const auto before = fields(s);
        bool threw = false;
        g_fail_in = (int64_t)n;
        try {
            op(s);
        } catch (const speq_dev::OutOfDeviceMemory&) {
            threw = true;
        }
        CHECK(threw && g_fail_in == 0);
        if (n >= keeps_from) CHECK(fields(s) == before);
        else CHECK(all_zero(s));
        CHECK(consistent(s, pad) == 0 && g_live.size() == owned(s));  // (nothing alive that the set does not hold)
        op(s);  // the same call on the same set
        CHECK(expect(s) && consistent(s, pad) == 0 && g_live.size() == owned(s));
    }
    CHECK(g_live.empty() && g_bad_free == 0 && g_made == g_freed);
    return 0;
}

SlotBuffers none() { return SlotBuffers(); }
SlotBuffers plain(uint64_t bytes, uint64_t records, bool qual) {
    SlotBuffers s;
    s.ensure(bytes, records, qual);
    return s;
}
size_t scratch_for(uint64_t bytes, uint64_t slots) { return (size_t)(bytes / 4 + slots * 8); }

int run() {
    // ensure, fresh: text and offsets on both sides; with qualities two more; the minimums
    if (fails_once_each("ensure fresh", 4, 0, none, [](SlotBuffers& s) { s.ensure(1000, 10, false); },
                        [](const SlotBuffers& s) { return s.cap_bytes == 1000 && s.cap_records == 10 && !s.h_qual; }))
        return 1;
    if (fails_once_each("ensure fresh with qualities", 6, 0, none, [](SlotBuffers& s) { s.ensure(1000, 10, true); },
                        [](const SlotBuffers& s) { return s.cap_bytes == 1000 && s.cap_records == 10 && s.h_qual; }))
        return 1;
    if (fails_once_each("ensure minimums", 4, 0, none, [](SlotBuffers& s) { s.ensure(1, 0, false); },
                        [](const SlotBuffers& s) { return s.cap_bytes == 64 && s.cap_records == 2; }))
        return 1;
    // ensure, growing: the old buffers go first, either size grows alone and the other stays, qualities are kept, and
    // so are the parse buffers of a set that has them (a failure empties those too)
    if (fails_once_each("ensure growing bytes", 4, 0, [] { return plain(1000, 10, false); },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) s.ensure(1000, 10, false);  // (the repeat after a failure)
                            s.ensure(5000, 4, false);
                        },
                        [](const SlotBuffers& s) { return s.cap_bytes == 5000 && s.cap_records == 10 && !s.h_qual; }))
        return 1;
    if (fails_once_each("ensure growing records, qualities kept", 6, 0, [] { return plain(1000, 10, true); },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) s.ensure(1000, 10, true);
                            s.ensure(100, 50, false);
                        },
                        [](const SlotBuffers& s) { return s.cap_bytes == 1000 && s.cap_records == 50 && s.h_qual; }))
        return 1;
    if (fails_once_each("ensure growing beside parse buffers", 4, 0,
                        [] {
                            SlotBuffers s = plain(1000, 10, false);
                            s.ensure_parse(1000, 10, 300, 0);
                            return s;
                        },
                        [](SlotBuffers& s) {
                            s.ensure(2000, 10, false);
                            if (!s.d_pseq) s.ensure_parse(1000, 10, 300, 0);  // (the repeat after a failure)
                        },
                        [](const SlotBuffers& s) {
                            return s.cap_bytes == 2000 && s.parse_bytes >= 1000 && s.d_scratch;
                        }))
        return 1;
    {  // ... and the old buffers are gone before the new ones are asked for
        g_what = "ensure frees first";
        SlotBuffers s = plain(1000, 10, true);
        g_fail_in = 1;
        bool threw = false;
        try {
            s.ensure(2000, 10, false);
        } catch (const speq_dev::OutOfDeviceMemory&) {
            threw = true;
        }
        CHECK(threw && g_live.empty() && all_zero(s));
    }
    // ensure, adding qualities to a set that has none: both halves or neither. n = 2 is the device half failing after
    // the host half was made: the set stays exactly as it was, with no host qualities either
    if (fails_once_each("ensure adding qualities", 2, 0, [] { return plain(1000, 10, false); },
                        [](SlotBuffers& s) { s.ensure(1000, 10, true); },
                        [](const SlotBuffers& s) { return s.cap_bytes == 1000 && s.h_qual && s.d_qual; }, 1))
        return 1;
    {
        g_what = "a quality buffer whose device half fails";
        SlotBuffers s = plain(1000, 10, false);
        const auto before = fields(s);
        g_fail_in = 2;
        bool threw = false;
        try {
            s.ensure(500, 5, true);
        } catch (const speq_dev::OutOfDeviceMemory&) {
            threw = true;
        }
        CHECK(threw && !s.h_qual && !s.d_qual && fields(s) == before && g_live.size() == 4);
        s.ensure(500, 5, true);
        CHECK(s.h_qual && s.d_qual && s.cap_bytes == 1000 && consistent(s, 0) == 0 && g_live.size() == 6);
        s.ensure(500, 5, false);  // nothing to do: no allocation
        CHECK(g_live.size() == 6);
    }
    CHECK(g_live.empty() && g_bad_free == 0 && g_made == g_freed);
    // ensure_parse, fresh: sized for the slot's capacity; without scratch neither offsets nor scratch, and the pad
    if (fails_once_each("ensure_parse fresh with scratch", 4, 0, [] { return plain(1000, 10, false); },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) s.ensure(1000, 10, false);  // (the repeat after a failure)
                            s.ensure_parse(600, 4, 300, 0, scratch_for);
                        },
                        [](const SlotBuffers& s) {
                            return s.parse_bytes == 1000 && s.parse_slots == 10 && s.scratch_bytes == 330;
                        }))
        return 1;
    if (fails_once_each("ensure_parse fresh without scratch", 2, 16, [] { return plain(1000, 10, false); },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) s.ensure(1000, 10, false);
                            s.ensure_parse(600, 4, 0, 16);
                        },
                        [](const SlotBuffers& s) {
                            return s.parse_bytes == 1000 && s.parse_slots == 10 && s.scratch_bytes == 0 && !s.d_poff;
                        }))
        return 1;
    // ensure_parse, growing: at least the request and half as much again as before
    if (fails_once_each("ensure_parse growing with scratch", 4, 0,
                        [] {
                            SlotBuffers s = plain(1000, 10, false);
                            s.ensure_parse(600, 4, 300, 0);
                            return s;
                        },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) {
                                s.ensure(1000, 10, false);
                                s.ensure_parse(600, 4, 300, 0);
                            }
                            s.ensure_parse(1100, 12, 300, 0);
                        },
                        [](const SlotBuffers& s) {
                            return s.parse_bytes == 1500 && s.parse_slots == 15 && s.scratch_bytes == 450;
                        }))
        return 1;
    if (fails_once_each("ensure_parse growing without scratch", 2, 16,
                        [] {
                            SlotBuffers s = plain(1000, 10, false);
                            s.ensure_parse(600, 4, 0, 16);
                            return s;
                        },
                        [](SlotBuffers& s) {
                            if (s.cap_bytes == 0) {
                                s.ensure(1000, 10, false);
                                s.ensure_parse(600, 4, 0, 16);
                            }
                            s.ensure_parse(4000, 4, 0, 16);
                        },
                        [](const SlotBuffers& s) {
                            return s.parse_bytes == 4000 && s.parse_slots == 15 && !s.d_scratch;
                        }))
        return 1;
    {  // a request that fits allocates nothing; more scratch alone grows the set
        g_what = "ensure_parse steady state";
        SlotBuffers s = plain(1000, 10, false);
        s.ensure_parse(600, 4, 300, 0);
        const uint64_t made0 = g_made;
        s.ensure_parse(1000, 10, 300, 0);
        s.ensure_parse(1, 1, 0, 16);
        CHECK(g_made == made0);
        s.ensure_parse(600, 4, 301, 0);
        CHECK(g_made == made0 + 4 && s.scratch_bytes == 450 && consistent(s, 0) == 0);
    }
    CHECK(g_live.empty() && g_bad_free == 0 && g_made == g_freed);
    // full: the whole set of a raw submit; a failure part-way leaves nothing behind
    {
        g_what = "full";
        const uint64_t made0 = g_made;
        {
            SlotBuffers s = SlotBuffers::full(1000, 10, 300);
            CHECK(g_made - made0 == 8 && g_live.size() == 8 && consistent(s, 0) == 0 && !s.h_qual);
            CHECK(s.cap_bytes == 1000 && s.cap_records == 10 && s.parse_bytes == 1000 && s.parse_slots == 10 &&
                  s.scratch_bytes == 300);
            SlotBuffers tiny = SlotBuffers::full(1, 0, 20);  // (the minimums)
            CHECK(tiny.cap_bytes == 64 && tiny.parse_bytes == 64 && tiny.cap_records == 2 && tiny.parse_slots == 2);
        }
        CHECK(g_live.empty());
        for (int64_t n = 1; n <= 8; ++n) {
            g_fail_in = n;
            bool threw = false;
            try {
                SlotBuffers s = SlotBuffers::full(1000, 10, 300);
            } catch (const speq_dev::OutOfDeviceMemory&) {
                threw = true;
            }
            CHECK(threw && g_live.empty());
            SlotBuffers again = SlotBuffers::full(1000, 10, 300);
            CHECK(consistent(again, 0) == 0 && g_live.size() == 8);
        }
    }
    CHECK(g_live.empty() && g_bad_free == 0 && g_made == g_freed);
    {  // a move into an empty set and into a full one: the source is empty, the target's old buffers are freed once
        g_what = "move";
        SlotBuffers a = SlotBuffers::full(1000, 10, 300);
        a.ensure(1000, 10, true);
        const auto was = fields(a);
        const uint64_t made0 = g_made, freed0 = g_freed;
        SlotBuffers b(std::move(a));
        CHECK(all_zero(a) && a.empty() && fields(b) == was && g_made == made0 && g_freed == freed0);
        SlotBuffers c;
        c = std::move(b);
        CHECK(all_zero(b) && fields(c) == was && g_freed == freed0 && consistent(c, 0) == 0);
        SlotBuffers d = plain(2000, 20, true);
        d.ensure_parse(100, 1, 0, 16);
        CHECK(g_live.size() == 10 + 8);
        d = std::move(c);
        CHECK(all_zero(c) && fields(d) == was && g_freed == freed0 + 8 && g_live.size() == 10 && consistent(d, 0) == 0);
        SlotBuffers& self = d;
        d = std::move(self);  // onto itself: nothing
        CHECK(fields(d) == was && g_live.size() == 10);
        a.ensure(100, 3, false);  // a moved-from set is an empty one
        CHECK(consistent(a, 0) == 0 && a.cap_bytes == 100);
        d.clear();
        CHECK(all_zero(d) && g_live.size() == 4);
    }
    CHECK(g_live.empty() && g_bad_free == 0 && g_made == g_freed);
    return 0;
}
}  // namespace

int main() {
    if (run()) return 1;
    std::printf("ok\n");
    return 0;
}
