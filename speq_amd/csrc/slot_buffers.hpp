// The buffers of one pipeline slot, and of one set reserved ahead of a FASTQ stream, as one owner. Host-only, no HIP
// include: written against dev_mem.hpp's seam and a second one for page-locked host memory, so
// tests/slot_buffers_check.cpp runs it over malloc. pipeline.cpp does not use it yet: it still keeps a slot's buffers
// as raw pointers with its own allocation and cleanup paths, and the library does not define the pinned seam.
//
// Invariant: after any call that throws, the set is either exactly as it was or empty with every capacity 0. A pointer
// is never set beside a capacity that does not describe it, and a host buffer never exists without its device twin.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "dev_mem.hpp"

namespace speq_dev {

// How a page-locked host buffer was obtained, which is how it has to be released.
enum class PinnedHow : uint8_t { registered, host_malloc };
struct PinnedMem {
    void* p = nullptr;
    PinnedHow how = PinnedHow::registered;
};

namespace mem {
// `bytes` of page-locked host memory, or throws (std::bad_alloc, speq::DeviceError). Not a device allocation: neither
// counted by speq_debug_allocs nor failed by speq_debug_fail_alloc.
PinnedMem pinned_alloc(size_t bytes, const char* who);
void pinned_free(void* p, PinnedHow how) noexcept;  // null: nothing
}  // namespace mem

// Move-only owner of one page-locked host allocation: the pointer, and how it was obtained.
template <class T>
class PinnedPtr {
    T* p_ = nullptr;
    PinnedHow how_ = PinnedHow::registered;

public:
    PinnedPtr() = default;
    static PinnedPtr alloc(size_t count, const char* who) {
        const PinnedMem m = mem::pinned_alloc(count * sizeof(T), who);
        PinnedPtr r;
        r.p_ = static_cast<T*>(m.p);
        r.how_ = m.how;
        return r;
    }
    PinnedPtr(PinnedPtr&& o) noexcept : p_(std::exchange(o.p_, nullptr)), how_(o.how_) {}
    PinnedPtr& operator=(PinnedPtr&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            how_ = o.how_;
        }
        return *this;
    }
    PinnedPtr(const PinnedPtr&) = delete;
    PinnedPtr& operator=(const PinnedPtr&) = delete;
    ~PinnedPtr() { reset(); }

    T* get() const { return p_; }
    void reset() { mem::pinned_free(std::exchange(p_, nullptr), how_); }
    explicit operator bool() const { return p_ != nullptr; }
};

struct SlotFields {  // (its own moves move the pointers and copy the capacities: SlotBuffers zeroes the source's)
    // what a producer fills (page-locked) and where it is copied to: cap_bytes of text (d_seq: + 64, the GPU parser
    // reads 16-B windows), cap_records + 1 offsets; qualities only when asked for: raw-text submits (GPU FASTQ
    // parsing) use the base buffer alone, which halves the pinned memory of a FASTQ stream
    PinnedPtr<uint8_t> h_seq, h_qual;
    PinnedPtr<uint64_t> h_off;
    DevPtr<uint8_t> d_seq, d_qual;
    DevPtr<uint64_t> d_off;
    uint64_t cap_bytes = 0, cap_records = 0;
    // raw and packed submits: parsed or unpacked bases and qualities (parse_bytes each), and for raw submits
    // parse_slots + 1 offsets and the parser's scratch; allocated on first use
    DevPtr<uint8_t> d_pseq, d_pqual;
    DevPtr<uint64_t> d_poff;
    DevPtr<> d_scratch;
    uint64_t parse_bytes = 0, parse_slots = 0;
    size_t scratch_bytes = 0;
};

struct SlotBuffers : SlotFields {
    SlotBuffers() = default;
    SlotBuffers(SlotBuffers&& o) noexcept : SlotFields(std::move(o)) { o.clear(); }
    SlotBuffers& operator=(SlotBuffers&& o) noexcept {  // frees what it held; o is empty afterwards
        if (this != &o) {
            SlotFields::operator=(std::move(o));
            o.clear();
        }
        return *this;
    }
    ~SlotBuffers() { clear(); }  // (host buffers, their device twins, then the parse set: the order of clear())

    bool empty() const { return !h_seq && !d_pseq; }

    void clear() {
        clear_io();
        clear_parse();
    }

    // Grows the set to at least (bytes, records), and adds qualities when asked for; a set that has them keeps them.
    // Frees first and allocates then, so the old and the new buffers are never alive together.
    void ensure(uint64_t bytes, uint64_t records, bool qual) {
        bytes = std::max<uint64_t>(bytes, 64);
        records = std::max<uint64_t>(records, 2);
        const bool grow = bytes > cap_bytes || records > cap_records;
        try {
            if (grow) {
                bytes = std::max(bytes, cap_bytes);
                records = std::max(records, cap_records);
                qual = qual || h_qual;
                clear_io();
                h_seq = PinnedPtr<uint8_t>::alloc(bytes, "slot text");
                h_off = PinnedPtr<uint64_t>::alloc(records + 1, "slot offsets");
                d_seq = DevPtr<uint8_t>::alloc(bytes + 64, "slot text");
                d_off = DevPtr<uint64_t>::alloc(records + 1, "slot offsets");
                cap_bytes = bytes;
                cap_records = records;
            }
            if (qual && !h_qual) {  // both halves, then both in
                PinnedPtr<uint8_t> h = PinnedPtr<uint8_t>::alloc(cap_bytes, "slot qualities");
                DevPtr<uint8_t> d = DevPtr<uint8_t>::alloc(cap_bytes, "slot qualities");
                h_qual = std::move(h);
                d_qual = std::move(d);
            }
        } catch (...) {
            if (grow) clear();  // (qualities alone: nothing was touched)
            throw;
        }
    }

    // The parse buffers of a raw (scratch > 0) or packed (scratch == 0: neither offsets nor scratch) submit of `bytes`
    // bases in `slots` records. freeing device memory waits for the whole device, so a set that has to grow sizes for
    // the slot's capacity and by half, which keeps reallocation out of the steady state. scratch_for(bytes, slots):
    // the scratch that a submit of the grown size would ask for. pad: bytes past the end that the unpack kernels write.
    template <class ScratchFor>
    void ensure_parse(uint64_t bytes, uint64_t slots, size_t scratch, uint64_t pad, ScratchFor&& scratch_for) {
        if (bytes <= parse_bytes && slots <= parse_slots && scratch <= scratch_bytes) return;
        const uint64_t pb = std::max({bytes, parse_bytes * 3 / 2, cap_bytes});
        const uint64_t ps = std::max({slots, parse_slots * 3 / 2, cap_records});
        const size_t sb = scratch ? std::max({scratch, scratch_bytes * 3 / 2, (size_t)scratch_for(pb, ps)}) : 0;
        clear_parse();
        try {
            d_pseq = DevPtr<uint8_t>::alloc(pb + pad, "slot parsed bases");
            d_pqual = DevPtr<uint8_t>::alloc(pb + pad, "slot parsed qualities");
            if (sb) {
                d_poff = DevPtr<uint64_t>::alloc(ps + 1, "slot parsed offsets");
                d_scratch = DevPtr<>::alloc(sb, "slot parse scratch");
            }
            parse_bytes = pb;
            parse_slots = ps;
            scratch_bytes = sb;
        } catch (...) {
            clear();
            throw;
        }
    }
    void ensure_parse(uint64_t bytes, uint64_t slots, size_t scratch, uint64_t pad) {
        ensure_parse(bytes, slots, scratch, pad, [](uint64_t, uint64_t) { return size_t(0); });
    }

    // A whole set for raw submits of up to (bytes, records): what is reserved ahead of a FASTQ stream.
    static SlotBuffers full(uint64_t bytes, uint64_t records, size_t scratch) {
        SlotBuffers s;  // (destroyed with whatever it holds when an allocation throws)
        s.ensure(bytes, records, false);
        s.ensure_parse(s.cap_bytes, s.cap_records, scratch, 0);
        return s;
    }

private:
    void clear_io() {
        h_seq.reset();
        h_qual.reset();
        h_off.reset();
        d_seq.reset();
        d_qual.reset();
        d_off.reset();
        cap_bytes = cap_records = 0;
    }
    void clear_parse() {
        d_pseq.reset();
        d_pqual.reset();
        d_poff.reset();
        d_scratch.reset();
        parse_bytes = parse_slots = 0;
        scratch_bytes = 0;
    }
};

}  // namespace speq_dev
