// What the diagnostic window passes beside the scan kernels share (per-unit report, read_report.hip, DESIGN.md §4n;
// marker coverage, read_markers.hip, §4o; marker track, marker_track.hip, §4t): every passing window of a tile of 64
// window starts gets an exact backward search, and host reads reach the device in staged batches. Each pass keeps its
// kernels in its own translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "device_index.hpp"
#include "host_reads.hpp"
#include "scan_device.hpp"

namespace speq_dev {

// Per-wave LDS: u16 prefix counts of bad positions [64 + k] | symbol codes [64 + k - 1], rounded to 16 B.
__host__ __device__ inline uint32_t wave_bytes(uint32_t k) { return (3u * (64u + k) + 15u) & ~15u; }
__device__ __forceinline__ uint16_t* wave_cnt(unsigned char* lds, uint32_t wave, uint32_t k) {
    return reinterpret_cast<uint16_t*>(lds + wave * wave_bytes(k));
}
__device__ __forceinline__ unsigned char* wave_sym(unsigned char* lds, uint32_t wave, uint32_t k) {
    return lds + wave * wave_bytes(k) + 2u * (64u + k);
}

// One tile of 64 window starts over `span` staged positions (span <= 64 + k - 1): at(p) gives position p's symbol
// code (0..3, or 4 for anything that ends a window) and whether it is bad; the wave's region then holds each symbol
// and the number of bad positions before it, so window j passes iff cnt[j + k] == cnt[j]. Lane j searches window j
// (has: window j exists; then j + k <= span) and returns the search's result with the interval start in `lo`;
// `passed`, where given, gets whether the lane's window passed the filter.
template <class At>
__device__ __forceinline__ int search_tile(const DevView& I, const Rsrc& R, unsigned char* sym, uint16_t* cnt,
                                           uint32_t span, uint32_t k, bool has, uint32_t lane, uint32_t& lo, At&& at,
                                           bool* passed = nullptr) {
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t bad_before = 0;
    for (uint32_t c = 0; c < span; c += 64u) {
        const uint32_t p = c + lane;
        const bool valid = p < span;
        uint32_t s = 4u;
        bool bad = false;
        if (valid) at(p, s, bad);
        const uint64_t bal = __ballot(bad);
        if (valid) {
            sym[p] = (unsigned char)s;
            cnt[p] = (uint16_t)(bad_before + (uint32_t)__popcll(bal & below));
        }
        bad_before += (uint32_t)__popcll(bal);
    }
    if (lane == 0) cnt[span] = (uint16_t)bad_before;
    wave_sync();
    const bool pass = has && cnt[lane + k] == cnt[lane];
    int res = -1;
    if (pass) {
        uint32_t hi;
        res = search_lds(I, R, sym + lane, k, true, lo, hi);
    }
    wave_sync();  // the next tile restages this wave's region
    if (passed) *passed = pass;
    return res;
}

// search_tile's at() over ASCII reads whose tile starts at position `first` of seq / qual: the scan's read filter (dna5
// symbol; bad when N, or when the Phred quality clamped to 0..41 is <= cutoff). A macro that pastes the lambda into the
// kernel: as a functor or a function, in four forms tried, k_marker_reads compiled to other code than it had (in one
// form two VGPRs more, in another measured 0.4 % slower); pasted, it is that code byte for byte.
#define SPEQ_READ_TILE_AT(seq, qual, first, cutoff)                      \
    [&](uint32_t p, uint32_t& s, bool& bad) {                            \
        const uint64_t at = (first) + p;                                 \
        s = ascii_sym((seq)[at]);                                        \
        const int32_t q = min(max((int32_t)(qual)[at] - 33, 0), 41);     \
        bad = s == 4u || (uint32_t)q <= (cutoff);                        \
    }

// Host reads (checked: speq::check_host_reads) through a pass in batches of whole units: at most BATCH_RECORDS records
// and (a single longer unit aside) BATCH_BYTES bases each. Bases, qualities and the offsets rebased to 0 are staged in
// device buffers, pass(d_seq, d_qual, d_offsets, r0, n) issues its work for the n records from r0 on d->stream, and
// the stream is synchronised once per batch: what a pass allocates must outlive that wait (its return is too early).
// One staged pass at a time per process: the batches go through the replica's stream and wait for it.
constexpr uint64_t BATCH_RECORDS = 1ull << 20, BATCH_BYTES = 256ull << 20;
using StagedPass = std::function<void(const uint8_t*, const uint8_t*, const uint64_t*, uint64_t, uint64_t)>;
inline void for_staged_batches(const char* who, speq_device_index* d, const uint8_t* seq, const uint8_t* qual,
                               const uint64_t* offsets, uint64_t n_reads, uint32_t step, const StagedPass& pass) {
    static std::mutex mu;
    std::lock_guard<std::mutex> lk(mu);
    std::vector<uint64_t> rel;
    for (uint64_t r0 = 0; r0 < n_reads;) {
        const uint64_t r1 = speq::next_batch(offsets, n_reads, r0, step, BATCH_RECORDS, BATCH_BYTES);
        const uint64_t n = r1 - r0, bytes = offsets[r1] - offsets[r0];
        rel.resize(n + 1);
        for (uint64_t i = 0; i <= n; ++i) rel[i] = offsets[r0 + i] - offsets[r0];
        const DevPtr<uint8_t> ds = DevPtr<uint8_t>::alloc(bytes, who), dq = DevPtr<uint8_t>::alloc(bytes, who);
        const DevPtr<uint64_t> dof = DevPtr<uint64_t>::alloc(n + 1, who);
        SyncOnExit sync(d->stream);
        if (bytes) {
            HIP_OK(hipMemcpyAsync(ds.get(), seq + offsets[r0], bytes, hipMemcpyHostToDevice, d->stream));
            HIP_OK(hipMemcpyAsync(dq.get(), qual + offsets[r0], bytes, hipMemcpyHostToDevice, d->stream));
        }
        HIP_OK(hipMemcpyAsync(dof.get(), rel.data(), (n + 1) * 8, hipMemcpyHostToDevice, d->stream));
        pass(ds.get(), dq.get(), dof.get(), r0, n);
        HIP_OK(hipStreamSynchronize(d->stream));
        r0 = r1;
    }
}

}  // namespace speq_dev
