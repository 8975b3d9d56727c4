// What the host entry points do with a caller's read arrays before anything of the device is touched: the checks of
// {seq, qual, offsets} and the greedy cut into batches (speq_scan_reads, speq_report_reads, speq_markers_add_reads).
// Host-only: no HIP include (tests/host_reads_check.cpp is compiled with plain g++ and no ROCm include path).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "speq_scan.h"

namespace speq {

// End r1 of the batch [r0, r1) of whole units of `step` records (a read, or a pair; step divides n_reads - r0). The
// first unit is always taken, so a unit of more than max_bytes bases is a batch alone; then one unit at a time while
// the batch stays within max_records records and max_bytes bases. (r1 + step - r0 <= max_records is the
// r1 - r0 < max_records the pipeline had: the same when step divides max_records, as it does for every caller.)
inline uint64_t next_batch(const uint64_t* offsets, uint64_t n_reads, uint64_t r0, uint64_t step, uint64_t max_records,
                           uint64_t max_bytes) {
    uint64_t r1 = r0 + step;
    while (r1 < n_reads && r1 + step - r0 <= max_records && offsets[r1 + step] - offsets[r0] <= max_bytes) r1 += step;
    return r1;
}

// offsets[0 .. n_reads] non-decreasing, and buffers where there are bases (offsets non-null when n_reads > 0)
inline void check_host_reads(const char* who, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                             uint64_t n_reads) {
    if (n_reads == 0) return;
    for (uint64_t i = 0; i < n_reads; ++i)
        if (offsets[i + 1] < offsets[i]) throw std::invalid_argument(std::string(who) + ": offsets must be non-decreasing");
    if (offsets[n_reads] > offsets[0] && (!seq || !qual))
        throw std::invalid_argument(std::string(who) + ": null read buffer");
}

// the k of the window passes beside the scan (per-unit report, marker coverage)
inline void check_report_k(const char* who, uint32_t k) {
    if (k < 1 || k > SPEQ_REPORT_MAX_K)
        throw std::invalid_argument(std::string(who) + ": k must be in [1, " + std::to_string(SPEQ_REPORT_MAX_K) + "]");
}

// the bin width of the marker track
inline void check_track_bin(const char* who, uint32_t bin) {
    if (bin < 1 || bin > SPEQ_TRACK_MAX_BIN)
        throw std::invalid_argument(std::string(who) + ": bin must be in [1, " + std::to_string(SPEQ_TRACK_MAX_BIN) + "]");
}

}  // namespace speq
