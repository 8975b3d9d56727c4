// The marker handle (speq_markers, opaque in include/speq_scan.h) that the marker passes share: coverage per group
// (read_markers.hip) and the per-record track (marker_track.hip, §4t); and the track's bin layout, a
// host-only function of text_start.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "device_index.hpp"
#include "speq_scan.h"

struct speq_markers {
    speq_device_index* dev = nullptr;
    speq_scan_params params{};  // k and phred_cutoff, fixed at create
    uint64_t n = 0;             // SA positions
    uint32_t G = 0;
    speq_dev::DevPtr<uint32_t> d_depth;  // [n]: MARK | depth
};

namespace speq_dev {
constexpr uint32_t MARK = 0x80000000u;  // bit 31 of a depth word: the position starts a marker's interval
}

namespace speq {

// Loci of record r at scan length k: the window starts of fwd_r, text 2r of text_start[2R + 1] (a text's span ends with
// its separator).
inline uint64_t track_loci(const uint64_t* text_start, uint32_t r, uint32_t k) {
    const uint64_t L = text_start[2u * r + 1u] - text_start[2u * r] - 1u;
    return L >= k ? L - k + 1u : 0u;
}

// first_bin[R + 1] (may be null): the prefix of ceil(loci / bin) per record; returns first_bin[R].
inline uint64_t track_layout(const uint64_t* text_start, uint32_t R, uint32_t k, uint32_t bin, uint64_t* first_bin) {
    uint64_t at = 0;
    for (uint32_t r = 0; r < R; ++r) {
        if (first_bin) first_bin[r] = at;
        at += (track_loci(text_start, r, k) + bin - 1u) / bin;
    }
    if (first_bin) first_bin[R] = at;
    return at;
}

}  // namespace speq
