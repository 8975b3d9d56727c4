// Marker track (speq_markers_track*): where along each record the reads cover its markers. A locus is a
// window start of a forward text; a marker locus is one whose k-mer is a marker (the MARK bit at its interval start,
// read_markers.hip), and its depth is the k-mer's depth plus that of its reverse complement (once when the two are one
// k-mer). One pass over the forward texts reads the handle's depth words and folds the loci into bins of `bin` loci per
// record. A diagnostic pass beside the scan, run once per call; it writes only its own output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "markers_handle.hpp"
#include "window_pass.hpp"

namespace {

using namespace speq_dev;

constexpr uint32_t NONE = 0xFFFFFFFFu;               // no single-group interval
constexpr uint32_t BIN_WORDS = sizeof(speq_marker_bin) / 8;

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d));
    return v;
}

// One wave64 per tile of 64 loci of one record (tile_first[R + 1]: the prefix of tiles per forward text, so a tile
// never crosses a record's end). Lane j searches window p0 + j of the staged span, then the same span read backwards
// and complemented, where lane j holds the reverse complement of window p0 + (nw - 1 - j): one shuffle by the tile's
// own window count brings a locus's two interval starts into one lane. Equal starts are one k-mer, counted once.
// WIDE (bin >= 64): a tile touches at most two bins; ballots, a wave sum and a wave max, then lane 0's no-return
// atomics per touched bin. Else every marker lane adds to its own bin.
template <bool WIDE>
__global__ __launch_bounds__(BLOCK_THREADS) void k_marker_track(const DevView I, const uint8_t* __restrict__ text,
                                                                const uint64_t* __restrict__ text_start,
                                                                const uint32_t* __restrict__ tile_first,
                                                                const uint64_t* __restrict__ first_bin, uint32_t n_rec,
                                                                uint32_t k, uint32_t bin,
                                                                const uint32_t* __restrict__ depth,
                                                                unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint16_t* cnt = wave_cnt(lds, wave, k);
    unsigned char* sym = wave_sym(lds, wave, k);
    const Rsrc R = make_rsrc(I);
    const uint32_t n_tiles = tile_first[n_rec];
    for (uint32_t tv = blockIdx.x * WAVES_PER_BLOCK + wave; tv < n_tiles; tv += gridDim.x * WAVES_PER_BLOCK) {
        const uint32_t t = __builtin_amdgcn_readfirstlane(tv);
        uint32_t r = 0, r_hi = n_rec;  // the last record with tile_first[r] <= t: the one that owns tile t
        while (r_hi - r > 1u) {
            const uint32_t mid = (r + r_hi) >> 1;
            if (tile_first[mid] <= t) r = mid;
            else r_hi = mid;
        }
        const uint64_t base = text_start[2u * r];
        const uint32_t nwin = (uint32_t)(text_start[2u * r + 1u] - base) - k;  // L - k + 1, the separator taken off
        const uint32_t p0 = (t - tile_first[r]) * 64u;
        const uint32_t nw = min(64u, nwin - p0), span = nw + k - 1u;
        const uint8_t* src = text + base + p0;
        uint32_t lo_f = NONE, lo_r = NONE;
#pragma nounroll
        for (uint32_t pass = 0; pass < 2u; ++pass) {
            uint32_t lo = 0;
            const int res = search_tile(I, R, sym, cnt, span, k, lane < nw, lane, lo,
                                        [&](uint32_t p, uint32_t& s, bool& bad) {
                                            const uint32_t c = src[pass ? span - 1u - p : p];
                                            bad = c < 2u || c > 5u;
                                            s = bad ? 4u : (pass ? 5u - c : c - 2u);
                                        });
            const uint32_t v = (res >= 0 && lo < I.n) ? lo : NONE;
            if (pass) lo_r = v;
            else lo_f = v;
        }
        lo_r = (uint32_t)__shfl((int)lo_r, (int)((nw - 1u - lane) & 63u));
        bool mk = false;
        uint32_t d = 0;  // < 2^32: two depths below 2^31
        if (lo_f != NONE) {
            const uint32_t w = depth[lo_f];
            mk = (w & MARK) != 0u;
            d = w & ~MARK;
            if (mk && lo_r != NONE && lo_r != lo_f) d += depth[lo_r] & ~MARK;
        }
        const uint64_t row0 = first_bin[r];
        if (WIDE) {
            const uint32_t b0 = p0 / bin, edge = (b0 + 1u) * bin - p0;  // the lanes below `edge` lie in bin b0
            for (uint32_t h = 0; h < 2u; ++h) {
                if (h && edge >= nw) break;
                const bool in = mk && ((lane < edge) == (h == 0u));
                const uint64_t bm = __ballot(in);
                if (!bm) continue;
                const uint64_t bo = __ballot(in && d != 0u);
                const unsigned long long hs = wave_sum<unsigned long long>(in ? d : 0u);
                const uint32_t mx = wave_max(in ? d : 0u);
                if (lane == 0) {
                    unsigned long long* o = out + (row0 + b0 + h) * BIN_WORDS;
                    atomicAdd(&o[0], (unsigned long long)__popcll(bm));
                    if (bo) {
                        atomicAdd(&o[1], (unsigned long long)__popcll(bo));
                        atomicAdd(&o[2], hs);
                        atomicMax(&o[3], (unsigned long long)mx);
                    }
                }
            }
        } else if (mk) {
            unsigned long long* o = out + (row0 + (p0 + lane) / bin) * BIN_WORDS;
            atomicAdd(&o[0], 1ull);
            if (d) {
                atomicAdd(&o[1], 1ull);
                atomicAdd(&o[2], (unsigned long long)d);
                atomicMax(&o[3], (unsigned long long)d);
            }
        }
    }
}

uint32_t records_of(const speq_device_index* d) { return d->n_texts / 2u; }

void layout_impl(const speq_markers* m, uint32_t bin, uint64_t* n_bins, uint64_t* first_bin) {
    const char* who = "speq_markers_track_layout";
    if (!m) throw std::invalid_argument(std::string(who) + ": null handle");
    speq::check_track_bin(who, bin);
    const uint64_t nb = speq::track_layout(m->dev->text_start.data(), records_of(m->dev), m->params.k, bin, first_bin);
    if (n_bins) *n_bins = nb;
}

void track_impl(speq_markers* m, uint32_t bin, speq_marker_bin* out) {
    const char* who = "speq_markers_track";
    if (!m) throw std::invalid_argument(std::string(who) + ": null handle");
    if (!out) throw std::invalid_argument(std::string(who) + ": null output");
    speq::check_track_bin(who, bin);
    speq_device_index* d = m->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());  // the adds of every stream of the device have completed
    const uint32_t n_rec = records_of(d), k = m->params.k;
    const uint64_t* ts = d->text_start.data();
    std::vector<uint64_t> first_bin(n_rec + 1u);
    std::vector<uint32_t> tile_first(n_rec + 1u);
    const uint64_t n_bins = speq::track_layout(ts, n_rec, k, bin, first_bin.data());
    uint32_t tiles = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        tile_first[r] = tiles;
        tiles += (uint32_t)((speq::track_loci(ts, r, k) + 63u) / 64u);
    }
    tile_first[n_rec] = tiles;
    if (n_bins == 0) return;  // (then no record has a window, and there is no tile either)
    const DevPtr<> bins = DevPtr<>::alloc(n_bins * sizeof(speq_marker_bin), who);
    const DevPtr<uint64_t> d_first = dev_upload(first_bin);
    const DevPtr<uint32_t> d_tiles = dev_upload(tile_first);
    hipStream_t st = d->stream;
    SyncOnExit sync(st);
    HIP_OK(hipMemsetAsync(bins.get(), 0, n_bins * sizeof(speq_marker_bin), st));
    const DevView v = speq::search_view(d, k);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384u);
    const size_t lds = (size_t)WAVES_PER_BLOCK * wave_bytes(k);
    auto* o = static_cast<unsigned long long*>(bins.get());
    if (bin >= 64u)
        hipLaunchKernelGGL(k_marker_track<true>, dim3(blocks), dim3(BLOCK_THREADS), lds, st, v, d->d_text,
                           d->d_text_start, d_tiles.get(), d_first.get(), n_rec, k, bin, m->d_depth.get(), o);
    else
        hipLaunchKernelGGL(k_marker_track<false>, dim3(blocks), dim3(BLOCK_THREADS), lds, st, v, d->d_text,
                           d->d_text_start, d_tiles.get(), d_first.get(), n_rec, k, bin, m->d_depth.get(), o);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, bins.get(), n_bins * sizeof(speq_marker_bin), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
}

}  // namespace

static_assert(sizeof(speq_marker_bin) == 32, "speq_marker_bin is four u64 words");

extern "C" {

int speq_markers_track_layout(const speq_markers* m, uint32_t bin, uint64_t* n_bins, uint64_t* first_bin) {
    return speq::guarded([&] { layout_impl(m, bin, n_bins, first_bin); });
}

int speq_index_track_layout(const speq_index* idx, uint32_t k, uint32_t bin, uint64_t* n_bins, uint64_t* first_bin) {
    return speq::guarded([&] {
        const char* who = "speq_index_track_layout";
        if (!idx) throw std::invalid_argument(std::string(who) + ": null index");
        speq::check_report_k(who, k);
        speq::check_track_bin(who, bin);
        const uint64_t nb = speq::track_layout(idx->fm.text_start.data(), idx->fm.n_records, k, bin, first_bin);
        if (n_bins) *n_bins = nb;
    });
}

int speq_markers_track(speq_markers* m, uint32_t bin, speq_marker_bin* out) {
    return speq::guarded_nomem([&] { track_impl(m, bin, out); });
}

}  // extern "C"
