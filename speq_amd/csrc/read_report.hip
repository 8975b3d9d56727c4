// Per-unit report (speq_report_reads_device / speq_report_reads): for every read, or pair, the number
// of passing, single-group and multi-group windows, the group of its first single-group window and the set of groups
// its windows are unique to. A diagnostic pass beside the scan kernels: every passing window gets an exact backward
// search (search_lds), no per-k structure is used, and nothing here is on the hot path of `speq scan`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "capi_internal.hpp"
#include "window_pass.hpp"

namespace {

using namespace speq_dev;

constexpr uint32_t NO_GROUP = 0xFFFFFFFFu;

// One wave64 owns one unit (a read, or the pair 2u, 2u + 1) and walks each mate in tiles of 64 window starts; lane j
// searches window tile + j (search_tile, window_pass.hpp) and ballots fold the lanes' results into the unit's record
// and group set. No other wave touches the unit's rows, so lane 0 writes them with plain loads and stores (the
// launcher cleared the set rows).
template <bool PAIRED>
__global__ __launch_bounds__(BLOCK_THREADS) void k_read_report(const DevView I, const uint8_t* __restrict__ seq,
                                                               const uint8_t* __restrict__ qual,
                                                               const uint64_t* __restrict__ off, uint64_t n_units,
                                                               uint32_t k, uint32_t cutoff, uint32_t W,
                                                               uint4* __restrict__ reports,
                                                               uint64_t* __restrict__ sets) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint16_t* cnt = wave_cnt(lds, wave, k);
    unsigned char* sym = wave_sym(lds, wave, k);
    const Rsrc R = make_rsrc(I);
    for (uint64_t u = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; u < n_units;
         u += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        uint32_t passing = 0, unique = 0, shared = 0, first = NO_GROUP;
        uint64_t* row = sets + u * W;
        for (uint32_t m = 0; m < (PAIRED ? 2u : 1u); ++m) {
            const uint64_t r = PAIRED ? 2u * u + m : u;
            const uint64_t beg = off[r], len = off[r + 1] - beg;
            if (len < k) continue;
            const uint64_t nwin = len - k + 1u;
            for (uint64_t tile = 0; tile < nwin; tile += 64u) {
                const uint32_t span = (uint32_t)min((uint64_t)(64u + k - 1u), len - tile);  // staged positions
                uint32_t lo = 0;
                bool pass;
                const int res = search_tile(I, R, sym, cnt, span, k, tile + lane < nwin, lane, lo,
                                            SPEQ_READ_TILE_AT(seq, qual, beg + tile, cutoff), &pass);
                const uint64_t b_uni = __ballot(res >= 0);
                passing += (uint32_t)__popcll(__ballot(pass));
                unique += (uint32_t)__popcll(b_uni);
                shared += (uint32_t)__popcll(__ballot(res == -2));
                if (b_uni != 0ull) {
                    if (first == NO_GROUP) first = (uint32_t)__shfl(res, __builtin_ctzll(b_uni));
                    uint64_t rest = b_uni;  // wave-uniform: one round per distinct group of the tile
                    while (rest != 0ull) {
                        const int g = __shfl(res, __builtin_ctzll(rest));
                        rest &= ~__ballot(res == g);
                        if (lane == 0 && (uint32_t)g < I.G) row[(uint32_t)g >> 6] |= 1ull << ((uint32_t)g & 63u);
                    }
                }
            }
        }
        if (lane == 0) reports[u] = make_uint4(passing, unique, shared, first);
    }
}

void check_params(const char* who, const speq_device_index* d, const speq_scan_params* p, uint64_t n_reads) {
    if (!p) throw std::invalid_argument(std::string(who) + ": null params");
    speq::check_report_k(who, p->k);
    if (p->paired && (n_reads & 1))
        throw std::invalid_argument(std::string(who) + ": paired report needs an even record count");
    if (!d) throw std::invalid_argument(std::string(who) + ": null device index");
}

void report_device_impl(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_offsets,
                        uint64_t n_reads, const speq_scan_params* p, speq_read_report* d_reports, uint64_t* d_sets,
                        hipStream_t st) {
    check_params("speq_report_reads_device", d, p, n_reads);
    const uint64_t n_units = p->paired ? n_reads / 2 : n_reads;
    if (n_units == 0) return;
    if (!d_seq || !d_qual || !d_offsets || !d_reports || !d_sets)
        throw std::invalid_argument("speq_report_reads_device: null buffer");
    if ((reinterpret_cast<uintptr_t>(d_reports) & 15u) || (reinterpret_cast<uintptr_t>(d_sets) & 7u))
        throw std::invalid_argument("speq_report_reads_device: reports must be 16-byte and sets 8-byte aligned");
    DeviceGuard g(d->device);
    const uint32_t W = (uint32_t)SPEQ_SET_WORDS(d->G);
    HIP_OK(hipMemsetAsync(d_sets, 0, n_units * W * sizeof(uint64_t), st));
    const DevView v = speq::search_view(d, p->k);
    const size_t lds = (size_t)WAVES_PER_BLOCK * wave_bytes(p->k);  // 13 KiB at k = 1024
    const uint64_t blocks = std::min<uint64_t>((n_units + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384u);
    uint4* rep = reinterpret_cast<uint4*>(d_reports);
    const auto kernel = p->paired ? k_read_report<true> : k_read_report<false>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(BLOCK_THREADS), lds, st, v, d_seq, d_qual, d_offsets, n_units,
                       p->k, p->phred_cutoff, W, rep, d_sets);
    HIP_OK(hipGetLastError());
}

void report_host_impl(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                      uint64_t n_reads, const speq_scan_params* p, speq_read_report* reports, uint64_t* sets) {
    const char* who = "speq_report_reads";
    check_params(who, d, p, n_reads);
    if (n_reads == 0) return;
    if (!offsets || !reports || !sets) throw std::invalid_argument("speq_report_reads: null argument");
    speq::check_host_reads(who, seq, qual, offsets, n_reads);
    const uint32_t per = p->paired ? 2u : 1u, W = (uint32_t)SPEQ_SET_WORDS(d->G);
    DeviceGuard g(d->device);
    const uint64_t most = std::min(n_reads, BATCH_RECORDS) / per;  // units of the largest batch
    // (for_staged_batches waits for its stream before it leaves, by a throw too: the two outlive every batch's work)
    const DevPtr<speq_read_report> drep = DevPtr<speq_read_report>::alloc(most, who);
    const DevPtr<uint64_t> dset = DevPtr<uint64_t>::alloc(most * W, who);
    const StagedPass pass = [&](const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint64_t r0,
                                uint64_t n) {  // (the results leave with the batch's one stream wait)
        const uint64_t units = n / per, u0 = r0 / per;
        report_device_impl(d, d_seq, d_qual, d_off, n, p, drep.get(), dset.get(), d->stream);
        HIP_OK(hipMemcpyAsync(reports + u0, drep.get(), units * sizeof(speq_read_report), hipMemcpyDeviceToHost,
                              d->stream));
        HIP_OK(hipMemcpyAsync(sets + u0 * W, dset.get(), units * W * 8, hipMemcpyDeviceToHost, d->stream));
    };
    for_staged_batches(who, d, seq, qual, offsets, n_reads, per, pass);
}

}  // namespace

static_assert(sizeof(speq_read_report) == 16, "speq_read_report is one 16-byte store");

extern "C" {

int speq_report_reads_device(speq_device_index* d, const uint8_t* d_seq, const uint8_t* d_qual,
                             const uint64_t* d_offsets, uint64_t n_reads, const speq_scan_params* params,
                             speq_read_report* d_reports, uint64_t* d_sets, void* stream) {
    return speq::guarded([&] {
        report_device_impl(d, d_seq, d_qual, d_offsets, n_reads, params, d_reports, d_sets,
                           static_cast<hipStream_t>(stream));
    });
}

int speq_report_reads(speq_device_index* d, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                      uint64_t n_reads, const speq_scan_params* params, speq_read_report* reports, uint64_t* sets) {
    return speq::guarded([&] { report_host_impl(d, seq, qual, offsets, n_reads, params, reports, sets); });
}

}  // extern "C"
