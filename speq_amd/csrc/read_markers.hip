// Marker coverage (speq_markers_*): how many of each group's markers the reads cover, and how deep. A
// marker of group g is a distinct N-free k-mer of the indexed texts whose occurrences all lie in texts of g; it is
// named by the start `lo` of its SA interval. The handle keeps one u32 per SA position: bit 31 marks a marker (set by
// one pass over the texts at create), bits 0..30 count the passing read windows equal to it. A diagnostic pass beside
// the scan kernels, shaped like the per-unit report (read_report.hip): every passing window gets an exact backward
// search (search_lds), no per-k structure is used, and nothing here is on the hot path of `speq scan`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_internal.hpp"
#include "markers_handle.hpp"
#include "window_pass.hpp"

namespace {

using namespace speq_dev;

constexpr uint32_t LDS_TALLY_GROUPS = 512u;   // the fold tallies in LDS up to this many groups (26 KiB), else in HBM
constexpr uint32_t COV_WORDS = sizeof(speq_marker_cov) / 8;  // u64 words of one group's record
// per-block tally of the fold, per group: u64 hits, then u32 {markers, observed, max_depth, bins[8]}
constexpr uint32_t TALLY_U32 = 3u + SPEQ_MARKER_BINS;
__host__ __device__ inline uint32_t tally_bytes(uint32_t G) { return G * (8u + 4u * TALLY_U32); }

// Read pass: one wave64 per read, tiles of 64 window starts. A window whose k-mer lies in one group adds 1 to the
// depth word at its interval start: a no-return atomic, one per lane (adjacent windows have different starts).
__global__ __launch_bounds__(BLOCK_THREADS) void k_marker_reads(const DevView I, const uint8_t* __restrict__ seq,
                                                                const uint8_t* __restrict__ qual,
                                                                const uint64_t* __restrict__ off, uint64_t n_reads,
                                                                uint32_t k, uint32_t cutoff,
                                                                uint32_t* __restrict__ depth) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint16_t* cnt = wave_cnt(lds, wave, k);
    unsigned char* sym = wave_sym(lds, wave, k);
    const Rsrc R = make_rsrc(I);
    for (uint64_t r = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave; r < n_reads;
         r += (uint64_t)gridDim.x * WAVES_PER_BLOCK) {
        const uint64_t beg = off[r], len = off[r + 1] - beg;
        if (len < k) continue;
        const uint64_t nwin = len - k + 1u;
        for (uint64_t tile = 0; tile < nwin; tile += 64u) {
            const uint32_t span = (uint32_t)min((uint64_t)(64u + k - 1u), len - tile);
            uint32_t lo = 0;
            const int res = search_tile(I, R, sym, cnt, span, k, tile + lane < nwin, lane, lo,
                                        SPEQ_READ_TILE_AT(seq, qual, beg + tile, cutoff));
            if (res >= 0 && lo < I.n) atomicAdd(&depth[lo], 1u);
        }
    }
}

// Marker pass: the same search over every window of the FM text (SA-alphabet codes: A..T = 2..5; separators, the
// terminator and N end a window, so a window of A, C, G, T only lies wholly inside one text). One wave per tile of 64
// text positions; a single-group result marks its interval start.
__global__ __launch_bounds__(BLOCK_THREADS) void k_marker_texts(const DevView I, const uint8_t* __restrict__ text,
                                                                uint32_t k, uint32_t* __restrict__ depth) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint16_t* cnt = wave_cnt(lds, wave, k);
    unsigned char* sym = wave_sym(lds, wave, k);
    const Rsrc R = make_rsrc(I);
    const uint64_t n = I.n;
    if (n < k) return;
    const uint64_t nwin = n - k + 1u;
    for (uint64_t tile = ((uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave) * 64u; tile < nwin;
         tile += (uint64_t)gridDim.x * WAVES_PER_BLOCK * 64u) {
        const uint32_t span = (uint32_t)min((uint64_t)(64u + k - 1u), n - tile);
        uint32_t lo = 0;
        const int res = search_tile(I, R, sym, cnt, span, k, tile + lane < nwin, lane, lo,
                                    [&](uint32_t p, uint32_t& s, bool& bad) {
                                        const uint32_t c = text[tile + p];
                                        bad = c < 2u || c > 5u;
                                        s = bad ? 4u : c - 2u;
                                    });
        if (res >= 0 && lo < I.n) atomicOr(&depth[lo], MARK);
    }
}

__device__ __forceinline__ uint32_t depth_bin(uint32_t dp) { return min(dp, (uint32_t)SPEQ_MARKER_BINS - 1u); }

// Fold: grid-stride over SA positions; a marked position's group is that of the one-position interval [i, i + 1).
// LDS_TALLY: the block tallies in LDS and flushes its non-zero words once; else every marker goes to HBM atomics.
template <bool LDS_TALLY>
__global__ __launch_bounds__(256) void k_marker_fold(const DevView I, const uint32_t* __restrict__ depth,
                                                     unsigned long long* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t G = I.G;
    unsigned long long* t_hits = reinterpret_cast<unsigned long long*>(lds);
    uint32_t* t_w = reinterpret_cast<uint32_t*>(lds + 8u * (LDS_TALLY ? G : 0u));
    if (LDS_TALLY) {
        for (uint32_t i = threadIdx.x; i < G; i += blockDim.x) t_hits[i] = 0ull;
        for (uint32_t i = threadIdx.x; i < G * TALLY_U32; i += blockDim.x) t_w[i] = 0u;
        __syncthreads();
    }
    const Rsrc R = make_rsrc(I);
    const uint64_t n = I.n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t w = depth[i];
        if (!(w & MARK)) continue;
        const int g = classify(I, R, (uint32_t)i, (uint32_t)i + 1u);
        if (g < 0 || (uint32_t)g >= G) continue;
        const uint32_t dp = w & ~MARK;
        if (LDS_TALLY) {
            uint32_t* t = t_w + (uint32_t)g * TALLY_U32;
            atomicAdd(&t[0], 1u);
            if (dp) {
                atomicAdd(&t[1], 1u);
                atomicMax(&t[2], dp);
                atomicAdd(&t_hits[g], (unsigned long long)dp);
            }
            atomicAdd(&t[3u + depth_bin(dp)], 1u);
        } else {
            unsigned long long* o = out + (uint64_t)g * COV_WORDS;
            atomicAdd(&o[0], 1ull);
            if (dp) {
                atomicAdd(&o[1], 1ull);
                atomicAdd(&o[2], (unsigned long long)dp);
                atomicMax(&o[3], (unsigned long long)dp);
            }
            atomicAdd(&o[4u + depth_bin(dp)], 1ull);
        }
    }
    if (LDS_TALLY) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < G * TALLY_U32; i += blockDim.x) {
            const uint32_t v = t_w[i];
            if (!v) continue;
            const uint32_t g = i / TALLY_U32, f = i - g * TALLY_U32;
            unsigned long long* o = out + (uint64_t)g * COV_WORDS;
            if (f == 2u) atomicMax(&o[3], (unsigned long long)v);
            else atomicAdd(&o[f < 2u ? f : f + 1u], (unsigned long long)v);  // markers, observed | bins at 4..
        }
        for (uint32_t g = threadIdx.x; g < G; g += blockDim.x)
            if (t_hits[g]) atomicAdd(&out[(uint64_t)g * COV_WORDS + 2u], t_hits[g]);
    }
}

// speq_markers_list: the group of every marked position (0xFFFFFFFF elsewhere)
__global__ __launch_bounds__(256) void k_marker_groups(const DevView I, const uint32_t* __restrict__ depth,
                                                       uint32_t* __restrict__ group) {
    const Rsrc R = make_rsrc(I);
    const uint64_t n = I.n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        group[i] = (depth[i] & MARK) ? (uint32_t)classify(I, R, (uint32_t)i, (uint32_t)i + 1u) : 0xFFFFFFFFu;
}

void check_create(const speq_device_index* d, const speq_scan_params* p, speq_markers** out) {
    const char* who = "speq_markers_create";
    if (!p) throw std::invalid_argument(std::string(who) + ": null params");
    speq::check_report_k(who, p->k);
    if (!d) throw std::invalid_argument(std::string(who) + ": null device index");
    if (!out) throw std::invalid_argument(std::string(who) + ": null output");
}

uint32_t grid_1d(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 16384u)); }

void create_impl(speq_device_index* d, const speq_scan_params* p, speq_markers** out) {
    check_create(d, p, out);
    DeviceGuard g(d->device);
    auto m = std::make_unique<speq_markers>();
    m->dev = d;
    m->params = *p;
    m->n = d->view.n;
    m->G = d->G;
    m->d_depth = DevPtr<uint32_t>::alloc(m->n, "speq_markers_create");
    hipStream_t st = d->stream;
    SyncOnExit sync(st);  // (declared after m: the stream is idle before a throw frees the handle's array)
    HIP_OK(hipMemsetAsync(m->d_depth.get(), 0, m->n * 4, st));
    const DevView v = speq::search_view(d, p->k);
    const uint64_t tiles = m->n >= p->k ? (m->n - p->k + 1 + 63) / 64 : 0;
    if (tiles) {
        const uint64_t blocks = std::min<uint64_t>((tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384u);
        hipLaunchKernelGGL(k_marker_texts, dim3((uint32_t)blocks), dim3(BLOCK_THREADS),
                           (size_t)WAVES_PER_BLOCK * wave_bytes(p->k), st, v, d->d_text, p->k, m->d_depth.get());
        HIP_OK(hipGetLastError());
    }
    // the adds come on the callers' streams: the marks are complete before the handle exists
    HIP_OK(hipStreamSynchronize(st));
    *out = m.release();
}

void add_device_impl(speq_markers* m, const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_offsets,
                     uint64_t n_reads, hipStream_t st) {
    if (n_reads > 0 && (!d_seq || !d_qual || !d_offsets))
        throw std::invalid_argument("speq_markers_add_reads_device: null buffer");
    if (!m) throw std::invalid_argument("speq_markers_add_reads_device: null handle");
    if (n_reads == 0) return;
    speq_device_index* d = m->dev;
    DeviceGuard g(d->device);
    const uint32_t k = m->params.k;
    const DevView v = speq::search_view(d, k);
    const uint64_t blocks = std::min<uint64_t>((n_reads + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, 16384u);
    hipLaunchKernelGGL(k_marker_reads, dim3((uint32_t)blocks), dim3(BLOCK_THREADS),
                       (size_t)WAVES_PER_BLOCK * wave_bytes(k), st, v, d_seq, d_qual, d_offsets, n_reads, k,
                       m->params.phred_cutoff, m->d_depth.get());
    HIP_OK(hipGetLastError());
}

void add_host_impl(speq_markers* m, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                   uint64_t n_reads) {
    const char* who = "speq_markers_add_reads";
    // (the handle last: every check of the arrays is made before anything of the device is touched)
    if (n_reads > 0 && !offsets) throw std::invalid_argument(std::string(who) + ": null offsets");
    speq::check_host_reads(who, seq, qual, offsets, n_reads);
    if (!m) throw std::invalid_argument(std::string(who) + ": null handle");
    if (n_reads == 0) return;
    speq_device_index* d = m->dev;
    DeviceGuard g(d->device);
    // (the staging buffers go with the batch; nothing is copied back)
    for_staged_batches(who, d, seq, qual, offsets, n_reads, 1,
                       [&](const uint8_t* d_seq, const uint8_t* d_qual, const uint64_t* d_off, uint64_t, uint64_t n) {
                           add_device_impl(m, d_seq, d_qual, d_off, n, d->stream);
                       });
}

void finalize_impl(speq_markers* m, speq_marker_cov* out) {
    if (!m) throw std::invalid_argument("speq_markers_finalize: null handle");
    if (!out) throw std::invalid_argument("speq_markers_finalize: null output");
    speq_device_index* d = m->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());  // the adds of every stream of the device have completed
    const uint32_t G = m->G;
    const DevPtr<> cov = DevPtr<>::alloc((size_t)G * sizeof(speq_marker_cov), "speq_markers_finalize");
    hipStream_t st = d->stream;
    SyncOnExit sync(st);
    HIP_OK(hipMemsetAsync(cov.get(), 0, (size_t)G * sizeof(speq_marker_cov), st));
    const DevView v = speq::search_view(d, m->params.k);
    auto* o = static_cast<unsigned long long*>(cov.get());
    if (G <= LDS_TALLY_GROUPS)
        hipLaunchKernelGGL(k_marker_fold<true>, dim3(std::min(grid_1d(m->n), 2048u)), dim3(256), tally_bytes(G), st, v,
                           m->d_depth.get(), o);
    else
        hipLaunchKernelGGL(k_marker_fold<false>, dim3(grid_1d(m->n)), dim3(256), 0, st, v, m->d_depth.get(), o);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(out, cov.get(), (size_t)G * sizeof(speq_marker_cov), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
}

void list_impl(speq_markers* m, uint64_t* n_markers, uint32_t* lo, uint32_t* group, uint32_t* depth) {
    if (!m) throw std::invalid_argument("speq_markers_list: null handle");
    speq_device_index* d = m->dev;
    DeviceGuard g(d->device);
    HIP_OK(hipDeviceSynchronize());
    const uint64_t n = m->n;
    std::vector<uint32_t> w(n), grp;
    HIP_OK(hipMemcpy(w.data(), m->d_depth.get(), n * 4, hipMemcpyDeviceToHost));
    if (group) {
        const DevPtr<uint32_t> dg = DevPtr<uint32_t>::alloc(n, "speq_markers_list");
        SyncOnExit sync(d->stream);
        hipLaunchKernelGGL(k_marker_groups, dim3(grid_1d(n)), dim3(256), 0, d->stream,
                           speq::search_view(d, m->params.k), m->d_depth.get(), dg.get());
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(d->stream));
        grp.resize(n);
        HIP_OK(hipMemcpy(grp.data(), dg.get(), n * 4, hipMemcpyDeviceToHost));
    }
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!(w[i] & MARK)) continue;
        if (lo) lo[c] = (uint32_t)i;
        if (group) group[c] = grp[i];
        if (depth) depth[c] = w[i] & ~MARK;
        ++c;
    }
    if (n_markers) *n_markers = c;
}

}  // namespace

static_assert(sizeof(speq_marker_cov) == 96, "speq_marker_cov is twelve u64 words");

extern "C" {

int speq_markers_create(speq_device_index* d, const speq_scan_params* params, speq_markers** out) {
    return speq::guarded_nomem([&] { create_impl(d, params, out); });
}

int speq_markers_add_reads_device(speq_markers* m, const uint8_t* d_seq, const uint8_t* d_qual,
                                  const uint64_t* d_offsets, uint64_t n_reads, void* stream) {
    return speq::guarded_nomem([&] { add_device_impl(m, d_seq, d_qual, d_offsets, n_reads, static_cast<hipStream_t>(stream)); });
}

int speq_markers_add_reads(speq_markers* m, const uint8_t* seq, const uint8_t* qual, const uint64_t* offsets,
                           uint64_t n_reads) {
    return speq::guarded_nomem([&] { add_host_impl(m, seq, qual, offsets, n_reads); });
}

int speq_markers_finalize(speq_markers* m, speq_marker_cov* out) {
    return speq::guarded_nomem([&] { finalize_impl(m, out); });
}

int speq_markers_list(speq_markers* m, uint64_t* n_markers, uint32_t* lo, uint32_t* group, uint32_t* depth) {
    return speq::guarded_nomem([&] { list_impl(m, n_markers, lo, group, depth); });
}

void speq_markers_free(speq_markers* m) { delete m; }

}  // extern "C"
