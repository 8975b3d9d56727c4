// Decode of one staged 16-base chunk (k_scan_ax's refill, ax_scan.hip stage_decode): ASCII bases and Phred+33 quality
// bytes -> 2-bit codes, bad-base bits, quality-change bits. DESIGN.md §4s.
// Host and device: the device side takes gfx950's one-instruction forms (v_perm_b32, v_dot4_u32_u8), the host side
// plain C++ of the same meaning, so tests/ax_decode_check.cpp runs the very formulas of the kernel. Includes nothing
// of ROCm: compiles with plain g++.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AXD_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define AXD_FN inline
#endif

namespace speq_dev {

// byte j of the result = byte (sel's byte j, in 0..3) of tab (v_perm_b32 with the table as its low source)
AXD_FN uint32_t axd_perm4(uint32_t tab, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, tab, sel);
#else
    uint32_t r = 0;
    for (int j = 0; j < 4; ++j) r |= ((tab >> (8u * ((sel >> (8 * j)) & 3u))) & 0xFFu) << (8 * j);
    return r;
#endif
}
// acc + the sum over the four bytes of a's byte times b's byte (v_dot4_u32_u8, no clamp)
AXD_FN uint32_t axd_udot4(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int j = 0; j < 4; ++j) acc += ((a >> (8 * j)) & 0xFFu) * ((b >> (8 * j)) & 0xFFu);
    return acc;
#endif
}
// top bit of every byte of v that is not zero (exact: no carry between bytes); the other bits are not defined
AXD_FN uint32_t axd_nonzero_top(uint32_t v) { return ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v; }

// The quality filter of a scan as the decode takes it: a base fails iff clamp(byte - 33, 0, 41) <= cutoff, a byte of
// 128 or more counting as 41. qt4: the largest failing byte (at most 0x7F) in all four bytes; allbad: 0x80 in every
// byte when every base fails (cutoff >= 41), else 0.
AXD_FN uint32_t axd_qt4(uint32_t cutoff) {
    const uint32_t qt = cutoff > 0x7Fu - 33u ? 0x7Fu : 33u + cutoff;
    return qt * 0x01010101u;
}
AXD_FN uint32_t axd_allbad(uint32_t cutoff) { return cutoff >= 41u ? 0x80808080u : 0u; }

// One chunk: sd = its 16 base bytes, qd = its 16 quality bytes (little-endian dwords: base 4 i + j is byte j of dword
// i); qprev = the quality byte before the chunk (LOCAL only).
//   cw   2-bit codes, base b at bits 2 b: ((x >> 1) ^ (x >> 2)) & 3 of the lower-cased byte x (a c g t/u -> 0 1 2 3;
//        every other byte keeps the code its bits give)
//   bad  bit b: base b is none of ACGTUacgtu, or fails the quality filter
//   chb  (LOCAL, else 0) bit b: quality byte b differs from the byte before it
template <bool LOCAL>
AXD_FN void ax_decode_chunk(const uint32_t (&sd)[4], const uint32_t (&qd)[4], uint32_t qt4, uint32_t allbad,
                            uint32_t qprev, uint32_t& cw, uint32_t& bad, uint32_t& chb) {
    uint32_t c = 0, bl = 0, bh = 0, hl = 0, hh = 0;
    uint32_t qp = qprev << 24;  // the previous dword (its top byte is the previous quality)
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 4; ++i) {
        const uint32_t x = sd[i] | 0x20202020u;  // lower case
        const uint32_t c4 = ((x >> 1) ^ (x >> 2)) & 0x03030303u;
        c |= axd_udot4(c4, 0x40100401u, 0u) << (8 * i);  // four codes -> one byte
        const uint32_t canon = axd_perm4(0x74676361u, c4);  // the letter of that code
        const uint32_t x2 = x & ~((x >> 4) & 0x01010101u);  // u -> t (no other byte becomes a, c, g or t)
        const uint32_t nzb = axd_nonzero_top(x2 ^ canon);   // top bits: not ACGTU
        const uint32_t y = qd[i];
        const uint32_t badq = (((0x80808080u | qt4) - (y & 0x7F7F7F7Fu)) & ~y) | allbad;  // top bits: y <= qt, y < 128
        const uint32_t f = ((nzb | badq) >> 7) & 0x01010101u;
        // four flags -> four bits, two dwords per accumulator (the weights of the second still fit a byte)
        if (i == 0) bl = axd_udot4(f, 0x08040201u, 0u);
        if (i == 1) bl = axd_udot4(f, 0x80402010u, bl);
        if (i == 2) bh = axd_udot4(f, 0x08040201u, 0u);
        if (i == 3) bh = axd_udot4(f, 0x80402010u, bh);
        if (LOCAL) {
            const uint32_t prev = (y << 8) | (qp >> 24);
            const uint32_t g = (axd_nonzero_top(y ^ prev) >> 7) & 0x01010101u;
            if (i == 0) hl = axd_udot4(g, 0x08040201u, 0u);
            if (i == 1) hl = axd_udot4(g, 0x80402010u, hl);
            if (i == 2) hh = axd_udot4(g, 0x08040201u, 0u);
            if (i == 3) hh = axd_udot4(g, 0x80402010u, hh);
            qp = y;
        }
    }
    cw = c;
    bad = bl | (bh << 8);
    chb = hl | (hh << 8);
}

}  // namespace speq_dev
