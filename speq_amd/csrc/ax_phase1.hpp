// Phase-1 arithmetic of k_scan_ax (ax_scan.hip) with the instructions the result does not need taken out: the first
// mismatch of a run in one pass. DESIGN.md §4u.
// Host and device: the device side takes gfx950's one-instruction forms (v_alignbit_b32, v_ffbl_b32, v_add_u32 clamp),
// the host side plain C++ of the same meaning, so tests/ax_phase1_check.cpp runs the very formulas of the kernel.
// Includes nothing of ROCm: compiles with plain g++.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define AXP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define AXP_FN inline
#endif

namespace speq_dev {

constexpr uint32_t AXP_CMPD = 10;            // 16-base dwords one run compares (AX_CMP / 16)
constexpr uint32_t AXP_NONE = 0xFFFFFFFFu;   // no set bit

// ({hi, lo} >> (s & 31))[31:0]
AXP_FN uint32_t axp_alignbit(uint32_t hi, uint32_t lo, uint32_t s) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    s &= 31u;
    return s ? (lo >> s) | (hi << (32u - s)) : lo;
#endif
}
// index of the lowest set bit; of 0: AXP_NONE. That is v_ffbl_b32 as the hardware defines it, and the host says so
// explicitly. (The instruction by name: written as `x ? ctz(x) : -1` the compiler does not use its result for 0 and
// adds a compare and a select per call.)
AXP_FN uint32_t axp_ffbl(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x ? (uint32_t)__builtin_ctz(x) : AXP_NONE;
#endif
}
// min(a + b, 2^32 - 1)
AXP_FN uint32_t axp_add_sat(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_elementwise_add_sat(a, b);
#else
    const uint32_t r = a + b;
    return r < a ? 0xFFFFFFFFu : r;
#endif
}
AXP_FN uint32_t axp_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// First base at which a read differs from the text over the next cl <= 160 bases, else cl.
//   T    the text's 2-bit dwords from the granule of the run's text position p: 16 bases each (of granule g: T[2 g],
//        T[2 g + 1]); the run starts at base s5 = p & 31 of T
//   rw   the read's 2-bit dwords from the dword of its slot position; the run starts at bit rsh = 2 (position & 15)
// Dwords past cl bases may hold anything: a difference there only counts as "none before cl". One v_ffbl_b32 per dword
// (0xFFFFFFFF for equal dwords), a saturating add of the dword's first bit and a minimum over all, instead of a
// compare and a select per dword: the lowest differing bit of the 320, halved, is the base.
AXP_FN uint32_t axp_first_mismatch(const uint32_t (&T)[AXP_CMPD + 2], const uint32_t (&rw)[AXP_CMPD + 1], uint32_t s5,
                                   uint32_t rsh, uint32_t cl) {
    const uint32_t q16 = s5 >> 4, tsh = 2u * (s5 & 15u);
    uint32_t tq[AXP_CMPD + 1];  // the text's dwords from the one that holds base s5
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t i = 0; i <= AXP_CMPD; ++i) tq[i] = q16 ? T[i + 1] : T[i];
    uint32_t f = AXP_NONE;
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < AXP_CMPD; ++i) {
        const uint32_t x = axp_alignbit(tq[i + 1], tq[i], tsh) ^ axp_alignbit(rw[i + 1], rw[i], rsh);
        const uint32_t b = axp_ffbl(x);
        f = axp_min(f, i == 0 ? b : axp_add_sat(b, 32u * i));
    }
    return axp_min(f >> 1, cl);
}

}  // namespace speq_dev
